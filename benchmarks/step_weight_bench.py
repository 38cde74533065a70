"""Cost of sample weights and pos_weight in the fused train step and the
evaluator, same process, same build (models/fused_step.py,
models/fused_eval.py), at the bench shape.

Step arms, all ``fused_step(loss="bce")`` on the same batch and model:
  bce             unweighted (fwd_chain_kernel, WEIGHTED = false: what the
                  step always ran)
  bce_w           ``sample_weight=w`` (fwd_chain_kernel, WEIGHTED = true)
  bce_w_pw        ``sample_weight=w, pos_weight=3`` (the pos_weight branch)
Evaluator arms, ``FusedEvaluator(task="binary").update`` on a model whose
logits are spread like a trained one's (std ~2):
  eval            unweighted, with the AUC histogram
  eval_w          ``weighted=True``, fixed-point histogram adds
  eval_noauc      unweighted, ``auc=False``
  eval_w_noauc    ``weighted=True, auc=False``

Only the head epilogue differs between the arms of a group and the
weighted ones read 4 bytes more per row (1 MB per 250k-row batch against
~450 MB of by-products), so each weighted arm is expected inside the
run-to-run spread of its unweighted one. The yardstick is the unweighted
arm of the same process, not an earlier run.

The step arms alternate inside one timed loop, then the evaluator arms in
another; every call is bracketed by device events and the medians are
taken after one final synchronise. No optimizer step: the weights stay
put. Seeded; needs a GPU (no fallback). Prints one JSON line.

  python benchmarks/step_weight_bench.py --rows-per-batch 250000 --iters 50
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_variants(variants, args):
    """Sorted per-call event times (ms) of the alternating variants."""
    import torch

    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name, _ in variants}
    for _ in range(args.iters):
        for name, fn in variants:
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events[name].append((a, b))
    torch.cuda.synchronize()
    return {
        name: sorted(a.elapsed_time(b) for a, b in evs)
        for name, evs in events.items()
    }


def _iqr(v):
    # interquartile range: the run-to-run spread the medians sit in
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows-per-batch", type=int, default=250000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("step_weight_bench needs a GPU")
    from ray_shuffling_data_loader_amd.models.fused_eval import (
        FusedEvaluator,
    )
    from ray_shuffling_data_loader_amd.models.fused_step import (
        _layers,
        fused_step,
    )
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    if not getattr(_load_hip(), "HEAD_WEIGHTS", 0):
        raise SystemExit("step_weight_bench needs the weighted heads")
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    M = args.rows_per_batch
    model = TabularMLP(100).to(dev)
    x = torch.randn(M, 100, device=dev).bfloat16()
    # a trained-looking spread: scale the head so the logits have std ~2
    ev0 = FusedEvaluator(model)
    with torch.no_grad():
        std = ev0.predict(x).std().item()
        _layers(model)[3].weight.mul_(2.0 / max(std, 1e-6))
    logits = ev0.predict(x)
    target = torch.bernoulli(torch.sigmoid(logits))
    # importance-style weights in (0, 4], fp32 [M], a tenth of them 0
    w = torch.rand(M, device=dev) * 4.0
    w[torch.rand(M, device=dev) < 0.1] = 0.0

    losses = {}

    def step(name, **kw):
        def fn():
            losses[name] = fused_step(model, x, target, loss="bce", **kw)
        return fn

    steps = [
        ("bce", step("bce")),
        ("bce_w", step("bce_w", sample_weight=w)),
        ("bce_w_pw", step("bce_w_pw", sample_weight=w, pos_weight=3.0)),
    ]
    ms = time_variants(steps, args)

    evs = {
        "eval": FusedEvaluator(model, task="binary"),
        "eval_w": FusedEvaluator(model, task="binary", weighted=True),
        "eval_noauc": FusedEvaluator(model, task="binary", auc=False),
        "eval_w_noauc": FusedEvaluator(model, task="binary", auc=False,
                                       weighted=True),
    }
    evals = [
        (name, (lambda e=e: e.update(x, target, w) if e.weighted
                else e.update(x, target)))
        for name, e in evs.items()
    ]
    ms.update(time_variants(evals, args))
    med = {name: statistics.median(v) for name, v in ms.items()}

    out = {
        "bench": "step_weight_bench",
        "rows_per_batch": M,
        "iters": args.iters,
        "warmup": args.warmup,
        "seed": args.seed,
        "logit_std": round(logits.std().item(), 4),
    }
    for name in ms:
        out[name + "_ms_median"] = round(med[name], 5)
        out[name + "_ms_min_max"] = [round(ms[name][0], 5),
                                     round(ms[name][-1], 5)]
        out[name + "_ms_iqr"] = round(_iqr(ms[name]), 5)
    out["bce_w_over_bce"] = round(med["bce_w"] / med["bce"], 4)
    out["bce_w_pw_over_bce"] = round(med["bce_w_pw"] / med["bce"], 4)
    out["eval_w_over_eval"] = round(med["eval_w"] / med["eval"], 4)
    out["eval_w_noauc_over_eval_noauc"] = round(
        med["eval_w_noauc"] / med["eval_noauc"], 4)
    for name in ("bce", "bce_w", "bce_w_pw"):
        out[name + "_loss"] = float(losses[name])
    m, mw = evs["eval"].compute(), evs["eval_w"].compute()
    out.update({
        "eval_rows_seen": m["rows"],
        "eval_logloss": m["logloss"],
        "eval_auc": m["auc"],
        "eval_w_weight_sum": mw["weight_sum"],
        "eval_w_logloss": mw["logloss"],
        "eval_w_auc": mw["auc"],
    })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
