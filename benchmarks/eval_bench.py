"""Per-batch cost of the forward-only evaluation path against the training
forward, same process, same build (models/fused_eval.py).

  (a) eval_update   FusedEvaluator.update(x, target): x swizzle + eval
                    chain + eval_accumulate (3 launches at steady state;
                    the weight stage is cached)
  (b) train_fwd     hip.fwd_chain_bf16(..., target=, xt_out=): the
                    training forward with all its emissions (a1^T/a2^T
                    fragments, mask words, a3, dy, both x layouts); this
                    binding also re-swizzles the weights per call

With ``--task binary`` the variants are instead
  (a) eval_regression   the regression evaluator, as above
  (b) eval_binary       FusedEvaluator(task="binary").update on a model
                        whose logits are spread like a trained one's
                        (std ~2): the AUC histogram's atomics scatter
  (c) eval_binary_const the same on a constant-logit model (zero head
                        weights): every row of a class adds to ONE
                        histogram bin, the atomic hot-spot worst case
  (d) eval_binary_noauc (b) with auc=False: no histogram at all
all on 0/1 labels, in the same run.

The variants alternate inside one timed loop; every call is bracketed
by device events and the medians are taken after one final synchronise.
Seeded; needs a GPU (no fallback). Prints one JSON line.

  python benchmarks/eval_bench.py --rows-per-batch 250000 --iters 50
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


def binary_main(args, model, x) -> None:
    import copy

    import torch

    from ray_shuffling_data_loader_amd.models.fused_eval import (
        FusedEvaluator,
    )
    from ray_shuffling_data_loader_amd.models.fused_step import _layers

    M = x.shape[0]
    # a trained-looking spread: scale the head so the logits have std ~2
    ev0 = FusedEvaluator(model)
    with torch.no_grad():
        std = ev0.predict(x).std().item()
        _layers(model)[3].weight.mul_(2.0 / max(std, 1e-6))
        const = copy.deepcopy(model)
        _layers(const)[3].weight.zero_()
    logits = ev0.predict(x)
    labels = torch.bernoulli(torch.sigmoid(logits))
    evs = {
        "eval_regression": FusedEvaluator(model),
        "eval_binary": FusedEvaluator(model, task="binary"),
        "eval_binary_const": FusedEvaluator(const, task="binary"),
        "eval_binary_noauc": FusedEvaluator(model, task="binary",
                                            auc=False),
    }
    variants = [
        (name, (lambda e=e: e.update(x, labels))) for name, e in evs.items()
    ]
    ms = time_variants(variants, args)
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {
        "bench": "eval_bench",
        "task": "binary",
        "rows_per_batch": M,
        "iters": args.iters,
        "warmup": args.warmup,
        "seed": args.seed,
        "logit_std": round(logits.std().item(), 4),
    }
    for name in evs:
        out[name + "_ms_median"] = round(med[name], 5)
        out[name + "_ms_min_max"] = [round(ms[name][0], 5),
                                     round(ms[name][-1], 5)]
    for name in ("eval_binary", "eval_binary_const", "eval_binary_noauc"):
        out[name + "_over_regression"] = round(
            med[name] / med["eval_regression"], 4)
    m = evs["eval_binary"].compute()
    mc = evs["eval_binary_const"].compute()
    out.update({
        "eval_rows_seen": m["rows"],
        "eval_logloss": m["logloss"],
        "eval_auc": m["auc"],
        "const_logloss": mc["logloss"],
        "const_auc": mc["auc"],
    })
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows-per-batch", type=int, default=250000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--task", choices=["regression", "binary"],
                    default="regression")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU")
    from ray_shuffling_data_loader_amd.models.fused_eval import (
        FusedEvaluator,
    )
    from ray_shuffling_data_loader_amd.models.fused_step import (
        _layers,
        _weight_buffers,
    )
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    hip = _load_hip()
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    M = args.rows_per_batch
    model = TabularMLP(100).to(dev)
    x = torch.randn(M, 100, device=dev).bfloat16()
    target = torch.randn(M, 1, device=dev)
    if args.task == "binary":
        return binary_main(args, model, x)

    ev = FusedEvaluator(model)
    lin = _layers(model)
    buf = _weight_buffers(model, lin)
    biases = [m.bias.detach() for m in lin]
    mchunks = 2 * ((M + 31) // 32)
    xt = torch.empty(4 * mchunks * 512, dtype=torch.bfloat16, device=dev)

    def eval_update():
        ev.update(x, target)

    def train_fwd():
        hip.fwd_chain_bf16(
            x, buf["W1p"], biases[0], buf["W2"], biases[1], buf["W3"],
            biases[2], buf["w4"], biases[3], target=target, xt_out=xt,
        )

    variants = [("eval_update", eval_update), ("train_fwd", train_fwd)]
    ms = time_variants(variants, args)
    med = {name: statistics.median(v) for name, v in ms.items()}
    metrics = ev.compute()
    print(json.dumps({
        "bench": "eval_bench",
        "rows_per_batch": M,
        "iters": args.iters,
        "warmup": args.warmup,
        "seed": args.seed,
        "eval_update_ms_median": round(med["eval_update"], 5),
        "train_fwd_ms_median": round(med["train_fwd"], 5),
        "eval_over_train_fwd": round(
            med["eval_update"] / med["train_fwd"], 4),
        "eval_update_ms_min_max": [round(ms["eval_update"][0], 5),
                                   round(ms["eval_update"][-1], 5)],
        "train_fwd_ms_min_max": [round(ms["train_fwd"][0], 5),
                                 round(ms["train_fwd"][-1], 5)],
        "eval_launches_per_batch": 3,
        "eval_rows_seen": metrics["rows"],
        "eval_mse": metrics["mse"],
    }))


if __name__ == "__main__":
    main()
