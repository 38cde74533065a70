"""Cost of a whole training step, update included, with the optimizer
outside and inside the fused step (models/fused_optim.py), same process,
same build, at the bench shape:

  A, A'  ``fused_step`` + ``torch.optim.SGD(momentum=0.9, fused=True).step()``
         — the path without ``optimizer=``; listed twice, so |A - A'| is
         the run-to-run spread the comparison has to clear
  B      ``fused_step(optimizer=FusedOptimizer("sgd", momentum=0.9))``
  C      ``fused_step(optimizer=FusedOptimizer("adamw"))``

Every arm trains its own copy of one seeded model on the same batch. The
arms alternate inside one timed loop (A, B, C, A'); every call is
bracketed by device events and the medians are taken after one final
synchronise. Seeded; needs a GPU (no fallback). Prints one JSON line.

  python benchmarks/step_optim_bench.py --rows-per-batch 250000 --iters 50
"""

import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows-per-batch", type=int, default=250000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("step_optim_bench needs a GPU")
    from ray_shuffling_data_loader_amd.models.fused_optim import (
        FusedOptimizer,
    )
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    if not getattr(_load_hip(), "STEP_OPTIM", 0):
        raise SystemExit("step_optim_bench needs an extension with "
                         "STEP_OPTIM")
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    M = args.rows_per_batch
    base = TabularMLP(100).to(dev)
    x = torch.randn(M, 100, device=dev).bfloat16()
    target = torch.bernoulli(torch.full((M, 1), 0.5, device=dev))

    losses = {}

    def torch_arm(name):
        model = copy.deepcopy(base)
        opt = torch.optim.SGD(model.parameters(), lr=args.lr, momentum=0.9,
                              fused=True)

        def fn():
            losses[name] = fused_step(model, x, target)
            opt.step()
        return fn

    def fused_arm(name, kind, **kw):
        model = copy.deepcopy(base)
        opt = FusedOptimizer(model, kind, lr=args.lr, **kw)

        def fn():
            losses[name] = fused_step(model, x, target, optimizer=opt)
        return fn

    variants = [
        ("A", torch_arm("A")),
        ("B", fused_arm("B", "sgd", momentum=0.9)),
        ("C", fused_arm("C", "adamw")),
        ("A2", torch_arm("A2")),
    ]
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
    ms = {
        name: sorted(a.elapsed_time(b) for a, b in evs)
        for name, evs in events.items()
    }
    med = {name: statistics.median(v) for name, v in ms.items()}

    def spread(v):
        # interquartile range of one arm's samples
        q = statistics.quantiles(v, n=4)
        return q[2] - q[0]

    run_spread = abs(med["A"] - med["A2"])
    out = {
        "bench": "step_optim_bench",
        "rows_per_batch": M,
        "iters": args.iters,
        "warmup": args.warmup,
        "seed": args.seed,
        "lr": args.lr,
        "torch_sgd_step_ms_median": round(med["A"], 5),
        "torch_sgd_again_step_ms_median": round(med["A2"], 5),
        "run_to_run_spread_ms": round(run_spread, 5),
        "fused_sgd_step_ms_median": round(med["B"], 5),
        "fused_adamw_step_ms_median": round(med["C"], 5),
        "fused_sgd_over_torch_sgd": round(med["B"] / med["A"], 4),
        "fused_sgd_within_spread_or_faster":
            bool(med["B"] <= med["A"] + run_spread),
    }
    for name, key in (("A", "torch_sgd"), ("A2", "torch_sgd_again"),
                      ("B", "fused_sgd"), ("C", "fused_adamw")):
        out[f"{key}_step_ms_min_max"] = [round(ms[name][0], 5),
                                         round(ms[name][-1], 5)]
        out[f"{key}_step_ms_iqr"] = round(spread(ms[name]), 5)
        out[f"{key}_loss"] = float(losses[name])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
