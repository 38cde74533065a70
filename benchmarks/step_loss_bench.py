"""Cost of the fused train step under its two objectives, same process,
same build (models/fused_step.py): ``fused_step(loss="mse")`` against
``fused_step(loss="bce")`` at the bench shape.

Only the head epilogue of the forward chain differs between the two, so
the BCE step is expected inside the run-to-run spread of the MSE step.

The two variants alternate inside one timed loop on the same batch, the
same model and 0/1 labels (valid for both); every call is bracketed by
device events and the medians are taken after one final synchronise. No
optimizer step: the weights stay put, so both see the same work. Seeded;
needs a GPU (no fallback). Prints one JSON line.

  python benchmarks/step_loss_bench.py --rows-per-batch 250000 --iters 50
"""

import argparse
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
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("step_loss_bench needs a GPU")
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    M = args.rows_per_batch
    model = TabularMLP(100).to(dev)
    x = torch.randn(M, 100, device=dev).bfloat16()
    target = torch.bernoulli(torch.full((M, 1), 0.5, device=dev))

    losses = {}

    def step(name):
        def fn():
            losses[name] = fused_step(model, x, target, loss=name)
        return fn

    variants = [("mse", step("mse")), ("bce", step("bce"))]
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
        # interquartile range: the run-to-run spread the medians sit in
        q = statistics.quantiles(v, n=4)
        return q[2] - q[0]

    print(json.dumps({
        "bench": "step_loss_bench",
        "rows_per_batch": M,
        "iters": args.iters,
        "warmup": args.warmup,
        "seed": args.seed,
        "mse_step_ms_median": round(med["mse"], 5),
        "bce_step_ms_median": round(med["bce"], 5),
        "bce_over_mse": round(med["bce"] / med["mse"], 4),
        "mse_step_ms_min_max": [round(ms["mse"][0], 5),
                                round(ms["mse"][-1], 5)],
        "bce_step_ms_min_max": [round(ms["bce"][0], 5),
                                round(ms["bce"][-1], 5)],
        "mse_step_ms_iqr": round(spread(ms["mse"]), 5),
        "bce_step_ms_iqr": round(spread(ms["bce"]), 5),
        "mse_loss": float(losses["mse"]),
        "bce_loss": float(losses["bce"]),
    }))


if __name__ == "__main__":
    main()
