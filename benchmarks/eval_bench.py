"""Per-batch cost of the forward-only evaluation path against the training
forward, same process, same build (models/fused_eval.py).

  (a) eval_update   FusedEvaluator.update(x, target): x swizzle + eval
                    chain + eval_accumulate (3 launches at steady state;
                    the weight stage is cached)
  (b) train_fwd     hip.fwd_chain_bf16(..., target=, xt_out=): the
                    training forward with all its emissions (a1^T/a2^T
                    fragments, mask words, a3, dy, both x layouts); this
                    binding also re-swizzles the weights per call

The two variants alternate inside one timed loop; every call is bracketed
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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows-per-batch", type=int, default=250000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
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
