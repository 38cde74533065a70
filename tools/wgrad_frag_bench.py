#!/usr/bin/env python3
"""Time the fragment-major wgrad path (wgrad_frag kernel + slab_reduce)
at the three flagship shapes. A/B the pinned-schedule variants with
RSDL_WGRAD_SCHED=1 (see profiles/r02/wgrad_sched_asm.md).

``--ab [ROUNDS]`` instead times the wgrad kernel ALONE (the raw slab
partials, no zero-fill and no slab_reduce), alternating the direct
kernel (variant 1) and the LDS-ring kernel (variant 2) in one process,
and applies the rule a per-shape default has to pass: every ring timing
below every direct timing, and the median difference at least three
times the larger within-variant spread. One JSON line per shape.

``--grouped [ROUNDS]`` times the step's three wgrad launches against the
one grouped launch that replaces them (wgrad_grouped_kernel), alternated
the same way; RSDL_WGRAD_GROUP_SLABS picks the split under test."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ray_shuffling_data_loader_amd.ops.shuffle_ops import (  # noqa: E402
    _WGRAD_FRAG_CFG,
    _load_hip,
    wgrad_frag,
)

SHAPES = [(512, 128), (256, 512), (128, 256)]  # (N, K) of dW1, dW2, dW3


def t(fn, iters=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def inputs(N, K, mchunks, dev="cuda"):
    # AT is dz^T [N-tiles][mchunks][512], BT is src^T.
    at = torch.randn(N // 32 * mchunks * 512, device=dev).bfloat16()
    bt = torch.randn(K // 32 * mchunks * 512, device=dev).bfloat16()
    return at, bt


def ab(M, rounds):
    hip = _load_hip()
    mchunks = 2 * ((M + 31) // 32)
    for N, K in SHAPES:
        nt_w, kt_w = _WGRAD_FRAG_CFG[(N, K)]
        at, bt = inputs(N, K, mchunks)
        us = {1: [], 2: []}
        nslabs = 0
        # round -1 is a discarded warm-up pair: the first timing after
        # the inputs are generated runs while the clocks still settle
        for r in range(-1, rounds):
            for v in (1, 2):
                def run():
                    return hip.wgrad_frag_partials_bf16(
                        at, bt, N, K, mchunks, nt_w, kt_w, variant=v)
                nslabs = run().shape[0]
                us_v = t(run) * 1e3
                if r >= 0:
                    us[v].append(us_v)
        # unique bytes: A^T + B^T fragments once (the re-reads by the
        # other output blocks of a slab are meant to hit in L2), plus
        # the fp32 partials written
        by = (at.numel() + bt.numel()) * 2 + nslabs * N * K * 4
        med = {v: statistics.median(us[v]) for v in us}
        spread = max(max(us[v]) - min(us[v]) for v in us)
        diff = med[1] - med[2]
        passes = max(us[2]) < min(us[1]) and diff >= 3 * spread
        print(json.dumps({
            "shape": [N, K], "tile": [nt_w, kt_w], "M": M,
            "direct_us": [round(x, 2) for x in us[1]],
            "lds_us": [round(x, 2) for x in us[2]],
            "direct_med_us": round(med[1], 2),
            "lds_med_us": round(med[2], 2),
            "direct_TBps": round(by / med[1] / 1e6, 2),
            "lds_TBps": round(by / med[2] / 1e6, 2),
            "bytes_MB": round(by / 1e6, 1),
            "median_diff_us": round(diff, 2),
            "max_spread_us": round(spread, 2),
            "lds_passes_rule": passes,
        }), flush=True)


def grouped(M, rounds):
    """The three wgrads as the step launches them at variant 0, alone (raw
    partials): three launches against the one grouped launch, alternated
    in one process; the same rule as ``ab``. One JSON line."""
    hip = _load_hip()
    mchunks = 2 * ((M + 31) // 32)
    ins = [inputs(N, K, mchunks) for N, K in SHAPES]
    cfg = [_WGRAD_FRAG_CFG[s] for s in SHAPES]

    def three():
        return [hip.wgrad_frag_partials_bf16(at, bt, N, K, mchunks, nt, kt)
                for (N, K), (at, bt), (nt, kt) in zip(SHAPES, ins, cfg)]

    def one():
        return hip.wgrad_grouped_partials_bf16(
            ins[0][0], ins[0][1], ins[1][0], ins[1][1], ins[2][0],
            ins[2][1], mchunks)

    arms = {"three": three, "grouped": one}
    us = {k: [] for k in arms}
    slabs = {k: [p.shape[0] for p in fn()] for k, fn in arms.items()}
    for r in range(-1, rounds):  # round -1: discarded warm-up pair
        for k, fn in arms.items():
            us_k = t(fn) * 1e3
            if r >= 0:
                us[k].append(us_k)
    in_by = sum(at.numel() + bt.numel() for at, bt in ins) * 2
    by = {k: in_by + sum(ns * N * K * 4
                         for ns, (N, K) in zip(slabs[k], SHAPES))
          for k in arms}
    med = {k: statistics.median(us[k]) for k in us}
    spread = max(max(us[k]) - min(us[k]) for k in us)
    diff = med["three"] - med["grouped"]
    passes = max(us["grouped"]) < min(us["three"]) and diff >= 3 * spread
    print(json.dumps({
        "M": M,
        "group_slabs": os.environ.get("RSDL_WGRAD_GROUP_SLABS", "default"),
        "three_slabs": slabs["three"], "grouped_slabs": slabs["grouped"],
        "three_us": [round(x, 2) for x in us["three"]],
        "grouped_us": [round(x, 2) for x in us["grouped"]],
        "three_med_us": round(med["three"], 2),
        "grouped_med_us": round(med["grouped"], 2),
        "three_bytes_MB": round(by["three"] / 1e6, 1),
        "grouped_bytes_MB": round(by["grouped"] / 1e6, 1),
        "three_TBps": round(by["three"] / med["three"] / 1e6, 2),
        "grouped_TBps": round(by["grouped"] / med["grouped"] / 1e6, 2),
        "median_diff_us": round(diff, 2),
        "max_spread_us": round(spread, 2),
        "grouped_passes_rule": passes,
    }), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ab", type=int, nargs="?", const=5, default=0,
                   metavar="ROUNDS")
    p.add_argument("--grouped", type=int, nargs="?", const=7, default=0,
                   metavar="ROUNDS")
    p.add_argument("--rows", type=int, default=250_000)
    args = p.parse_args()
    M = args.rows
    if args.ab:
        ab(M, args.ab)
        return
    if args.grouped:
        grouped(M, args.grouped)
        return
    mchunks = 2 * ((M + 31) // 32)
    print(f"RSDL_WGRAD_SCHED={os.environ.get('RSDL_WGRAD_SCHED', '0')}")
    for N, K in SHAPES:
        at, bt = inputs(N, K, mchunks)
        ms = t(lambda: wgrad_frag(at, bt, N, K, mchunks))
        by = (at.numel() + bt.numel()) * 2  # bf16 stream bytes
        print(
            f"wgrad_frag N={N:3d} K={K:3d}: {ms * 1e3:7.1f} us  "
            f"{by / ms / 1e6:6.0f} GB/s effective"
        )


if __name__ == "__main__":
    main()
