"""Forward + backward of the 19 DATA_SPEC embedding columns at the bench
batch: EmbeddingMLP's eager path against the fused lookup
(models/fused_embedding.py), same process, same build.

  (a) eager   19 x (clamp_min, %, nn.Embedding) + torch.cat, fp32 concat,
              backward = 19 embedding_dense_backward calls
  (b) fused   fused_embedding: one forward launch (bf16 concat), backward
              = one-hot MFMA kernel + fold for the small tables, one stable
              sort + run sums for the large ones; one variant per value of
              --dense-max (the _DENSE_MAX_ROWS threshold between the two)

Both arms get the gradient of the concat handed in (fp32 for the eager
concat, the same values in bf16 for the fused one) and leave dense fp32
``.grad`` on every table. The variants alternate inside one timed loop;
every call is bracketed by device events and the medians are taken after
one final synchronise. Seeded; needs a GPU (no fallback). Prints one JSON
line.

  python benchmarks/embed_bench.py --rows-per-batch 250000 --iters 30
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eval_bench import time_variants  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows-per-batch", type=int, default=250000)
    ap.add_argument("--embed-dim", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-max", type=int, nargs="+", default=None,
                    help="_DENSE_MAX_ROWS values to time (default: the "
                    "module's)")
    ap.add_argument("--only", choices=["eager", "fused"], default=None,
                    help="run one arm only (kernel traces)")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("embed_bench needs a GPU")
    from ray_shuffling_data_loader_amd.data_generation import DATA_SPEC
    from ray_shuffling_data_loader_amd.models import fused_embedding as fe
    from ray_shuffling_data_loader_amd.models.mlp import EmbeddingMLP

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    B, D = args.rows_per_batch, args.embed_dim
    cards = [c for name, (_, c, _) in DATA_SPEC.items() if name != "labels"]
    model = EmbeddingMLP(cards, embed_dim=D).to(dev)
    tables = [e.weight for e in model.embeddings]
    # the loader's "views" output: [B, 1] columns, uniform over each range
    idx = [torch.randint(0, c, (B, 1), device=dev) for c in cards]
    dout16 = torch.randn(B, len(cards) * D, device=dev).bfloat16()
    dout32 = dout16.float()

    def eager():
        for w in tables:
            w.grad = None
        out = torch.cat(
            [
                emb(x.clamp_min(0).squeeze(-1) % emb.num_embeddings)
                for emb, x in zip(model.embeddings, idx)
            ],
            dim=1,
        )
        out.backward(dout32)

    def fused_at(dense_max):
        def run():
            fe._DENSE_MAX_ROWS = dense_max
            for w in tables:
                w.grad = None
            fe.fused_embedding(idx, tables).backward(dout16)
        return run

    sweep = args.dense_max or [fe._DENSE_MAX_ROWS]
    variants = []
    if args.only != "fused":
        variants.append(("eager", eager))
    if args.only != "eager":
        variants += [(f"fused_dense_max_{m}", fused_at(m)) for m in sweep]
    ms = time_variants(variants, args)
    med = {name: statistics.median(v) for name, v in ms.items()}

    # the two arms computed the same gradients (fp32 sums, other orders)
    worst = 0.0
    if args.only is None:
        eager()
        ref = [w.grad.clone() for w in tables]
        fused_at(sweep[0])()
        for w, r in zip(tables, ref):
            scale = r.abs().max().clamp_min(1e-30)
            worst = max(worst, ((w.grad - r).abs().max() / scale).item())
    out = {
        "bench": "embed_bench",
        "rows_per_batch": B,
        "embed_dim": D,
        "tables": len(cards),
        "iters": args.iters,
        "warmup": args.warmup,
        "seed": args.seed,
        "grad_max_rel_diff_vs_eager": worst,
    }
    for name in med:
        out[name + "_ms_median"] = round(med[name], 5)
        out[name + "_ms_min_max"] = [round(ms[name][0], 5),
                                     round(ms[name][-1], 5)]
        if name != "eager" and "eager" in med:
            out[name + "_over_eager"] = round(med[name] / med["eager"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
