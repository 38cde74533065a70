"""CPU mirror of the fused multi-table embedding
(models/fused_embedding.py): the same forward bytes and the same exact-case
gradients as the HIP path is held to in test_fused_embedding_gpu.py, the
EmbeddingMLP switch and the DDP example's argument check."""

import importlib.util
import os

import pytest
import torch

from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from ray_shuffling_data_loader_amd.models.mlp import EmbeddingMLP

I64_MAX = torch.iinfo(torch.int64).max


def make_indices(B, cards, device, seed=0):
    """[B] int64 per table: values on both sides of [0, card), with the
    wrap's edge values in the leading rows (rotated per table so that B = 1
    meets a different one in each)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t, c in enumerate(cards):
        x = torch.randint(-10, 3 * c + 1, (B,), generator=g)
        edge = [-5, c, c + 1, 2**33 + 7, I64_MAX]
        edge = (edge[t % 5:] + edge[:t % 5])[:B]
        x[:len(edge)] = torch.tensor(edge)
        out.append(x.to(device))
    return out


def make_tables(cards, D, device, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [
        torch.randn(c, D, generator=g).to(device).requires_grad_()
        for c in cards
    ]


def exact_dout(B, width, device, seed=2):
    """Integers in [-8, 8] times 2^-3: exact in bf16, and with B < 2^21
    every partial sum is a multiple of 2^-3 below 2^21, exact in fp32 in
    any order."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-8, 9, (B, width), generator=g)
    return (k.float() / 8).bfloat16().to(device)


def forward_ref(idx, tables):
    return torch.cat(
        [
            w.detach()[x.reshape(-1).clamp_min(0) % w.shape[0]]
            for x, w in zip(idx, tables)
        ],
        1,
    ).bfloat16()


def backward_ref64(idx, tables, dout):
    """fp64 index_add_ per table (on the CPU), plus per element the count
    n_r of rows that hit it and the sum S_r of their |g|."""
    D = tables[0].shape[1]
    ref, cnt, mag = [], [], []
    for t, (x, w) in enumerate(zip(idx, tables)):
        c = w.shape[0]
        i = (x.reshape(-1).clamp_min(0) % c).cpu()
        g = dout[:, t * D:(t + 1) * D].double().cpu()
        ref.append(torch.zeros(c, D, dtype=torch.float64).index_add_(0, i, g))
        mag.append(
            torch.zeros(c, D, dtype=torch.float64).index_add_(0, i, g.abs())
        )
        cnt.append(torch.bincount(i, minlength=c).double()[:, None])
    return ref, cnt, mag


def run_backward(idx, tables, dout):
    for w in tables:
        w.grad = None
    fe.fused_embedding(idx, tables).backward(dout)
    return [w.grad for w in tables]


@pytest.mark.parametrize("B,D", [(1, 8), (33, 16), (97, 32)])
def test_cpu_mirror_forward_and_exact_backward(B, D):
    cards = (3, 17, 5000)
    idx = make_indices(B, cards, "cpu")
    tables = make_tables(cards, D, "cpu")
    out = fe.fused_embedding(idx, tables)
    assert out.dtype == torch.bfloat16
    assert torch.equal(out, forward_ref(idx, tables))
    # one [B, T] matrix and [B, 1] columns are the same lookup
    assert torch.equal(fe.fused_embedding(torch.stack(idx, 1), tables), out)
    assert torch.equal(
        fe.fused_embedding([x[:, None] for x in idx], tables), out
    )
    dout = exact_dout(B, len(cards) * D, "cpu")
    grads = run_backward(idx, tables, dout)
    ref, _, _ = backward_ref64(idx, tables, dout)
    for g, r in zip(grads, ref):
        assert g.dtype == torch.float32
        assert torch.equal(g, r.float())
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 1


def test_embedding_mlp_switch_keeps_state_dict():
    cards = (3, 17, 300)
    a = EmbeddingMLP(cards)
    b = EmbeddingMLP(cards, fused_embedding=True)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    idx = make_indices(31, cards, "cpu")
    assert b(idx).shape == a(idx).shape == (31, 1)


def test_train_ddp_rejects_fused_embedding_without_tabular():
    path = os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "examples", "ddp", "train_ddp.py",
    )
    spec = importlib.util.spec_from_file_location("_train_ddp_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit, match="--spec tabular"):
        mod.parse_args(["--fused-embedding"])
    args = mod.parse_args(["--fused-embedding", "--spec", "tabular"])
    assert args.fused_embedding
