"""The sparse embedding update kernels (csrc/embed_optim.hip) on the GPU:
bit-equality with FusedEmbeddingOptimizer's torch-op fallback at the shapes
where the 16-position chunking can go wrong, the run sums on rounded values,
the absence of any dense buffer and the EmbeddingMLP wiring."""

import functools

import pytest
import torch

from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from ray_shuffling_data_loader_amd.models.mlp import EmbeddingMLP
from test_fused_embedding_cpu import exact_dout, make_indices, make_tables
from test_fused_embedding_gpu import (  # noqa: F401  (regime: a fixture)
    REGIMES,
    assert_within_fp32_bound,
    regime,
)
from test_fused_embedding_optim_cpu import KINDS, make_opt, run_step

pytestmark = pytest.mark.gpu

DEV = "cuda"


def check_bit_equal(kind, cards, D, B, index_fn):
    """Three steps, fresh indices each: GPU tables and state == the
    fallback's on CPU copies of the same inputs."""
    cpu = make_tables(cards, D, "cpu")
    gpu = [w.detach().to(DEV).requires_grad_() for w in cpu]
    opts = make_opt(kind, cpu), make_opt(kind, gpu)
    for step in range(3):
        idx = index_fn(step)
        dout = exact_dout(B, len(cards) * D, "cpu", seed=50 + step)
        run_step(opts[0], idx, cpu, dout)
        run_step(opts[1], [x.to(DEV) for x in idx], gpu, dout.to(DEV))
    for t, (a, b) in enumerate(zip(cpu, gpu)):
        assert torch.equal(a.detach(), b.detach().cpu()), f"table {t}"
        for s in opts[0].state[t]:
            assert torch.equal(opts[0].state[t][s],
                               opts[1].state[t][s].cpu()), f"state {t}"
    assert opts[1].step_count == 3


def seeded(B, cards):
    return lambda step: make_indices(B, cards, "cpu", seed=step)


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
@pytest.mark.parametrize("card", (1, 3, 17, 257, 5000))
@pytest.mark.parametrize("B", (1, 15, 16, 17, 97, 1000))
@pytest.mark.parametrize("kind", KINDS)
def test_bit_equal_to_fallback(kind, B, card, regime):
    cards = (card, 40)
    check_bit_equal(kind, cards, 16, B, seeded(B, cards))


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
@pytest.mark.parametrize("D", (8, 32))
@pytest.mark.parametrize("kind", KINDS)
def test_bit_equal_other_widths(kind, D, regime):
    cards = (33, 300, 5000)
    check_bit_equal(kind, cards, D, 1000, seeded(1000, cards))


RUN_SHAPES = {  # B and the indices of one table of B rows
    # a permutation: every run has length 1
    "unit": (1000, lambda step: [torch.randperm(
        1000, generator=torch.Generator().manual_seed(step))]),
    # every key change sits on a chunk boundary
    "boundary": (64, lambda step: [torch.arange(64) // 16]),
    # a single run of length B
    "one": (1000, lambda step: [torch.full((1000,), 7)]),
}


@pytest.mark.parametrize("regime", REGIMES[:1], indirect=True)
@pytest.mark.parametrize("runs", sorted(RUN_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_bit_equal_run_shapes(kind, runs, regime):
    B, index_fn = RUN_SHAPES[runs]
    check_bit_equal(kind, (B,), 16, B, index_fn)


@pytest.mark.parametrize("regime", REGIMES[:2], indirect=True)
def test_run_sums_on_rounded_values(regime):
    """sgd with lr = 1 on zero tables: p' = -g exactly."""
    B, D, cards = 1000, 16, (3, 300, 5000)
    idx = make_indices(B, cards, DEV)
    g = torch.Generator().manual_seed(4)
    dout = torch.randn(B, len(cards) * D, generator=g).bfloat16().to(DEV)
    runs = []
    for _ in range(2):
        tables = [torch.zeros(c, D, device=DEV).requires_grad_()
                  for c in cards]
        opt = fe.FusedEmbeddingOptimizer(tables, kind="sgd", lr=1.0)
        run_step(opt, idx, tables, dout)
        runs.append([-w.detach() for w in tables])
    assert_within_fp32_bound(runs[0], idx, runs[0], dout)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_no_dense_buffer():
    """O(B * T * D) bytes, where a dense gradient would be 128 MB."""
    B, D, card = 1000, 16, 2_000_000
    tables = [torch.zeros(card, D, device=DEV).requires_grad_()]
    idx = make_indices(B, (card,), DEV)
    dout = exact_dout(B, D, DEV)
    opt = fe.FusedEmbeddingOptimizer(tables, kind="sgd")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run_step(opt, idx, tables, dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak bytes over baseline", peak)
    assert peak < card * D * 4 // 8
    assert tables[0].grad is None and tables[0].detach().any()


def test_embedding_mlp_wiring():
    B, cards = 1000, (3, 300, 5000)
    torch.manual_seed(5)
    model = EmbeddingMLP(
        cards, fused_embedding=True,
        embedding_optimizer=functools.partial(
            fe.FusedEmbeddingOptimizer, kind="adagrad", lr=0.1),
    ).to(DEV)
    opt = model.embedding_optimizer
    tables = [e.weight for e in model.embeddings]
    assert all(a is b for a, b in zip(opt.tables, tables))
    before = [w.detach().clone() for w in tables]
    versions = [w._version for w in tables]
    idx = [x[:, None] for x in make_indices(B, cards, DEV)]
    target = torch.randn(B, 1, device=DEV)
    with torch.autocast("cuda", torch.bfloat16):
        loss = torch.nn.functional.mse_loss(model(idx), target)
    loss.backward()
    opt.step()
    for t, (w, w0, v) in enumerate(zip(tables, before, versions)):
        assert w.grad is None and w._version > v
        assert not torch.equal(w.detach(), w0)
        assert opt.state[t]["sum"].device == w.device
    assert all(p.grad is not None for p in model.mlp.parameters())
