"""The fused multi-table embedding kernels (csrc/embed.hip) on the GPU:
forward bytes against gather + cat + cast, both backward regimes against an
fp64 index_add_ (exactly where every order is exact, to the truncating-fp32
bound otherwise), and the EmbeddingMLP switch."""

import pytest
import torch

from ray_shuffling_data_loader_amd.data_generation import DATA_SPEC
from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from ray_shuffling_data_loader_amd.models.mlp import EmbeddingMLP
from test_fused_embedding_cpu import (
    backward_ref64,
    exact_dout,
    forward_ref,
    make_indices,
    make_tables,
    run_backward,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BATCHES = (1, 31, 33, 97, 1000)
SPEC_CARDS = [c for name, (_, c, _) in DATA_SPEC.items() if name != "labels"]
# _DENSE_MAX_ROWS: every table sorted / every table one-hot / the default
REGIMES = (0, 10**6, None)


@pytest.fixture
def regime(request, monkeypatch):
    if request.param is not None:
        monkeypatch.setattr(fe, "_DENSE_MAX_ROWS", request.param)
    return request.param


@pytest.mark.parametrize("D", (8, 16, 32))
@pytest.mark.parametrize("B", BATCHES)
def test_forward_bytes(B, D):
    cards = (3, 17, 5000)
    idx = make_indices(B, cards, DEV)
    tables = make_tables(cards, D, DEV)
    assert torch.equal(fe.fused_embedding(idx, tables), forward_ref(idx, tables))


@pytest.mark.parametrize("form", ("strided", "matrix", "spec"))
def test_forward_bytes_index_forms(form):
    cards = SPEC_CARDS if form == "spec" else (3, 17, 5000)
    idx = make_indices(97, cards, DEV)
    tables = make_tables(cards, 16, DEV)
    want = forward_ref(idx, tables)
    if form == "strided":  # stride-5 column views of a packed [B, 5] block
        block = torch.full((97, 5), -1, dtype=torch.int64, device=DEV)
        for t, x in enumerate(idx):
            block[:, 1 + t] = x
        given = [block[:, 1 + t] for t in range(3)]
        assert given[0].stride(0) == 5
    elif form == "matrix":
        given = torch.stack(idx, 1)
    else:
        given = [x[:, None] for x in idx]
    assert torch.equal(fe.fused_embedding(given, tables), want)


def check_exact(idx, tables, B):
    dout = exact_dout(B, len(tables) * tables[0].shape[1], DEV)
    grads = run_backward(idx, tables, dout)
    ref, cnt, _ = backward_ref64(idx, tables, dout)
    for g, r, n in zip(grads, ref, cnt):
        assert torch.equal(g.cpu(), r.float())
        assert not g.cpu()[n[:, 0] == 0].any()  # untouched rows: exact zeros
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 1


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
@pytest.mark.parametrize("card", (1, 3, 16, 17, 33, 256, 257, 5000))
@pytest.mark.parametrize("B", BATCHES)
def test_backward_exact(B, card, regime):
    cards = (card, 40)
    check_exact(make_indices(B, cards, DEV), make_tables(cards, 16, DEV), B)


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
@pytest.mark.parametrize("D", (8, 32))
def test_backward_exact_other_widths(D, regime):
    cards = (33, 300, 5000)
    check_exact(make_indices(1000, cards, DEV), make_tables(cards, D, DEV),
                1000)


@pytest.mark.parametrize("regime", REGIMES[:2], indirect=True)
@pytest.mark.parametrize("runs", ("one", "unit"))
def test_backward_exact_run_lengths(runs, regime):
    B = 1000
    if runs == "one":  # a single run of length B, one hot row
        idx = [torch.full((B,), 7, dtype=torch.int64, device=DEV)]
    else:  # a permutation: every run has length 1
        idx = [torch.randperm(B, generator=torch.Generator().manual_seed(3))
               .to(DEV)]
    check_exact(idx, make_tables((B,), 16, DEV), B)


def assert_within_fp32_bound(grads, idx, tables, dout):
    """|got - ref64| <= n_r * 2^-23 * S_r per element: 2^-23 is the unit
    roundoff of a truncating fp32 accumulator, which bounds every add of
    any summation order and of the MFMA's internal accumulation."""
    ref, cnt, mag = backward_ref64(idx, tables, dout)
    for g, r, n, s in zip(grads, ref, cnt, mag):
        err = (g.double().cpu() - r).abs()
        bound = n * 2.0**-23 * s
        print("max err", err.max().item(), "max bound", bound.max().item())
        assert (err <= bound).all()


@pytest.mark.parametrize("regime", REGIMES[:2], indirect=True)
def test_backward_rounded_values(regime):
    B, cards = 1000, (3, 300, 5000)
    idx = make_indices(B, cards, DEV)
    tables = make_tables(cards, 16, DEV)
    g = torch.Generator().manual_seed(4)
    dout = torch.randn(B, 48, generator=g).bfloat16().to(DEV)
    first = [x.clone() for x in run_backward(idx, tables, dout)]
    assert_within_fp32_bound(first, idx, tables, dout)
    again = run_backward(idx, tables, dout)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_embedding_mlp_fused_matches_default():
    B, cards = 1000, (3, 300, 5000)
    torch.manual_seed(5)
    plain = EmbeddingMLP(cards).to(DEV)
    fused = EmbeddingMLP(cards, fused_embedding=True).to(DEV)
    fused.load_state_dict(plain.state_dict())
    idx = [x[:, None] for x in make_indices(B, cards, DEV)]
    target = torch.randn(B, 1, device=DEV)
    seen = []
    fused.mlp[0].register_forward_pre_hook(
        lambda m, inp: inp[0].register_hook(seen.append) and None
    )
    with torch.autocast("cuda", torch.bfloat16):
        lp = torch.nn.functional.mse_loss(plain(idx), target)
        lf = torch.nn.functional.mse_loss(fused(idx), target)
    # one bf16 ulp of the concat feeding three layers
    torch.testing.assert_close(lf, lp, rtol=2.0**-7, atol=0)
    lf.backward()
    (dout,) = seen
    assert dout.dtype == torch.bfloat16 and dout.shape == (B, 48)
    tables = [e.weight for e in fused.embeddings]
    assert_within_fp32_bound([w.grad for w in tables], idx, tables, dout)
