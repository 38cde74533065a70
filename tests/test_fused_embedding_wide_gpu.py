"""The fused embedding kernels at D = 64 and 128 (csrc/embed.hip,
csrc/embed_optim.hip): the column-sliced one-hot backward, the 16- and
32-lane row groups of the sorted regime and the forward's rows of more than
one workgroup, held to the oracles of the narrow widths' tests."""

import pytest
import torch

import test_fused_embedding_order_cpu as oc
import test_fused_embedding_order_gpu as og
from _shuffle_cases import BF16, assert_same_bits
from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from ray_shuffling_data_loader_amd.ops import shuffle_ops
from test_fused_embedding_cpu import (
    exact_dout, forward_ref, make_indices, make_tables)
from test_fused_embedding_gpu import (  # noqa: F401  (regime: a fixture)
    REGIMES, check_exact, regime)
from test_fused_embedding_optim_cpu import KINDS
from test_fused_embedding_optim_gpu import check_bit_equal, seeded

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("D", (64, 128))]

DEV = "cuda"
CARDS = (3, 300, 5000)
ALL_REGIMES = pytest.mark.parametrize("regime", REGIMES, indirect=True)


def test_served(D):
    cards, B = (40, 5000), 33
    idx, tables = make_indices(B, cards, DEV), make_tables(cards, D, DEV)
    assert fe._kernels_serve(idx, tables)
    hip = shuffle_ops._load_hip()
    w = [t.detach().clone() for t in tables]
    out, widx = hip.embed_concat_fwd(idx, w, True)
    assert out.shape == (B, 2 * D) and widx.shape == (B, 2)
    dout = exact_dout(B, 2 * D, DEV)
    hip.embed_bwd_onehot(dout, widx, torch.zeros(40, D, device=DEV), [0],
                         [40], [0])
    keys, pos = fe._sorted_keys(widx, cards, [0, 40], [1])
    hip.embed_runs_update(dout, widx, keys, pos, [1], [40], w[1:], [],
                          hip.EMBED_SGD, 0.1, 0.0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", (1, 33, 1000))
def test_forward_bytes(B, D):
    cards = (3, 17, 5000)
    idx, tables = make_indices(B, cards, DEV), make_tables(cards, D, DEV)
    want = forward_ref(idx, tables)
    assert torch.equal(fe.fused_embedding(idx, tables), want)
    if B == 33:  # stride-5 column views of a packed [B, 5] block
        block = torch.full((B, 5), -1, dtype=torch.int64, device=DEV)
        block[:, 1:4] = torch.stack(idx, 1)
        views = [block[:, 1 + t] for t in range(3)]
        assert torch.equal(fe.fused_embedding(views, tables), want)


def test_forward_rounding_and_long_rows(D):
    idx, tables, want = oc.rounding_case(D)
    out = fe.fused_embedding(og.on_gpu(idx), og.on_gpu(tables))
    assert_same_bits(out, want, BF16, f"D={D}")
    cards = tuple((3, 300)[t % 2] for t in range(64))  # 8 * D pieces a row
    idx, tables = make_indices(97, cards, DEV), make_tables(cards, D, DEV)
    assert torch.equal(fe.fused_embedding(idx, tables),
                       forward_ref(idx, tables))


@ALL_REGIMES
@pytest.mark.parametrize("card", (1, 33, 129, 257, 5000))
@pytest.mark.parametrize("B", (1, 31, 1000))
def test_backward_exact(B, card, regime, D):
    cards = (card, 40)
    check_exact(make_indices(B, cards, DEV), make_tables(cards, D, DEV), B)


@ALL_REGIMES
def test_slab_cap_exact(regime, D):
    """B = 32769: 65 slabs of 512 rows at both widths, the last of 1 row."""
    check_exact(make_indices(32769, CARDS, DEV), make_tables(CARDS, D, DEV),
                32769)


@og.ONEHOT
@pytest.mark.parametrize("kind", KINDS)
def test_slab_cap_bit_equal(kind, regime, D):
    check_bit_equal(kind, CARDS, D, 32769, seeded(32769, CARDS))


@ALL_REGIMES
@pytest.mark.parametrize("kind", KINDS)
def test_update_bit_equal(kind, regime, D):
    """The exact_dout sums are exact, their squares are not: rowwise_adagrad
    pins the butterfly of distances 1 .. D/8 against the fallback's."""
    cards = (33, 300, 5000)
    check_bit_equal(kind, cards, D, 1000, seeded(1000, cards))


@og.SORTED
@pytest.mark.parametrize("B", (16, 17))
@pytest.mark.parametrize("kind", KINDS)
def test_update_bit_equal_chunk_edge(kind, B, regime, D):
    check_bit_equal(kind, (5000, 40), D, B, seeded(B, (5000, 40)))


@og.ONEHOT
def test_fold_order(regime, D):
    """Slab partials in ascending slab order (S = 320, 63 slabs), in every
    column slice, for the dense gradient and the update."""
    idx, dout = [torch.arange(20001) % 512], oc.wide_dout(20001, D, 303)
    want = [oc.replay_fold(idx[0], 512, dout, 512)]
    og.assert_tables_equal(og.dense_grads(idx, (512,), D, dout), want, "dense")
    og.assert_tables_equal(og.sgd_g(idx, (512,), D, dout), want, "update")


@og.SORTED
def test_sorted_order(regime, D):
    (idx, dout), cards = oc.order_case(1000, D), oc.ORDER_CARDS
    og.assert_tables_equal(og.dense_grads(idx, cards, D, dout),
                           oc.replay_runs_dense(idx, cards, dout), "dense")
    want = oc.replay_runs_update(idx, cards, oc.all_large(cards), dout)
    og.assert_tables_equal(og.sgd_g(idx, cards, D, dout),
                           [want[t] for t in oc.all_large(cards)], "update")
