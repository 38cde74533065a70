"""The fused embedding kernels (csrc/embed.hip, csrc/embed_optim.hip) held
to their documented summation orders, bit for bit, on values whose fp32 sums
depend on the order (the replays of test_fused_embedding_order_cpu.py); the
benchmark's slab geometry on exact values; and the lookup's rounding, index
and table-count edges. No comparison here has a tolerance."""

import functools

import pytest
import torch

from _shuffle_cases import BF16, assert_same_bits
from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from test_fused_embedding_cpu import (
    backward_ref64,
    forward_ref,
    make_indices,
    make_tables,
    run_backward,
)
from test_fused_embedding_gpu import (  # noqa: F401  (regime: a fixture)
    REGIMES,
    check_exact,
    regime,
)
from test_fused_embedding_optim_cpu import KINDS
from test_fused_embedding_optim_gpu import (
    RUN_SHAPES,
    check_bit_equal,
    seeded,
)
from test_fused_embedding_order_cpu import (
    CHUNK,
    ORDER_BATCHES,
    ORDER_CARDS,
    WIDTHS,
    WRAP_CARDS,
    all_large,
    fold_card,
    fold_case,
    order_case,
    replay_fold,
    replay_runs_dense,
    replay_runs_update,
    rounding_case,
    run_shape_case,
    single_run_case,
    three_table_case,
    wrap_case,
    wrap_forward_ref,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SORTED = pytest.mark.parametrize("regime", (0,), indirect=True)
ONEHOT = pytest.mark.parametrize("regime", (10**6,), indirect=True)


def on_gpu(xs):
    return [x.to(DEV) for x in xs]


def dense_grads(idx, cards, D, dout):
    tables = make_tables(cards, D, DEV)
    return [g.cpu() for g in run_backward(on_gpu(idx), tables, dout.to(DEV))]


def poison_carry(N, D):
    """The update's ``carry`` scratch is not cleared: pass 2 must read only
    the slots pass 1 wrote. Fill a block of carry's size with NaN and free
    it, so that the caching allocator will normally hand that block to the
    binding. Best effort: nothing guarantees the reuse."""
    n = -(-N // CHUNK) * 2 * D
    if n:
        torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def sgd_g(idx, cards, D, dout):
    """g per table as the update kernels sum it: sgd with lr = 1 on zero
    tables gives p' = 0 - g exactly."""
    tables = [torch.zeros(c, D, device=DEV).requires_grad_() for c in cards]
    opt = fe.FusedEmbeddingOptimizer(tables, kind="sgd", lr=1.0)
    fe.fused_embedding(on_gpu(idx), tables, optimizer=opt).backward(
        dout.to(DEV))
    large = [c for c in cards if c > fe._DENSE_MAX_ROWS]
    poison_carry(len(large) * dout.shape[0], D)
    opt.step()
    return [-w.detach().cpu() for w in tables]


def assert_tables_equal(got, want, what):
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == torch.float32
        assert torch.equal(g, w), (
            f"{what}, table {t}: {int((g != w).any(1).sum())} rows differ")


# ----- B. the summation orders ------------------------------------------------


@functools.lru_cache(maxsize=None)
def dense_replay(case, D):
    idx, dout, cards = sorted_case(case, D)
    return replay_runs_dense(idx, cards, dout)


@functools.lru_cache(maxsize=None)
def update_replay(case, D):
    idx, dout, cards = sorted_case(case, D)
    large = all_large(cards)
    got = replay_runs_update(idx, cards, large, dout)
    return [got[t] for t in large]


def sorted_case(case, D):
    """(idx, dout, cards): a batch size of ORDER_BATCHES at ORDER_CARDS,
    "single", "three" or a name of RUN_SHAPES (D = 16)."""
    if case == "single":
        return single_run_case(D)
    if case == "three":
        return three_table_case(D)
    if case in RUN_SHAPES:
        return run_shape_case(case)
    return (*order_case(case, D), ORDER_CARDS)


@SORTED
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("case", (1000, "single"))
def test_dense_backward_order(case, D, regime):
    """embed_bwd_runs: ascending batch row inside a run."""
    idx, dout, cards = sorted_case(case, D)
    assert_tables_equal(dense_grads(idx, cards, D, dout),
                        dense_replay(case, D), f"{case}, D={D}")


@SORTED
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("case", ORDER_BATCHES + ("single", "three"))
def test_sparse_update_order(case, D, regime):
    """embed_runs_update and embed_carry_update: ascending batch row inside
    16-position chunks of the stably sorted keys, then chunks ascending."""
    idx, dout, cards = sorted_case(case, D)
    assert_tables_equal(sgd_g(idx, cards, D, dout), update_replay(case, D),
                        f"{case}, D={D}")


@SORTED
@pytest.mark.parametrize("runs", sorted(RUN_SHAPES))
def test_sparse_update_order_run_shapes(runs, regime):
    idx, dout, cards = sorted_case(runs, 16)
    assert_tables_equal(sgd_g(idx, cards, 16, dout), update_replay(runs, 16),
                        runs)


@functools.lru_cache(maxsize=None)
def fold_replay(D):
    """The fold-order table's replay and the exact table's fp64 sum."""
    idx, dout, cards = fold_case(D)
    (small,), _, _ = backward_ref64(
        idx[1:], [torch.empty(cards[1], D)], dout[:, D:])
    return [replay_fold(idx[0], cards[0], dout[:, :D], fold_card(D)),
            small.float()]


@ONEHOT
@pytest.mark.parametrize("D", WIDTHS)
def test_fold_order_dense(D, regime):
    """embed_bwd_fold: slab partials in ascending slab order (S = 320, 63
    slabs, the last of 161 rows)."""
    idx, dout, cards = fold_case(D)
    assert_tables_equal(dense_grads(idx, cards, D, dout), fold_replay(D),
                        f"D={D}")


@ONEHOT
@pytest.mark.parametrize("D", WIDTHS)
def test_fold_order_update(D, regime):
    """embed_fold_update: the same order."""
    idx, dout, cards = fold_case(D)
    assert_tables_equal(sgd_g(idx, cards, D, dout), fold_replay(D), f"D={D}")


# ----- C. large-batch slab geometry, exact values -----------------------------

SLAB_CARDS = (3, 300, 5000)
SLAB_CASES = (
    # the capped slab (2048 / 1024 / 512 rows), 65 slabs, the last of 1 row
    (8, 131073), (16, 65537), (32, 32769),
    # the uncapped slab of 320 rows, with a part and a full last slab
    (16, 20001), (16, 20000),
)
HOT_B = 65537  # every index 7: one row across all slabs and all chunks


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
@pytest.mark.parametrize("D,B", SLAB_CASES)
def test_large_batch_exact(D, B, regime):
    check_exact(make_indices(B, SLAB_CARDS, DEV),
                make_tables(SLAB_CARDS, D, DEV), B)


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
@pytest.mark.parametrize("D,B", SLAB_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_large_batch_bit_equal(kind, D, B, regime):
    check_bit_equal(kind, SLAB_CARDS, D, B, seeded(B, SLAB_CARDS))


@pytest.mark.parametrize("regime", REGIMES[:2], indirect=True)
def test_hot_row_exact(regime):
    idx = [torch.full((HOT_B,), 7, dtype=torch.int64, device=DEV)]
    check_exact(idx, make_tables((40,), 16, DEV), HOT_B)


@pytest.mark.parametrize("regime", REGIMES[:2], indirect=True)
@pytest.mark.parametrize("kind", KINDS)
def test_hot_row_bit_equal(kind, regime):
    check_bit_equal(kind, (40,), 16, HOT_B,
                    lambda step: [torch.full((HOT_B,), 7)])


# ----- D. value and index edges -----------------------------------------------


@pytest.mark.parametrize("D", WIDTHS)
def test_forward_rounding_edges(D):
    """RNE ties, overflow to inf, +-inf, +-0, fp32 subnormals and NaNs
    through the forward's rounding, against the integer oracle."""
    idx, tables, want = rounding_case(D)
    out = fe.fused_embedding(on_gpu(idx), on_gpu(tables))
    assert_same_bits(out, want, BF16, f"D={D}")


@pytest.mark.parametrize("D", WIDTHS)
def test_index_wrap_forward(D):
    idx, rows = wrap_case()
    tables = make_tables(WRAP_CARDS, D, DEV)
    assert fe._kernels_serve(on_gpu(idx), tables)
    assert torch.equal(fe.fused_embedding(on_gpu(idx), tables).cpu(),
                       wrap_forward_ref(rows, tables))


@pytest.mark.parametrize("regime", REGIMES, indirect=True)
def test_index_wrap_backward(regime):
    idx, rows = wrap_case()
    check_exact(on_gpu(idx), make_tables(WRAP_CARDS, 16, DEV), len(rows[0]))


MANY = {T: tuple((3, 300)[t % 2] for t in range(T)) for T in (64, 65)}


def many_tables(T):
    """(idx, tables) of T tables, D = 8, B = 97. 64 is the most the kernels
    take (by-value argument structs of that many entries); 65 must go the
    torch-op way."""
    idx = make_indices(97, MANY[T], DEV)
    tables = make_tables(MANY[T], 8, DEV)
    assert fe._kernels_serve(idx, tables) == (T == 64)
    return idx, tables


@pytest.mark.parametrize("T", (64, 65))
def test_table_count_forward_and_backward(T):
    idx, tables = many_tables(T)
    assert torch.equal(fe.fused_embedding(idx, tables),
                       forward_ref(idx, tables))
    check_exact(idx, tables, 97)


@pytest.mark.parametrize("T", (64, 65))
@pytest.mark.parametrize("kind", KINDS)
def test_table_count_bit_equal(kind, T):
    many_tables(T)
    check_bit_equal(kind, MANY[T], 8, 97, seeded(97, MANY[T]))
