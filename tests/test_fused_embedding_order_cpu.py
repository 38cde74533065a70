"""Order-replay oracles for the fused embedding kernels (csrc/embed.hip,
csrc/embed_optim.hip), their inputs and the conditions those inputs must
meet, all on the CPU; test_fused_embedding_order_gpu.py holds the kernels to
them bit for bit.

The kernels promise a fixed summation order. A replay performs that order
with one fp32 add at a time in numpy, written from the documentation (the
file headers, FusedEmbeddingOptimizer's docstring, docs/DESIGN.md) and not
from the kernels:

  replay_runs_dense    a table row's gradient is the chain
                       ((+0 + g_b1) + g_b2) + ... over the batch rows that
                       hit it, ascending (embed_bwd_runs)
  replay_runs_update   the stably sorted keys of the sorted regime are cut
                       into chunks of 16 positions from position 0; every
                       (run, chunk) segment is such a chain in position
                       order, and a row's g is its first segment plus the
                       later ones, chunks ascending (embed_runs_update,
                       embed_carry_update)
  replay_fold          the slab partials added in ascending slab order
                       (embed_bwd_fold, embed_fold_update), for inputs that
                       hit a row at most once per slab: a partial is then
                       one bf16 value or +0, the matrix core's own order
                       drops out, and g is the ascending-batch-row chain

An order only shows where fp32 adds round, so the inputs are wide_dout: bf16
values whose exponents spread over 2^-12 .. 2^12. The self-checks below are
conditions on these inputs (each replay differs from the order it must tell
apart) and print the share of rows that differ.

The forward rounding and index-wrap edge cases of the lookup live here too,
with an integer round-to-nearest-even on the fp32 bits as the oracle.
"""

import functools

import numpy as np
import pytest
import torch

from _shuffle_cases import BF16, assert_same_bits
from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from test_fused_embedding_cpu import (
    backward_ref64,
    exact_dout,
    make_tables,
    run_backward,
)

I64_MIN = torch.iinfo(torch.int64).min
I64_MAX = torch.iinfo(torch.int64).max
CHUNK = 16  # positions of a chunk of the sorted regime's update

WIDTHS = (8, 16, 32)
ORDER_CARDS = (300, 5000, 40)
ORDER_BATCHES = (15, 16, 17, 33, 1000)


# ----- inputs -----------------------------------------------------------------


def wide_dout(B, width, seed):
    """bf16 [B, width] whose exponents spread over 25 binades, so that an
    fp32 sum of a few of them rounds and its order shows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, width, generator=g)
    e = torch.randint(-12, 13, (B, width), generator=g)
    return (x * torch.pow(2.0, e)).bfloat16()


def hot_indices(B, cards, seed):
    """[B] int64 per table, inside [0, card): two rows in three hit the
    table's first, middle or last row, the rest any row, so that short
    batches have runs of three and more as well, at both ends of a table's
    stretch of the sorted keys."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for c in cards:
        hot = torch.tensor([0, c // 2, c - 1])[
            torch.randint(0, 3, (B,), generator=g)]
        cold = torch.randint(0, c, (B,), generator=g)
        pick = torch.randint(0, 3, (B,), generator=g) < 2
        out.append(torch.where(pick, hot, cold))
    return out


# (B, D) -> the first seed of hot_indices and wide_dout, counting up from 0,
# at which self-checks 2 and 3 hold (test_order_inputs_are_sharp); 0 where
# not listed. Short batches need the search: a run that crosses a chunk
# boundary with a single position behind it sums as the plain chain does,
# and at B = 17 the first table's last two positions straddle a boundary.
ORDER_SEEDS = {
    (15, 8): 28, (16, 8): 4, (17, 8): 564, (33, 8): 5,
    (16, 16): 4, (17, 16): 100, (33, 16): 1,
    (17, 32): 22,
}


def order_inputs(B, D, seed):
    return (hot_indices(B, ORDER_CARDS, 100 + seed),
            wide_dout(B, len(ORDER_CARDS) * D, 200 + seed))


@functools.lru_cache(maxsize=None)
def order_case(B, D):
    """(idx, dout) of the sorted regime's order tests at ORDER_CARDS."""
    return order_inputs(B, D, ORDER_SEEDS.get((B, D), 0))


@functools.lru_cache(maxsize=None)
def single_run_case(D):
    """One table of 1000 rows, every index 7: one run of length B."""
    B = 1000
    return [torch.full((B,), 7)], wide_dout(B, D, 300), (B,)


@functools.lru_cache(maxsize=None)
def three_table_case(D):
    """B = 5 and three tables: N = 15, one chunk spans all three. The seed
    is the first from 301 at which reversing the runs shows in every table
    at every width."""
    idx = [torch.tensor(r) for r in
           ([1, 1, 2, 1, 1], [4999, 0, 4999, 4999, 0], [39, 39, 39, 39, 39])]
    return idx, wide_dout(5, 3 * D, 345), ORDER_CARDS


FOLD_B = 20001
FOLD_SMALL = 3  # rows of the second table, which gets exact values


def fold_card(D):
    """The one-hot regime's largest slab: 2048 / 1024 / 512 rows."""
    return 16384 // D


@functools.lru_cache(maxsize=None)
def fold_case(D):
    """idx[b] = b % card with card = the largest slab, so that every aligned
    slab of any smaller size holds a row at most once; a 3-row table with
    exact values next to it."""
    card = fold_card(D)
    g = torch.Generator().manual_seed(302)
    idx = [torch.arange(FOLD_B) % card,
           torch.randint(0, FOLD_SMALL, (FOLD_B,), generator=g)]
    dout = torch.cat([wide_dout(FOLD_B, D, 303),
                      exact_dout(FOLD_B, D, "cpu", seed=304)], 1)
    return idx, dout, (card, FOLD_SMALL)


# ----- the replays ------------------------------------------------------------


def _chain(groups, vals, ngroups, reverse=False):
    """out[g] = ((+0 + v_1) + v_2) + ... over the items of group g in item
    order (``reverse``: in reversed item order), one fp32 add at a time."""
    groups = np.asarray(groups, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float32)
    n = len(groups)
    out = np.zeros((ngroups,) + vals.shape[1:], dtype=np.float32)
    if n == 0:
        return out
    order = np.argsort(groups, kind="stable")
    if reverse:
        order = order[::-1]
    gs = groups[order]
    start = np.r_[True, gs[1:] != gs[:-1]]
    rank = np.arange(n) - np.maximum.accumulate(
        np.where(start, np.arange(n), 0))
    for k in range(int(rank.max()) + 1):
        sel = order[rank == k]  # at most one item per group
        out[groups[sel]] = out[groups[sel]] + vals[sel]
    return out


def _rows(idx, cards):
    """max(i, 0) % card per table, in Python-int arithmetic."""
    return [
        np.array([max(int(v), 0) % c for v in x.reshape(-1).tolist()],
                 dtype=np.int64)
        for x, c in zip(idx, cards)
    ]


def _f32(dout):
    return dout.float().cpu().numpy()


def replay_runs_dense(idx, cards, dout, reverse=False):
    """fp32 [card, D] per table: what embed_bwd_runs documents."""
    g = _f32(dout)
    D = g.shape[1] // len(cards)
    return [
        torch.from_numpy(
            _chain(r, g[:, t * D:(t + 1) * D], c, reverse=reverse))
        for t, (r, c) in enumerate(zip(_rows(idx, cards), cards))
    ]


def sorted_positions(idx, cards, large, reverse=False):
    """(keys, table, batch row) of the sorted regime's N = len(large) * B
    positions: the tables of ``large`` in ascending table number, each with
    its B batch rows ascending, key = flat row offset + wrapped index,
    sorted stably (``reverse``: descending batch row inside equal keys)."""
    rows = _rows(idx, cards)
    offs = np.concatenate([[0], np.cumsum(cards)])
    B = len(rows[0])
    large = sorted(large)
    keys = np.concatenate([offs[t] + rows[t] for t in large])
    tab = np.repeat(np.asarray(large, dtype=np.int64), B)
    b = np.tile(np.arange(B), len(large))
    order = (np.lexsort((-b, keys)) if reverse
             else np.argsort(keys, kind="stable"))
    return keys[order], tab[order], b[order]


def replay_runs_update(idx, cards, large, dout, chunk=CHUNK, reverse=False):
    """{t: fp32 [card_t, D]} for t in ``large``: the g that embed_runs_update
    and embed_carry_update document."""
    g = _f32(dout)
    D = g.shape[1] // len(cards)
    keys, tab, b = sorted_positions(idx, cards, large, reverse=reverse)
    n = len(keys)
    vals = g.reshape(len(b) // len(large), len(cards), D)[b, tab]
    pos = np.arange(n)
    start = np.r_[True, keys[1:] != keys[:-1]] | (pos % chunk == 0)
    seg = np.cumsum(start) - 1
    seg_sum = _chain(seg, vals, int(seg[-1]) + 1)
    # 0 + first segment is the first segment: the same chain over segments
    flat = _chain(keys[start], seg_sum, int(sum(cards)))
    offs = np.concatenate([[0], np.cumsum(cards)])
    return {t: torch.from_numpy(flat[offs[t]:offs[t] + cards[t]].copy())
            for t in large}


def crossing_tables(idx, cards, large, chunk=CHUNK):
    """The tables of ``large`` that have a run in more than one chunk."""
    keys, tab, _ = sorted_positions(idx, cards, large)
    pos = np.arange(len(keys))
    same = keys[1:] == keys[:-1]
    cross = same & (pos[1:] % chunk == 0)
    return sorted(set(tab[1:][cross].tolist()))


def replay_fold(idx, card, dout, max_slab, descending=False):
    """fp32 [card, D]: the ascending-slab fold for one table whose rows are
    hit at most once in any aligned slab of up to ``max_slab`` rows (two hits
    of a row lie ``max_slab`` or more apart; asserted). ``dout`` is the
    table's [B, D] slice."""
    (r,) = _rows([idx], [card])
    order = np.argsort(r, kind="stable")
    rs = r[order]
    gap = np.diff(order)[rs[1:] == rs[:-1]]
    assert len(gap) == 0 or gap.min() >= max_slab
    return torch.from_numpy(_chain(r, _f32(dout), card, reverse=descending))


# ----- self-checks ------------------------------------------------------------


def rows_differ(a, b):
    """(rows that differ, rows that are not zero in a)."""
    return int((a != b).any(1).sum()), int((a != 0).any(1).sum())


def max_run(idx, card):
    (r,) = _rows([idx], [card])
    return int(np.bincount(r).max())


def all_large(cards):
    return list(range(len(cards)))


def sorted_cases():
    """(name, idx, dout, cards) of every sorted-regime order case."""
    from test_fused_embedding_optim_gpu import RUN_SHAPES

    out = []
    for D in WIDTHS:
        for B in ORDER_BATCHES:
            out.append((f"B{B}-D{D}", *order_case(B, D), ORDER_CARDS))
        out.append((f"single-D{D}", *single_run_case(D)))
        out.append((f"three-D{D}", *three_table_case(D)))
    for name, (B, index_fn) in sorted(RUN_SHAPES.items()):
        out.append((name, *run_shape_case(name)))
    return out


@functools.lru_cache(maxsize=None)
def run_shape_case(name):
    """(idx, dout, cards) of test_fused_embedding_optim_gpu.RUN_SHAPES[name]
    (its step-0 indices) with wide values, D = 16."""
    from test_fused_embedding_optim_gpu import RUN_SHAPES

    B, index_fn = RUN_SHAPES[name]
    return index_fn(0), wide_dout(B, 16, 305), (B,)


def assert_replay_within_bound(got, idx, cards, dout):
    """Self-check 5: |replay - fp64| <= n * 2^-23 * S, nothing infinite."""
    tables = [torch.empty(c, got[0].shape[1]) for c in cards]
    ref, cnt, mag = backward_ref64(idx, tables, dout)
    for g, r, n, s in zip(got, ref, cnt, mag):
        assert torch.isfinite(g).all()
        assert ((g.double() - r).abs() <= n * 2.0**-23 * s).all()


@pytest.mark.parametrize("D", WIDTHS)
def test_replays_equal_fp64_on_exact_values(D):
    """Self-check 1: where every order is exact, every replay is the fp64
    sum."""
    B = 1000
    idx = hot_indices(B, ORDER_CARDS, 1)
    dout = exact_dout(B, len(ORDER_CARDS) * D, "cpu")
    ref, _, _ = backward_ref64(
        idx, [torch.empty(c, D) for c in ORDER_CARDS], dout)
    dense = replay_runs_dense(idx, ORDER_CARDS, dout)
    upd = replay_runs_update(idx, ORDER_CARDS, all_large(ORDER_CARDS), dout)
    for t, r in enumerate(ref):
        assert torch.equal(dense[t], r.float())
        assert torch.equal(upd[t], r.float())
    fidx, _, fcards = fold_case(D)
    fdout = exact_dout(FOLD_B, D, "cpu", seed=6)
    (fref,), _, _ = backward_ref64(
        fidx[:1], [torch.empty(fcards[0], D)], fdout)
    assert torch.equal(
        replay_fold(fidx[0], fcards[0], fdout, fold_card(D)), fref.float())


def check_sharp(name, idx, dout, cards, must_cross=False):
    """Self-checks 2, 3 and 5 on one sorted-regime input; returns the number
    of rows in which chunks of 32 would give other bits than chunks of 16."""
    large = all_large(cards)
    dense = replay_runs_dense(idx, cards, dout)
    upd = replay_runs_update(idx, cards, large, dout)
    dense_r = replay_runs_dense(idx, cards, dout, reverse=True)
    upd_r = replay_runs_update(idx, cards, large, dout, reverse=True)
    upd_32 = replay_runs_update(idx, cards, large, dout, chunk=32)
    assert_replay_within_bound(dense, idx, cards, dout)
    assert_replay_within_bound([upd[t] for t in large], idx, cards, dout)
    crossing = crossing_tables(idx, cards, large)
    assert crossing or not must_cross, name
    chunk32 = 0
    for t in large:
        d, n = rows_differ(upd[t], dense[t])
        dr, _ = rows_differ(dense[t], dense_r[t])
        ur, _ = rows_differ(upd[t], upd_r[t])
        d32, _ = rows_differ(upd[t], upd_32[t])
        chunk32 += d32
        print(f"{name} table {t}: of {n} rows hit, chunked != chain in "
              f"{d}, chain != reversed in {dr}, chunked != reversed in "
              f"{ur}, chunks of 16 != chunks of 32 in {d32}")
        if t in crossing:
            assert d > 0, (name, t)
        if max_run(idx[t], cards[t]) >= 3:
            assert dr > 0 and ur > 0, (name, t)
    return chunk32


def test_order_inputs_are_sharp():
    """Self-checks 2, 3 and 5 on every sorted-regime input of the GPU tests:
    the chunked order differs from the plain chain in every table that has a
    run crossing a chunk boundary (every random case has one, except at
    B = 16, where the boundaries fall between the tables), both differ from
    themselves with the batch order inside the runs reversed in every table
    that has a run of three or more, and chunks of 32 positions would give
    other bits in every random case of B >= 33."""
    for name, idx, dout, cards in sorted_cases():
        must_cross = name.startswith("B") and len(idx[0]) % CHUNK != 0
        d32 = check_sharp(name, idx, dout, cards, must_cross)
        if name.startswith(("B33", "B1000")):
            assert d32 > 0, name


@pytest.mark.parametrize("D", WIDTHS)
def test_fold_inputs_are_sharp(D):
    """Self-checks 4 and 5: the ascending fold differs from the descending
    one."""
    idx, dout, cards = fold_case(D)
    up = replay_fold(idx[0], cards[0], dout[:, :D], fold_card(D))
    down = replay_fold(idx[0], cards[0], dout[:, :D], fold_card(D),
                       descending=True)
    d, n = rows_differ(up, down)
    print(f"D={D}: of {n} rows hit, ascending != descending in {d}")
    assert d > 0
    assert_replay_within_bound([up], idx[:1], cards[:1], dout[:, :D])
    with pytest.raises(AssertionError):  # two hits of a row inside one slab
        replay_fold(idx[0] % 7, cards[0], dout[:, :D], fold_card(D))


def test_chunked_order_by_hand():
    """Three values whose sum depends on where the chunk boundary falls:
    (2^24 + 1) + 1 = 2^24 twice over, 2^24 + (1 + 1) = 2^24 + 2."""
    B = 18  # positions 0..14 row 1, then a, b, c of row 2 at 15, 16, 17
    idx = [torch.tensor([1] * 15 + [2, 2, 2])]
    dout = torch.zeros(B, 8)
    dout[15:, 0] = torch.tensor([2.0**24, 1.0, 1.0])
    dout = dout.bfloat16()
    dense = replay_runs_dense(idx, (3,), dout)[0]
    upd = replay_runs_update(idx, (3,), [0], dout)[0]
    assert dense[2, 0] == 2.0**24 and upd[2, 0] == 2.0**24 + 2
    assert crossing_tables(idx, (3,), [0]) == [0]


# ----- forward rounding edges -------------------------------------------------

ROUNDING_BITS = (
    0x3F808000,  # tie, down to the even 0x3f80
    0x3F818000,  # tie, up to the even 0x3f82
    0x3F808001, 0x3F818001,  # just above a tie
    0x3F807FFF, 0x3F817FFF,  # just below
    0xBF808000, 0xBF818000,  # the ties, negative
    0x7F7FFFFF, 0x7F7F8000, 0xFF7FFFFF,  # over the top: +-inf
    0x7F7F7FFF,  # the largest value that stays finite
    0x7F800000, 0xFF800000,  # +-inf
    0x00000000, 0x80000000,  # +-0
    0x80008000,  # a negative subnormal tie, to -0
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF,  # fp32 subnormals
    0x7FC00000, 0x7F800001, 0x7FA00000,  # quiet and signalling NaNs
    0xFFC00000, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF,
)


def bf16_rne_bits(u32):
    """fp32 bit patterns -> bf16 bit patterns (uint16), round to nearest,
    ties to even, in integer arithmetic; every NaN becomes 0x7fc0."""
    u = np.asarray(u32, dtype=np.uint32).astype(np.uint64)
    keep, rest = u >> 16, u & 0xFFFF
    up = (rest > 0x8000) | ((rest == 0x8000) & ((keep & 1) == 1))
    out = keep + up  # a carry out of the mantissa is the next exponent
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, 0x7FC0, out).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def rounding_case(D):
    """(idx, tables, expected int16 bits [B, 2 * D]): a table whose element
    (r, j) is the (r + j)-th of the ROUNDING_BITS, so that every pattern
    meets every column, padded with five randn rows, and a randn table for
    company."""
    n = len(ROUNDING_BITS)
    cards = (n + 5, 17)
    g = torch.Generator().manual_seed(8)
    bits = [torch.randn(c, D, generator=g).numpy().view(np.uint32).copy()
            for c in cards]
    pat = np.array(ROUNDING_BITS, dtype=np.uint32)
    bits[0][:n] = pat[(np.arange(n)[:, None] + np.arange(D)[None, :]) % n]
    B = 2 * cards[0] + 1
    idx = [torch.arange(B) % c for c in cards]
    want = np.concatenate(
        [bf16_rne_bits(b)[x.numpy()] for b, x in zip(bits, idx)], 1)
    tables = [torch.from_numpy(b.view(np.float32)) for b in bits]
    return idx, tables, want.view(np.int16)


def test_rounding_oracle_by_hand():
    got = bf16_rne_bits(ROUNDING_BITS[:21])
    assert got.tolist() == [
        0x3F80, 0x3F82, 0x3F81, 0x3F82, 0x3F80, 0x3F81, 0xBF80, 0xBF82,
        0x7F80, 0x7F80, 0xFF80, 0x7F7F, 0x7F80, 0xFF80, 0x0000, 0x8000,
        0x8000, 0x0000, 0x0000, 0x0002, 0x0080]
    assert (bf16_rne_bits(ROUNDING_BITS[21:]) == 0x7FC0).all()
    for D in WIDTHS:  # every pattern lands in every column
        _, tables, _ = rounding_case(D)
        col = tables[0].numpy().view(np.uint32)
        assert all((col[:, j] == p).any() for j in range(D)
                   for p in ROUNDING_BITS)


@pytest.mark.parametrize("D", WIDTHS)
def test_forward_rounding_edges(D):
    idx, tables, want = rounding_case(D)
    out = fe.fused_embedding(idx, tables)
    assert_same_bits(out, want, BF16, f"D={D}")


# ----- index wrap -------------------------------------------------------------

WRAP_CARDS = (1, 3, 17, 5000, 65537)


def wrap_values(card):
    return [I64_MIN, -1, 0, card - 1, card, 2**31 - 1, 2**31, 2**31 + 1,
            2**32 - 1, 2**32, 2**32 + card, I64_MAX]


@functools.lru_cache(maxsize=None)
def wrap_case():
    """(idx, expected rows per table): the values on both sides of the
    32-bit / 64-bit switch of the wrap, and the expected row
    max(v, 0) % card in Python ints."""
    idx = [torch.tensor(wrap_values(c), dtype=torch.int64)
           for c in WRAP_CARDS]
    rows = [torch.tensor([max(v, 0) % c for v in wrap_values(c)])
            for c in WRAP_CARDS]
    return idx, rows


def wrap_forward_ref(rows, tables):
    return torch.cat(
        [w.detach().cpu()[r] for w, r in zip(tables, rows)], 1).bfloat16()


def test_index_wrap_edges():
    idx, rows = wrap_case()
    assert [r.tolist() for r in rows][1] == [0, 0, 0, 2, 0, 1, 2, 0, 0, 1,
                                             1, 1]
    for x, r, c in zip(idx, rows, WRAP_CARDS):  # backward_ref64's wrap
        assert torch.equal(x.clamp_min(0) % c, r)
    tables = make_tables(WRAP_CARDS, 16, "cpu")
    assert torch.equal(fe.fused_embedding(idx, tables),
                       wrap_forward_ref(rows, tables))
    dout = exact_dout(len(rows[0]), len(WRAP_CARDS) * 16, "cpu")
    grads = run_backward(idx, tables, dout)
    for t, (g, r) in enumerate(zip(grads, rows)):
        want = torch.zeros_like(g).index_add_(
            0, r, dout[:, t * 16:(t + 1) * 16].float())
        assert torch.equal(g, want)
