"""CPU checks of the shuffle oracle (tests/_shuffle_cases.py): the project's
CPU pack / unpack / gather / partition equal it on every named schema, and
the conditions its exact GPU comparison rests on hold (layout claims, no
subnormal results, in-range ints, ties that tell one rounding from two)."""

import numpy as np
import pytest
import torch

import _shuffle_cases as sc
from ray_shuffling_data_loader_amd.ops import shuffle_ops
from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
    gather_rows,
    pack_columns,
    partition_rows,
    unpack_permute,
)


def _t(a):
    return torch.from_numpy(np.array(a))


# ----- the project's CPU paths against the oracle ---------------------------


@pytest.mark.parametrize("name,n", sc.SCHEMA_CASES)
def test_cpu_pack_matches_oracle(name, n):
    schema = sc.schema_of(name)
    cols = sc.schema_columns(name, n)
    tcols = sc.cols_to_torch(cols, sc.schema_dtypes(schema))
    # the CPU path zero-fills padding, as the oracle does: every byte
    got = pack_columns(tcols, schema)
    assert np.array_equal(got.numpy(), sc.schema_packed(name, n))
    scatter = sc.perm_cases(n)["full"]
    got = pack_columns(tcols, schema, perm=_t(scatter))
    assert np.array_equal(got.numpy(), sc.pack_ref(cols, schema, scatter))
    # the oracle's scatter is the inverse of its gather
    assert np.array_equal(
        sc.pack_ref(cols, schema, scatter)[scatter], sc.schema_packed(name, n))


@pytest.mark.parametrize("name,n", sc.SCHEMA_CASES)
def test_cpu_unpack_matches_oracle(name, n):
    schema = sc.schema_of(name)
    packed = sc.schema_packed(name, n)
    for kind, perm in sc.perm_cases(n).items():
        want = sc.unpack_ref(packed, schema, perm)
        got = unpack_permute(
            _t(packed), schema, perm=None if perm is None else _t(perm))
        assert set(got) == set(want)
        for spec in schema.columns:
            sc.assert_same_bits(
                got[spec.name], want[spec.name], spec.dtype,
                (name, n, kind, spec.name))
    # identity unpack gives the columns back
    back = sc.unpack_ref(packed, schema)
    for spec in schema.columns:
        sc.assert_same_bits(
            back[spec.name], sc.schema_columns(name, n)[spec.name],
            spec.dtype, (name, n, spec.name))


@pytest.mark.parametrize("cell", sc.CAST_CELLS, ids=sc.cell_id)
def test_cpu_cast_matrix_matches_oracle(cell):
    src, dst = cell
    schema, _, packed = sc.cast_case(src, dst)
    out_dtypes = {"s": dst, "v": dst}
    perm = sc.perm_cases(sc.CAST_ROWS)["full"]
    want = sc.unpack_ref(packed, schema, perm, out_dtypes)
    got = unpack_permute(_t(packed), schema, _t(perm), out_dtypes)
    for name in ("s", "v"):
        assert got[name].dtype == dst
        sc.assert_same_bits(got[name], want[name], dst, (cell, name))


@pytest.mark.parametrize("stride", (16, 48, 416, 1024))
def test_cpu_gather_matches_oracle(stride):
    n = 257
    src = sc.rows_with_ids(n, stride)
    for kind, perm in sc.perm_cases(n).items():
        if perm is None:
            continue
        for dt in (torch.int64, torch.int32):
            got = gather_rows(_t(src), _t(perm).to(dt))
            assert np.array_equal(got.numpy(), src[perm]), (kind, dt)
    perm = sc.perm_cases(n)["subset"]
    out = torch.full((n, stride), 0xA5, dtype=torch.uint8)
    got = gather_rows(_t(src), _t(perm), out=out)
    assert np.array_equal(got.numpy(), src[perm])
    assert (out[len(perm):] == 0xA5).all()
    empty = gather_rows(_t(src), torch.empty(0, dtype=torch.int64))
    assert tuple(empty.shape) == (0, stride)


@pytest.mark.parametrize("kind", sc.DEST_PATTERNS)
@pytest.mark.parametrize("num_dests", (1, 2, 257, 1024))
@pytest.mark.parametrize("n", (0, 1, 255, 257, 4099))
def test_cpu_partition_matches_oracle(n, num_dests, kind):
    src = sc.rows_with_ids(n, 16)
    dest = sc.dest_pattern(kind, n, num_dests)
    assert n == 0 or (dest.min() >= 0 and dest.max() < num_dests)
    grouped, counts = partition_rows(_t(src), _t(dest), num_dests)
    assert np.array_equal(
        counts.numpy(), np.bincount(dest, minlength=num_dests))
    # the CPU path is the stable partition
    assert np.array_equal(
        grouped.numpy(), src[np.argsort(dest, kind="stable")])
    if kind == "every_second_empty":
        assert (counts.numpy()[1::2] == 0).all()


# ----- the conditions the exact comparison rests on -------------------------


def test_layout_claims():
    """The paths each named schema is there to reach, read off the layout."""
    lad = sc.schema_of("ladder")
    assert [sc.copy_width(lad, c.name) for c in lad.columns] == [
        16, 8, 4, 2, 1]
    assert [lad.offsets[c.name] for c in lad.columns] == [0, 16, 24, 28, 30]
    assert [c.row_bytes for c in lad.columns] == [16, 8, 4, 2, 3]
    assert lad.row_stride == 48
    # vec4 unpack: f32, numel % 4 == 0, offset % 16 == 0
    assert sc.schema_of("vec_aligned").offsets["v"] == 0
    assert sc.schema_of("vec_off8").offsets["v"] == 8
    assert sc.schema_of("vec_odd").col("v").numel % 4 != 0
    assert sc.schema_of("het").offsets["vec"] == 20  # 4 mod 16: no vec4
    # tiled pack: columns are handed over in DECLARED order; the fast path
    # needs scalars, 8-B ones first
    size = [c.row_bytes for c in sc.schema_of("fast84").columns]
    assert size == [8, 8, 4, 4]
    assert [c.row_bytes for c in sc.schema_of("slow48").columns] == [
        4, 4, 8, 8]
    assert [c.row_bytes for c in sc.schema_of("fast_only8").columns] == [8, 8]
    assert [c.row_bytes for c in sc.schema_of("fast_only4").columns] == [4, 4]
    # same bytes either way: only the declared order differs
    assert sc.schema_of("slow48").offsets == sc.schema_of("fast84").offsets
    # rows per LDS tile: min(128, 65536 // (row_stride + 8))
    wide = sc.schema_of("wide")
    assert wide.row_stride == 816 and 65536 // (816 + 8) == 79
    c128 = sc.schema_of("cols128")
    assert len(c128.columns) == 128 and c128.row_stride == 1024
    assert 65536 // (1024 + 8) == 63
    for name in sc.SCHEMAS:
        tile = min(128, 65536 // (sc.schema_of(name).row_stride + 8))
        rows = sc.ROWS[name]
        # a short single tile, and a tile edge with a tail
        assert min(rows) < tile and max(rows) > tile, name
        assert any(r % tile for r in rows if r > tile), name
    # the sweep kernel's schemas
    ok = [n for n in sc.SCHEMAS if shuffle_ops.row_sweep_ok(sc.schema_of(n))]
    assert "fast_only8" in ok and "vec_aligned" in ok and "ladder" not in ok


def test_no_subnormal_results_and_ints_in_range():
    for src, dst in sc.CAST_CELLS:
        schema, cols, packed = sc.cast_case(src, dst)
        # cast_ref asserts finite, in-range inputs for float -> int
        out = sc.unpack_ref(packed, schema, None, {"s": dst, "v": dst})
        for name, a in out.items():
            assert not sc.has_subnormal(a, dst), (src, dst, name)
    for name, n in sc.SCHEMA_CASES:
        for spec in sc.schema_of(name).columns:
            a = sc.schema_columns(name, n)[spec.name]
            assert not sc.has_subnormal(a, spec.dtype), (name, n, spec.name)


def test_f64_ties_tell_one_rounding_from_two():
    x = sc.cast_inputs(sc.F64, sc.BF16, sc.CAST_ROWS * 4)
    one = sc.cast_ref(x, sc.F64, sc.BF16)
    with np.errstate(over="ignore", invalid="ignore"):
        two = sc.cast_ref(x.astype(np.float32), sc.F32, sc.BF16)
    nan = np.isnan(x)
    differ = (one != two) & ~nan
    # a third of the 3 * (k // 4) constructed values sit 2^-40 beyond a
    # midpoint on the side away from the even neighbour
    assert differ.sum() >= sc.CAST_ROWS // 4, int(differ.sum())
    # ... and the project's own single-rounding cast agrees with the oracle
    mine = shuffle_ops._f64_to_bf16(torch.from_numpy(x.copy()))
    sc.assert_same_bits(mine, one, sc.BF16, "f64 -> bf16")
    # exact midpoints go to the even neighbour, both up and down
    t = sc.bf16_ties(512, np.random.default_rng(0))
    r = sc.bf16_bits(sc.bf16_round(t))
    assert (r & 1 == 0).all()
    v = np.abs(sc.bf16_value(r))
    assert (v > np.abs(t)).any() and (v < np.abs(t)).any()


def test_f32_ties_present():
    x = sc.cast_inputs(sc.F32, sc.BF16, sc.CAST_ROWS * 4)
    u = x.view(np.uint32)
    fin = np.isfinite(x)
    tie = fin & ((u & 0xFFFF) == 0x8000)
    above = fin & ((u & 0xFFFF) == 0x8001)
    below = fin & ((u & 0xFFFF) == 0x7FFF)
    assert tie.sum() >= 500 and above.sum() >= 500 and below.sum() >= 500
    r = sc.cast_ref(x, sc.F32, sc.BF16).view(np.uint16)
    hi = (u >> 16).astype(np.uint16)
    # ties to even: up where the kept bits are odd, down where even
    assert np.array_equal(r[tie], hi[tie] + (hi[tie] & 1))
    assert (hi[tie] & 1 == 1).any() and (hi[tie] & 1 == 0).any()
    assert np.array_equal(r[above], hi[above] + 1)
    assert np.array_equal(r[below], hi[below])


def test_int_edges_against_exact_arithmetic():
    for src, sig in ((sc.I64, None), (sc.I32, None)):
        x = sc.cast_inputs(src, sc.F32, sc.CAST_ROWS * 4)
        ints = [int(v) for v in x]
        f32 = sc.cast_ref(x, src, sc.F32)
        f64 = sc.cast_ref(x, src, sc.F64)
        assert [int(v) for v in f32] == [
            sc.round_int_to_bits(v, 24) for v in ints]
        assert [int(v) for v in f64] == [
            sc.round_int_to_bits(v, 53) for v in ints]
        assert sum(int(a) != b for a, b in zip(f32, ints)) > 100
        if src == sc.I64:
            for e in ((1 << 62) + 1, -(1 << 62) - 1):
                assert e in ints
            assert float(f64[ints.index((1 << 62) + 1)]) == 2.0 ** 62
            assert sum(int(a) != b for a, b in zip(f64, ints)) > 100
        else:
            assert max(ints) > 1 << 24 and (1 << 24) + 1 in ints
    # int -> bf16 is via f32: differs from one rounding on this value
    v = np.array([(1 << 30) + (1 << 22) + 1], dtype=np.int64)
    via = sc.bf16_value(sc.cast_ref(v, sc.I64, sc.BF16))[0]
    direct = sc.bf16_round(np.array([float(v[0])]))[0]
    assert via == 2.0 ** 30 and direct == 2.0 ** 30 + 2.0 ** 23


def test_float_to_int_edges_present():
    x = sc.cast_inputs(sc.F64, sc.I32, sc.CAST_ROWS * 4)
    r = sc.cast_ref(x, sc.F64, sc.I32)
    assert r.max() == 2**31 - 1 and r.min() == -(2**31)
    assert (np.trunc(x) != x).sum() > 1000  # fractions: truncation matters
    assert ((x < 0) & (np.trunc(x) != np.floor(x))).any()
    x = sc.cast_inputs(sc.F32, sc.I64, sc.CAST_ROWS * 4)
    r = sc.cast_ref(x, sc.F32, sc.I64)
    assert r.min() == -(2**63) and r.max() == 2**63 - 2**39


def test_unknown_kernel_dtype_is_a_type_error():
    for dt in (torch.int16, torch.int8, torch.bool):
        with pytest.raises(TypeError, match=str(dt).replace(".", r"\.")):
            shuffle_ops._dtype_code(dt)
