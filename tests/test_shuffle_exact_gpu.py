"""GPU: the loader's shuffle kernels (gather_rows, pack_columns,
pack_columns_tiled, unpack_permute, partition_build_perm) against the numpy
oracle of tests/_shuffle_cases.py. Every comparison is byte-exact: there is
no tolerance in this file. Unpack inputs come from the oracle's pack, so a
pack bug cannot cancel an unpack bug."""

import numpy as np
import pytest
import torch

import _shuffle_cases as sc
from ray_shuffling_data_loader_amd.ops import shuffle_ops
from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
    gather_rows,
    pack_columns,
    partition_rows,
    row_sweep_ok,
    unpack_permute,
)
from ray_shuffling_data_loader_amd.utils.schema import ColumnSpec, Schema

pytestmark = pytest.mark.gpu

ALL_DTYPES = (sc.F32, sc.F64, sc.I32, sc.I64, sc.F16, sc.BF16, sc.U8)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd import _rsdl_hip

    return _rsdl_hip


def _up(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a))
    return t.to(dev) if dtype is None else t.to(dev).to(dtype)


def _descr(schema):
    """(offsets, dtype codes) in declared column order, as the bindings
    take them."""
    return (
        [schema.offsets[c.name] for c in schema.columns],
        [shuffle_ops._dtype_code(c.dtype) for c in schema.columns],
    )


def _assert_payload(got, want, schema, what):
    """Payload bytes only: the pack kernels leave padding undefined."""
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (
        what, got.shape, want.shape)
    m = sc.payload_mask(schema)
    if np.array_equal(got[:, m], want[:, m]):
        return
    # Not the same bytes: read both back column by column (plain views, no
    # cast), which names the column and lets a NaN the pack's cast made
    # equal the oracle's NaN whatever its payload.
    g, w = sc.unpack_ref(got, schema), sc.unpack_ref(want, schema)
    for spec in schema.columns:
        sc.assert_same_bits(
            g[spec.name], w[spec.name], spec.dtype, (what, spec.name))


def _assert_columns(got, want, dtypes, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name, w in want.items():
        assert got[name].dtype == dtypes[name], (what, name, got[name].dtype)
        sc.assert_same_bits(got[name], w, dtypes[name], (what, name))


# ----- pack -----------------------------------------------------------------


@pytest.mark.parametrize("name,n", sc.SCHEMA_CASES)
def test_pack_tiled_and_scatter(dev, name, n):
    schema = sc.schema_of(name)
    cols = sc.schema_columns(name, n)
    tcols = sc.cols_to_torch(cols, sc.schema_dtypes(schema), dev)
    got = pack_columns(tcols, schema)  # no perm: the LDS-tiled kernel
    _assert_payload(got, sc.schema_packed(name, n), schema, (name, n, "tiled"))
    scatter = sc.perm_cases(n)["full"]
    got = pack_columns(tcols, schema, perm=_up(scatter, dev))
    _assert_payload(
        got, sc.pack_ref(cols, schema, scatter), schema, (name, n, "scatter"))


@pytest.mark.parametrize("name", ("het", "fast84", "ladder", "wide"))
def test_pack_entry_points_by_name(dev, hip, name):
    """The two bindings called directly, so neither can stand in for the
    other unnoticed behind ops.pack_columns."""
    schema = sc.schema_of(name)
    n = sc.ROWS[name][-1]
    cols = sc.schema_columns(name, n)
    tcols = sc.cols_to_torch(cols, sc.schema_dtypes(schema), dev)
    ordered = [tcols[c.name] for c in schema.columns]
    offs, codes = _descr(schema)
    want = sc.schema_packed(name, n)
    got = hip.pack_columns_tiled(ordered, offs, codes, schema.row_stride)
    _assert_payload(got, want, schema, (name, "pack_columns_tiled"))
    got = hip.pack_columns(ordered, offs, codes, schema.row_stride)
    _assert_payload(got, want, schema, (name, "pack_columns, no perm"))
    scatter = sc.perm_cases(n)["full"]
    got = hip.pack_columns(
        ordered, offs, codes, schema.row_stride, _up(scatter, dev))
    _assert_payload(got, sc.pack_ref(cols, schema, scatter), schema,
                    (name, "pack_columns, perm"))


@pytest.mark.parametrize("name", list(sc.SCHEMAS))
def test_pack_tiled_out_in_place(dev, name):
    """out= a row slice of a larger buffer: the rows outside stay put."""
    schema = sc.schema_of(name)
    n = sc.ROWS[name][-1]
    lo, extra = 3, 5
    buf = torch.full((lo + n + extra, schema.row_stride), SENTINEL,
                     dtype=torch.uint8, device=dev)
    tcols = sc.cols_to_torch(
        sc.schema_columns(name, n), sc.schema_dtypes(schema), dev)
    ret = pack_columns(tcols, schema, out=buf[lo : lo + n])
    assert ret.data_ptr() == buf[lo].data_ptr()
    _assert_payload(buf[lo : lo + n], sc.schema_packed(name, n), schema, name)
    assert bool((buf[:lo] == SENTINEL).all())
    assert bool((buf[lo + n :] == SENTINEL).all())


_PACK_CASTS = [(sc.I64, sc.F32), (sc.F64, sc.F32), (sc.F32, sc.BF16)]


@pytest.mark.parametrize("pair", _PACK_CASTS, ids=sc.cell_id)
def test_pack_casts_to_schema_dtype(dev, pair):
    """Tensors of another dtype than the schema's are cast while packing
    (the generic path of the tiled kernel)."""
    src, dst = pair
    schema = Schema([ColumnSpec("s", dst, 1), ColumnSpec("v", dst, 3)])
    n = sc.CAST_ROWS
    flat = sc.cast_inputs(src, dst, n * 4)
    cols = {"s": flat[:n], "v": flat[n:].reshape(n, 3)}
    dts = {"s": src, "v": src}
    tcols = sc.cols_to_torch(cols, dts, dev)
    want = sc.pack_ref(cols, schema, col_dtypes=dts)
    if dst == sc.BF16:
        assert schema.payload_bytes == 8
        assert not sc.has_subnormal(
            want[:, :8].copy().view(np.int16), sc.BF16)
    _assert_payload(pack_columns(tcols, schema), want, schema, (pair, "tiled"))
    scatter = sc.perm_cases(n)["full"]
    _assert_payload(
        pack_columns(tcols, schema, perm=_up(scatter, dev)),
        sc.pack_ref(cols, schema, scatter, col_dtypes=dts), schema,
        (pair, "scatter"))


def test_129_columns_raise(dev, hip):
    schema = Schema([ColumnSpec(f"f{i}", sc.F64, 1) for i in range(129)])
    cols = [torch.zeros(4, dtype=sc.F64, device=dev) for _ in range(129)]
    offs, codes = _descr(schema)
    with pytest.raises(RuntimeError, match="128 columns"):
        hip.pack_columns_tiled(cols, offs, codes, schema.row_stride)
    with pytest.raises(RuntimeError, match="128 columns"):
        hip.pack_columns(cols, offs, codes, schema.row_stride)
    packed = torch.zeros(4, schema.row_stride, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="128 columns"):
        hip.unpack_permute(packed, None, cols, offs, codes)


# ----- unpack_permute -------------------------------------------------------


@pytest.mark.parametrize("name,n", sc.SCHEMA_CASES)
def test_unpack_permute_exact(dev, name, n):
    schema = sc.schema_of(name)
    packed = sc.schema_packed(name, n)
    d_packed = _up(packed, dev)
    dts = sc.schema_dtypes(schema)
    for kind, perm in sc.perm_cases(n).items():
        d_perm = None if perm is None else _up(perm, dev)
        want = sc.unpack_ref(packed, schema, perm)
        got = unpack_permute(d_packed, schema, perm=d_perm)
        _assert_columns(got, want, dts, (name, n, kind))
        if row_sweep_ok(schema):
            got = unpack_permute(
                d_packed, schema, perm=d_perm, row_sweep=True)
            _assert_columns(got, want, dts, (name, n, kind, "row_sweep"))


def test_unpack_binding_by_name(dev, hip):
    name, n = "het", 4099
    schema = sc.schema_of(name)
    packed = sc.schema_packed(name, n)
    perm = sc.perm_cases(n)["repeats"]
    outs = [
        torch.empty((len(perm),) if c.numel == 1 else (len(perm), c.numel),
                    dtype=c.dtype, device=dev)
        for c in schema.columns
    ]
    offs, codes = _descr(schema)
    hip.unpack_permute(_up(packed, dev), _up(perm, dev), outs, offs, codes)
    want = sc.unpack_ref(packed, schema, perm)
    got = {c.name: o for c, o in zip(schema.columns, outs)}
    _assert_columns(got, want, sc.schema_dtypes(schema), name)


def test_sweep_schemas_exist():
    swept = [n for n in sc.SCHEMAS if row_sweep_ok(sc.schema_of(n))]
    assert {"vec_aligned", "vec_off8", "fast_only8"} <= set(swept), swept


@pytest.mark.parametrize("cell", sc.CAST_CELLS, ids=sc.cell_id)
def test_unpack_cast_matrix(dev, cell):
    src, dst = cell
    schema, _, packed = sc.cast_case(src, dst)
    d_packed = _up(packed, dev)
    out_dtypes = {"s": dst, "v": dst}
    for kind, perm in sc.perm_cases(sc.CAST_ROWS).items():
        got = unpack_permute(
            d_packed, schema, perm=None if perm is None else _up(perm, dev),
            out_dtypes=out_dtypes)
        want = sc.unpack_ref(packed, schema, perm, out_dtypes)
        _assert_columns(got, want, out_dtypes, (sc.cell_id(cell), kind))


@pytest.mark.parametrize("n", (257, 4099))
@pytest.mark.parametrize(
    "name", ("vec_aligned", "vec_off8", "vec_odd", "het"))
def test_unpack_f32_vectors_to_bf16(dev, name, n):
    """f32 -> bf16 on the vec4 path (vec_aligned) and on the scalar path it
    must fall back to, with constructed ties in every column."""
    schema = sc.schema_of(name)
    cols = dict(sc.schema_columns(name, n))
    out_dtypes = {}
    for spec in schema.columns:
        if spec.dtype == sc.F32:
            cols[spec.name] = sc.cast_inputs(
                sc.F32, sc.BF16, n * spec.numel, seed=spec.numel
            ).reshape(cols[spec.name].shape)
            out_dtypes[spec.name] = sc.BF16
    packed = sc.pack_ref(cols, schema)
    dts = {**sc.schema_dtypes(schema), **out_dtypes}
    for kind, perm in sc.perm_cases(n).items():
        got = unpack_permute(
            _up(packed, dev), schema,
            perm=None if perm is None else _up(perm, dev),
            out_dtypes=out_dtypes)
        want = sc.unpack_ref(packed, schema, perm, out_dtypes)
        for a, dt in ((want[k], dts[k]) for k in want):
            assert not sc.has_subnormal(a, dt)
        _assert_columns(got, want, dts, (name, n, kind))


# ----- gather_rows ----------------------------------------------------------


@pytest.mark.parametrize("perm_dtype", (torch.int64, torch.int32))
@pytest.mark.parametrize("stride", (16, 48, 416, 1024))
def test_gather_rows_exact(dev, stride, perm_dtype):
    n = 1031
    src = sc.rows_with_ids(n, stride)
    d_src = _up(src, dev)
    for kind in ("full", "subset", "repeats"):
        perm = sc.perm_cases(n)[kind]
        got = gather_rows(d_src, _up(perm, dev, perm_dtype))
        assert np.array_equal(got.cpu().numpy(), src[perm]), kind
    # out= longer than perm: the rows past perm.numel() stay put
    perm = sc.perm_cases(n)["subset"]
    out = torch.full((n + 7, stride), SENTINEL, dtype=torch.uint8, device=dev)
    ret = gather_rows(d_src, _up(perm, dev, perm_dtype), out=out)
    assert ret.shape[0] == len(perm) and ret.data_ptr() == out.data_ptr()
    assert np.array_equal(out[: len(perm)].cpu().numpy(), src[perm])
    assert bool((out[len(perm):] == SENTINEL).all())
    # n = 0
    empty = torch.empty(0, dtype=perm_dtype, device=dev)
    got = gather_rows(d_src, empty)
    assert tuple(got.shape) == (0, stride)
    gather_rows(d_src, empty, out=out)
    assert bool((out[len(perm):] == SENTINEL).all())
    assert np.array_equal(out[: len(perm)].cpu().numpy(), src[perm])


def test_gather_rows_refuses_24_byte_rows(dev):
    src = torch.zeros(8, 24, dtype=torch.uint8, device=dev)
    perm = torch.arange(8, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        gather_rows(src, perm)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        gather_rows(src, perm, out=torch.empty_like(src))


# ----- partition_build_perm / partition_rows --------------------------------

_PART_N = (0, 1, 255, 256, 257, 100_003, 266_243)


@pytest.mark.parametrize("num_dests", (1, 2, 257, 1024))
@pytest.mark.parametrize("n", _PART_N)
def test_partition_exact(dev, hip, n, num_dests):
    src = sc.rows_with_ids(n, 16)
    d_src = _up(src, dev)
    arange = np.arange(n, dtype=np.int64)
    for kind in sc.DEST_PATTERNS:
        dest = sc.dest_pattern(kind, n, num_dests)
        want_counts = np.bincount(dest, minlength=num_dests)
        for dest_dtype in (torch.int64, torch.int32):
            what = (n, num_dests, kind, dest_dtype)
            d_dest = _up(dest, dev, dest_dtype)
            perm, counts = hip.partition_build_perm(d_dest, num_dests)
            assert perm.dtype == torch.int32 and counts.dtype == torch.int64
            assert tuple(perm.shape) == (n,), what
            p = perm.cpu().numpy().astype(np.int64)
            assert np.array_equal(counts.cpu().numpy(), want_counts), what
            assert np.array_equal(np.sort(p), arange), what
            assert (np.diff(dest[p]) >= 0).all(), what
            grouped = gather_rows(d_src, perm)
            assert np.array_equal(grouped.cpu().numpy(), src[p]), what
            # the public op: its own perm (the order inside a destination
            # is not fixed), read back from the row ids the rows carry
            grouped, counts = partition_rows(d_src, d_dest, num_dests)
            assert counts.dtype == torch.int64
            assert np.array_equal(counts.cpu().numpy(), want_counts), what
            g = grouped.cpu().numpy()
            ids = np.ascontiguousarray(g[:, :8]).view(np.int64).reshape(n)
            assert np.array_equal(np.sort(ids), arange), what
            assert (np.diff(dest[ids]) >= 0).all(), what
            assert np.array_equal(g, src[ids]), what


# ----- dtypes outside the cast dispatch -------------------------------------


def _supported(src, dst):
    return src == dst or (src in sc.CAST_SRC and dst in sc.CAST_DST)


_SMALL = Schema([
    ColumnSpec("x", sc.F32, 1), ColumnSpec("h", sc.F16, 5),
    ColumnSpec("u", sc.U8, 1), ColumnSpec("b", sc.BF16, 2),
    ColumnSpec("u3", sc.U8, 3),
])


@pytest.mark.parametrize("n", (1, 255, 257, 4099))
def test_f16_bf16_u8_columns_round_trip(dev, n):
    """Same-dtype 2-B and 1-B columns are a byte copy in both pack kernels
    and in the unpack."""
    rng = np.random.default_rng(n)
    cols = {
        c.name: sc.random_column(
            c.dtype, (n,) if c.numel == 1 else (n, c.numel), rng)
        for c in _SMALL.columns
    }
    dts = sc.schema_dtypes(_SMALL)
    tcols = sc.cols_to_torch(cols, dts, dev)
    want = sc.pack_ref(cols, _SMALL)
    tiled = pack_columns(tcols, _SMALL)
    _assert_payload(tiled, want, _SMALL, (n, "tiled"))
    scatter = sc.perm_cases(n)["full"]
    got = pack_columns(tcols, _SMALL, perm=_up(scatter, dev))
    _assert_payload(got, sc.pack_ref(cols, _SMALL, scatter), _SMALL,
                    (n, "scatter"))
    perm = sc.perm_cases(n)["repeats"]
    back = unpack_permute(tiled, _SMALL, perm=_up(perm, dev))
    _assert_columns(back, sc.unpack_ref(want, _SMALL, perm), dts, n)


def _pair_inputs(src, dst, k):
    if src != dst and _supported(src, dst):
        return sc.cast_inputs(src, dst, k)
    return sc.random_column(src, (k,), np.random.default_rng(k))


@pytest.mark.parametrize("src", ALL_DTYPES, ids=lambda d: str(d)[6:])
def test_every_unpack_pair_is_exact_or_raises(dev, src):
    """packed dtype ``src`` -> tensor dtype ``dst`` for all 7 x 7 pairs:
    the oracle's bits, or an error that names the column and both dtypes.
    Never an unwritten tensor."""
    n = 257
    for dst in ALL_DTYPES:
        schema = Schema([ColumnSpec("ok", sc.F32, 1), ColumnSpec("c", src, 3)])
        cols = {"ok": sc.random_column(sc.F32, (n,), np.random.default_rng(1)),
                "c": _pair_inputs(src, dst, n * 3).reshape(n, 3)}
        packed = sc.pack_ref(cols, schema)
        call = lambda: unpack_permute(  # noqa: E731
            _up(packed, dev), schema, out_dtypes={"c": dst})
        if _supported(src, dst):
            want = sc.unpack_ref(packed, schema, None, {"c": dst})
            _assert_columns(call(), want, {"ok": sc.F32, "c": dst}, (src, dst))
        else:
            with pytest.raises(RuntimeError) as e:
                call()
            msg = str(e.value)
            assert "column 1" in msg, msg
            assert str(src)[6:] in msg and str(dst)[6:] in msg, msg


@pytest.mark.parametrize("src", ALL_DTYPES, ids=lambda d: str(d)[6:])
def test_every_pack_pair_is_exact_or_raises(dev, src):
    """tensor dtype ``src`` -> packed dtype ``dst``, both pack kernels."""
    n = 257
    scatter = sc.perm_cases(n)["full"]
    for dst in ALL_DTYPES:
        schema = Schema([ColumnSpec("ok", sc.F64, 1), ColumnSpec("c", dst, 3)])
        cols = {"ok": sc.random_column(sc.F64, (n,), np.random.default_rng(1)),
                "c": _pair_inputs(src, dst, n * 3).reshape(n, 3)}
        dts = {"ok": sc.F64, "c": src}
        tcols = sc.cols_to_torch(cols, dts, dev)
        for perm in (None, scatter):
            call = lambda: pack_columns(  # noqa: E731
                tcols, schema, perm=None if perm is None else _up(perm, dev))
            if _supported(src, dst):
                want = sc.pack_ref(cols, schema, perm, col_dtypes=dts)
                _assert_payload(call(), want, schema, (src, dst, perm is None))
            else:
                with pytest.raises(RuntimeError) as e:
                    call()
                msg = str(e.value)
                assert "column 1" in msg, msg
                assert str(src)[6:] in msg and str(dst)[6:] in msg, msg


def test_named_unsupported_pairs_raise(dev):
    """The three the issue names: f32 -> f16 and f16 -> f32 in unpack, and a
    bf16 tensor into an f32 schema in pack."""
    n = 8
    for src, dst in ((sc.F32, sc.F16), (sc.F16, sc.F32)):
        schema = Schema([ColumnSpec("c", src, 1)])
        packed = torch.zeros(n, 16, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match="column 0"):
            unpack_permute(packed, schema, out_dtypes={"c": dst})
    schema = Schema([ColumnSpec("c", sc.F32, 1)])
    # the standardizing unpack refuses what the plain one refuses
    aff = {"c": (torch.zeros(1, dtype=sc.F64), torch.ones(1, dtype=sc.F64))}
    with pytest.raises(RuntimeError, match="float32 to float16"):
        unpack_permute(packed, schema, out_dtypes={"c": sc.F16}, affine=aff)
    cols = {"c": torch.zeros(n, dtype=sc.BF16, device=dev)}
    with pytest.raises(RuntimeError, match="bfloat16 to float32"):
        pack_columns(cols, schema)
    with pytest.raises(RuntimeError, match="bfloat16 to float32"):
        pack_columns(cols, schema, perm=torch.arange(n, device=dev))


@pytest.mark.parametrize("dtype", (torch.int16, torch.int8, torch.bool))
def test_schema_dtype_without_kernel_is_a_type_error(dev, dtype):
    schema = Schema([ColumnSpec("c", dtype, 1)])
    cols = {"c": torch.zeros(8, device=dev).to(dtype)}
    with pytest.raises(TypeError, match=str(dtype).replace(".", r"\.")):
        pack_columns(cols, schema)
    packed = torch.zeros(8, 16, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError, match=str(dtype).replace(".", r"\.")):
        unpack_permute(packed, schema)


def test_read_files_packed_uint8_float16_columns(dev, tmp_path):
    """A Parquet file with uint8 and float16 columns: the GPU ingest gives
    the CPU path's payload bytes, which are the oracle's."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from ray_shuffling_data_loader_amd.io import (
        infer_schema,
        read_files_packed,
    )

    n = 1000
    rng = np.random.default_rng(11)
    cols = {
        "key": np.arange(n, dtype=np.int64),
        "h": sc.random_column(sc.F16, (n,), rng),
        "u": sc.random_column(sc.U8, (n,), rng),
        "x": sc.random_column(sc.F64, (n,), rng),
        "c": sc.random_column(sc.I32, (n,), rng),
    }
    path = str(tmp_path / "mixed.parquet")
    pq.write_table(pa.table(cols), path, row_group_size=300)
    schema = infer_schema(path)
    assert schema.col("h").dtype == sc.F16 and schema.col("u").dtype == sc.U8
    want = sc.pack_ref(cols, schema)
    cpu = read_files_packed([path], schema, torch.device("cpu"), 2)
    assert np.array_equal(cpu.numpy(), want)
    gpu = read_files_packed([path], schema, dev, 2)
    torch.cuda.synchronize()
    m = sc.payload_mask(schema)
    assert np.array_equal(gpu.cpu().numpy()[:, m], cpu.numpy()[:, m])
    _assert_payload(gpu, want, schema, "read_files_packed")
