"""Narrowed source cache (RSDL_NARROW_CACHE), CPU side.

Ops level: ``unpack_permute(narrow_rows(packed), narrow, perm)`` must equal
``unpack_permute(packed, schema, perm, out_dtypes, affine, nan_fill)`` bit
for bit (integer views, so NaNs compare too), and the narrow rows' padding
bytes must be zero. Engine level: knob 0 and knob 1 must hand the consumer
the identical partition sequence."""

import os
import tempfile

import pytest
import torch

from _narrow_cases import (
    CPU,
    FEATS as _FEATS,
    LAYOUTS,
    Recorder as _Recorder,
    assert_same_bits as _assert_same_bits,
    assert_same_sequence as _assert_same_sequence,
    bits as _bits,
    layout_columns,
    random_affine as _affine_for,
    run_engine,
    write_files as _write_files,
)
from _normalize_cases import mixed_columns, pack, wide_columns

from ray_shuffling_data_loader_amd.ops import shuffle_ops
from ray_shuffling_data_loader_amd.utils.schema import ColumnSpec, Schema

# (columns factory, out_dtypes, standardized columns)
_OPS_CASES = {
    "mixed_bf16": (
        lambda n: mixed_columns(n),
        {"d": torch.bfloat16, "s": torch.bfloat16, "v": torch.bfloat16,
         "big": torch.float32, "j": torch.float32, "k": torch.int32},
        ("d", "v", "j"),
    ),
    "wide_key": (
        lambda n: wide_columns(n, True),
        {"w": torch.bfloat16, "d": torch.float32, "v8": torch.bfloat16,
         "v3": torch.bfloat16, "j": torch.float32},
        ("w", "v8", "v3", "j"),
    ),
    "wide_nokey_f32": (
        lambda n: wide_columns(n, False),
        {"w": torch.float32, "d": torch.float32},
        ("w",),
    ),
}
for _l in LAYOUTS:
    _OPS_CASES["layout_" + _l] = (
        lambda n, _l=_l: layout_columns(_l, n)[0],
        layout_columns(_l, 1)[1],
        layout_columns(_l, 1)[2],
    )


@pytest.mark.parametrize("case", sorted(_OPS_CASES))
@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("mode", ["plain", "affine", "affine_fill"])
def test_narrow_then_unpack_equals_unpack(case, n, mode):
    make, out_dtypes, norm = _OPS_CASES[case]
    cols = make(n)
    packed, schema = pack(cols)
    affine = _affine_for(cols, norm) if mode != "plain" else None
    nan_fill = -1.5 if mode == "affine_fill" else None
    narrow = shuffle_ops.narrow_schema(schema, out_dtypes)
    assert narrow.row_stride < schema.row_stride
    block = shuffle_ops.narrow_rows(
        packed, schema, narrow, affine=affine, nan_fill=nan_fill
    )
    assert block.shape == (n, narrow.row_stride)
    assert block.dtype == torch.uint8
    # padding bytes are zero
    assert int(block[:, narrow.payload_bytes:].sum()) == 0
    g = torch.Generator().manual_seed(n)
    for perm in (None, torch.randperm(n, generator=g)):
        want = shuffle_ops.unpack_permute(
            packed, schema, perm, out_dtypes=out_dtypes, affine=affine,
            nan_fill=nan_fill,
        )
        got = shuffle_ops.unpack_permute(block, narrow, perm)
        _assert_same_bits(got, want, (case, n, mode, perm is not None))


def test_narrow_schema_keeps_names_order_and_rules():
    schema = Schema(
        [
            ColumnSpec("features", torch.float64, 100),
            ColumnSpec("labels", torch.float64, 1),
        ]
    )
    narrow = shuffle_ops.narrow_schema(schema, {"features": torch.bfloat16})
    assert narrow.names == schema.names
    # descending dtype size: the 8-B label first, 200 B of bf16 behind it
    assert narrow.offsets == {"labels": 0, "features": 8}
    assert (schema.row_stride, narrow.row_stride) == (816, 208)
    assert shuffle_ops.row_sweep_ok(narrow)


def test_narrow_supported_pairs():
    schema = Schema(
        [ColumnSpec("a", torch.float64, 4), ColumnSpec("b", torch.int32, 1)]
    )
    ok = shuffle_ops.narrow_schema(schema, {"a": torch.bfloat16})
    assert shuffle_ops.narrow_supported(schema, ok)
    # no cast kernel writes float16
    f16 = shuffle_ops.narrow_schema(schema, {"a": torch.float16})
    assert not shuffle_ops.narrow_supported(schema, f16)
    with pytest.raises(TypeError):
        shuffle_ops.narrow_rows(
            torch.zeros(2, schema.row_stride, dtype=torch.uint8), schema, f16
        )


def test_cpu_unpack_accepts_half_sources():
    n = 37
    g = torch.Generator().manual_seed(5)
    cols = {
        "h": torch.randn(n, 6, generator=g).to(torch.float16),
        "b": torch.randn(n, 3, generator=g).to(torch.bfloat16),
        "x": torch.randn(n, generator=g, dtype=torch.float64),
    }
    schema = Schema.from_columns(cols)
    # pack through integer views: the CPU pack has no bfloat16 either
    packed = torch.zeros(n, schema.row_stride, dtype=torch.uint8)
    pn = packed.numpy()
    for name, t in cols.items():
        spec = schema.col(name)
        np_dt = shuffle_ops._np_storage_dtype(spec.dtype)
        view = shuffle_ops._np_strided_view(
            pn, schema, name, spec.numel, np_dt)
        src = t.reshape(n, spec.numel)
        if t.dtype == torch.bfloat16:
            src = src.view(torch.int16)
        view[:] = src.numpy()
    perm = torch.randperm(n, generator=g)
    got = shuffle_ops.unpack_permute(packed, schema, perm)
    _assert_same_bits(got, {k: v[perm] for k, v in cols.items()})


# ----- engine -----------------------------------------------------------------


def _run_engine(monkeypatch, knob, filenames, **kw):
    rec, eng = run_engine(monkeypatch, knob, filenames, **kw)
    return rec.columns(), eng


_ENGINE_CASES = {
    "bf16": dict(out_dtypes={"x": torch.bfloat16}),
    "fp32": dict(out_dtypes={"x": torch.float32}),
    "bf16_two_trainers": dict(
        out_dtypes={"x": torch.bfloat16}, num_trainers=2),
    "standard": dict(
        out_dtypes={"x": torch.bfloat16}, normalize="standard"),
    "standard_fill": dict(
        out_dtypes={"x": torch.bfloat16}, normalize=["x", "cnt"],
        nan_fill=0.0),
    "standard_two_trainers_fp32": dict(
        out_dtypes={"x": torch.float32}, normalize=["x"], num_trainers=2),
    "host_cache": dict(
        out_dtypes={"x": torch.bfloat16}, source_cache="host"),
    "resume": dict(
        out_dtypes={"x": torch.bfloat16}, normalize=["x"], start_epoch=1),
}


@pytest.mark.parametrize("case", sorted(_ENGINE_CASES))
def test_engine_knob_on_equals_knob_off(tmp_path, monkeypatch, case):
    filenames = _write_files(str(tmp_path))
    kw = dict(_ENGINE_CASES[case], feature_matrix=("x", _FEATS))
    off, eng0 = _run_engine(monkeypatch, "0", filenames, **dict(kw))
    on, eng1 = _run_engine(monkeypatch, "1", filenames, **dict(kw))
    assert eng0._narrow_schema is None
    assert eng1._narrow_schema is not None
    assert eng0._cached_source.shape[1] == eng0.base_schema.row_stride
    assert eng1._cached_source.shape[1] == eng1._narrow_schema.row_stride
    assert eng1._narrow_schema.row_stride < eng1.base_schema.row_stride
    _assert_same_sequence(on, off)
    if kw.get("normalize") is not None:
        s0, s1 = eng0.column_stats(1), eng1.column_stats(1)
        for name in s0:
            for a, b in zip(s0[name], s1[name]):
                assert torch.equal(_bits(a), _bits(b)), name
    if case == "resume":
        # the resumed epoch is the one a full run produces
        full, _ = _run_engine(monkeypatch, "1", filenames,
                              **dict(kw, start_epoch=0))
        _assert_same_sequence(
            on, {k: v for k, v in full.items() if k[1] == 1})


def test_engine_keeps_wide_cache_when_not_smaller(tmp_path, monkeypatch):
    filenames = _write_files(str(tmp_path))
    # int32 -> float32 keeps every column's width: nothing to gain
    out, eng = _run_engine(
        monkeypatch, "1", filenames, normalize=["cnt"],
        feature_matrix=("x", _FEATS))
    assert eng._narrow_schema is None
    assert eng._cached_source.shape[1] == eng.base_schema.row_stride
    assert out[(0, 0)][0]["cnt"].dtype == torch.float32
    # not cached: nothing to narrow
    _, eng = _run_engine(
        monkeypatch, "1", filenames, out_dtypes={"x": torch.bfloat16},
        feature_matrix=("x", _FEATS), source_cache="none")
    assert eng._narrow_schema is None and eng._cached_source is None
    # the views path is untouched
    _, eng = _run_engine(
        monkeypatch, "1", filenames, feature_matrix=("x", _FEATS),
        output="views")
    assert eng._narrow_schema is None


# ----- two ranks over gloo ----------------------------------------------------


def _narrow_rank(rank, world, init_method, filenames, result_q):
    try:
        import torch.distributed as dist

        dist.init_process_group(
            "gloo", init_method=init_method, rank=rank, world_size=world
        )
        from ray_shuffling_data_loader_amd.engine import ShuffleEngine

        runs = {}
        for knob in ("0", "1"):
            os.environ["RSDL_NARROW_CACHE"] = knob
            rec = _Recorder()
            eng = ShuffleEngine(
                filenames, rec, num_epochs=2, num_reducers=4,
                num_trainers=world, rank=rank, device=CPU, seed=42,
                feature_matrix=("x", _FEATS),
                out_dtypes={"x": torch.bfloat16}, normalize=["x"],
            )
            eng.run()
            assert (eng._narrow_schema is not None) == (knob == "1")
            runs[knob] = {
                key: [
                    {n: p[n].clone() for n in p.columns}
                    for p in parts
                ]
                for key, parts in rec.parts.items()
            }
        _assert_same_sequence(runs["1"], runs["0"])
        rows = sum(
            p["key"].numel() for key, parts in runs["1"].items()
            if key[1] == 0 for p in parts
        )
        result_q.put((rank, rows))
        dist.destroy_process_group()
    except BaseException as e:  # surface to the parent
        import traceback

        result_q.put((rank, f"ERROR: {e}\n{traceback.format_exc()}"))


def test_distributed_knob_on_equals_knob_off(tmp_path, mp_spawn_context):
    filenames = _write_files(str(tmp_path), num_files=4, rows=300)
    world = 2
    port_file = tempfile.NamedTemporaryFile(delete=False)
    init_method = f"file://{port_file.name}"
    os.unlink(port_file.name)
    ctx = mp_spawn_context
    result_q = ctx.Queue()
    procs = [
        ctx.Process(
            target=_narrow_rank,
            args=(r, world, init_method, filenames, result_q),
        )
        for r in range(world)
    ]
    for p in procs:
        p.start()
    rows = {}
    for _ in range(world):
        rank, out = result_q.get(timeout=180)
        assert not isinstance(out, str), out
        rows[rank] = out
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the narrow rows crossed the exchange: every row arrived exactly once
    assert rows[0] + rows[1] == 4 * 300
    assert min(rows.values()) > 4 * 300 // 4
