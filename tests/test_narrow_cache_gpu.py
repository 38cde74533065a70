"""Narrowed source cache on the GPU: narrow_rows_kernel and the same-dtype
unpack (one grid pass per column, and the row-major sweep) against their CPU
mirrors, and the engine with RSDL_NARROW_CACHE 0 against 1. Layouts and
checks are shared with the CPU tests in tests/_narrow_cases.py."""

import pytest
import torch

from _narrow_cases import (
    FEATS,
    LAYOUTS,
    assert_same_bits,
    assert_same_sequence,
    layout_columns,
    random_affine,
    run_engine,
    typed_columns,
    write_files,
)
from _normalize_cases import pack

from ray_shuffling_data_loader_amd.ops import shuffle_ops

pytestmark = pytest.mark.gpu

# None is a multiple of the 256-thread block.
ROW_COUNTS = (1, 63, 257, 1000)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


_CASE_CACHE = {}


def _case(layout, n, mode):
    """The packed block, its CPU narrow block and the CPU reference columns
    (identity order), computed once per (layout, n, mode)."""
    key = (layout, n, mode)
    if key not in _CASE_CACHE:
        cols, out_dtypes, norm = layout_columns(layout, n)
        packed, schema = pack(cols)
        affine = random_affine(cols, norm) if mode != "plain" else None
        nan_fill = -1.5 if mode == "affine_fill" else None
        narrow = shuffle_ops.narrow_schema(schema, out_dtypes)
        block = shuffle_ops.narrow_rows(
            packed, schema, narrow, affine=affine, nan_fill=nan_fill)
        _CASE_CACHE[key] = dict(
            packed=packed, schema=schema, narrow=narrow, affine=affine,
            nan_fill=nan_fill, out_dtypes=out_dtypes, block=block,
            ref=typed_columns(block, narrow),
        )
    return _CASE_CACHE[key]


def test_layouts_are_what_they_claim():
    a = _case("a", 63, "plain")
    assert (a["schema"].row_stride, a["narrow"].row_stride) == (816, 208)
    assert a["narrow"].offsets == {"labels": 0, "features": 8}
    b = _case("b", 63, "plain")
    assert b["schema"].offsets["features"] % 16 == 8
    c = _case("c", 63, "plain")
    assert c["narrow"].payload_bytes < c["narrow"].row_stride  # has padding


@pytest.mark.parametrize("mode", ["plain", "affine", "affine_fill"])
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_narrow_rows_kernel_matches_cpu(dev, layout, n, mode):
    c = _case(layout, n, mode)
    got = shuffle_ops.narrow_rows(
        c["packed"].to(dev), c["schema"], c["narrow"], affine=c["affine"],
        nan_fill=c["nan_fill"],
    )
    assert got.shape == c["block"].shape and got.dtype == torch.uint8
    got = got.cpu()
    pad = got[:, c["narrow"].payload_bytes:]
    assert int(pad.to(torch.int64).sum()) == 0, "padding bytes must be zero"
    assert_same_bits(
        typed_columns(got, c["narrow"]), c["ref"], (layout, n, mode))


@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_narrow_unpack_kernels_match_cpu(dev, layout, n, with_perm):
    c = _case(layout, n, "affine_fill")
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(n, generator=g) if with_perm else None
    want = shuffle_ops.unpack_permute(c["block"], c["narrow"], perm)
    block = c["block"].to(dev)
    perm_d = perm.to(dev) if with_perm else None
    got = shuffle_ops.unpack_permute(block, c["narrow"], perm_d)
    # a copy: every bit, NaN payloads included
    assert_same_bits(got, want, (layout, n, "columns"), nan_payload=True)
    if shuffle_ops.row_sweep_ok(c["narrow"]):
        got = shuffle_ops.unpack_permute(
            block, c["narrow"], perm_d, row_sweep=True)
        assert_same_bits(got, want, (layout, n, "sweep"), nan_payload=True)
    else:
        assert layout in ("c", "d")  # the flagship rows do take the sweep


@pytest.mark.parametrize("mode", ["plain", "affine", "affine_fill"])
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_narrow_then_unpack_equals_fused_unpack_on_gpu(dev, layout, n, mode):
    """The invariant the engine relies on, kernel against kernel: every bit
    of every column, NaN payloads included."""
    c = _case(layout, n, mode)
    packed = c["packed"].to(dev)
    g = torch.Generator().manual_seed(n + 1)
    perm = torch.randperm(n, generator=g).to(dev)
    want = shuffle_ops.unpack_permute(
        packed, c["schema"], perm, out_dtypes=c["out_dtypes"],
        affine=c["affine"], nan_fill=c["nan_fill"],
    )
    block = shuffle_ops.narrow_rows(
        packed, c["schema"], c["narrow"], affine=c["affine"],
        nan_fill=c["nan_fill"],
    )
    for sweep in (False, True):
        got = shuffle_ops.unpack_permute(
            block, c["narrow"], perm, row_sweep=sweep)
        assert_same_bits(
            got, want, (layout, n, mode, sweep), nan_payload=True)


def test_misaligned_block_takes_narrower_lanes(dev):
    """A block that starts 8 B into a 16-B line (a row slice of a wider
    tensor cannot; a byte-offset view can): the kernels must read the real
    pointer alignment, not the schema offsets."""
    c = _case("a", 257, "affine")
    n, stride = c["packed"].shape
    raw = torch.zeros(n * stride + 16, dtype=torch.uint8, device=dev)
    packed = raw[8 : 8 + n * stride].view(n, stride)
    packed.copy_(c["packed"])
    assert packed.data_ptr() % 16 == 8
    got = shuffle_ops.narrow_rows(
        packed, c["schema"], c["narrow"], affine=c["affine"])
    assert_same_bits(typed_columns(got, c["narrow"]), c["ref"], "narrow")
    nstride = c["narrow"].row_stride
    raw2 = torch.zeros(n * nstride + 16, dtype=torch.uint8, device=dev)
    block = raw2[4 : 4 + n * nstride].view(n, nstride)
    block.copy_(c["block"])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    want = shuffle_ops.unpack_permute(c["block"], c["narrow"], perm)
    got = shuffle_ops.unpack_permute(block, c["narrow"], perm.to(dev))
    assert_same_bits(got, want, "unpack at 4 mod 8", nan_payload=True)


# ----- engine -----------------------------------------------------------------


@pytest.mark.parametrize("normalize", [None, ["x"]])
def test_engine_gpu_knob_on_equals_knob_off(
        dev, tmp_path, monkeypatch, normalize):
    rows = 4096
    filenames = write_files(str(tmp_path), num_files=4, rows=rows // 4)
    kw = dict(
        feature_matrix=("x", FEATS), out_dtypes={"x": torch.bfloat16},
        normalize=normalize, device=dev,
    )
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    alloc, seqs, strides = {}, {}, {}
    for knob in ("0", "1"):
        rec, eng = run_engine(monkeypatch, knob, filenames, **dict(kw))
        torch.cuda.synchronize()
        seqs[knob] = rec.columns()
        del rec
        # what is left on the device is the engine's cached block (and its
        # small tables, the same for either knob)
        alloc[knob] = torch.cuda.memory_allocated(dev) - base
        strides[knob] = (
            eng._cached_source.shape[1], eng.base_schema.row_stride)
        assert eng._cached_source.is_cuda
        assert (eng._narrow_schema is not None) == (knob == "1")
        if knob == "1":
            assert eng._cached_source.shape[1] == (
                eng._narrow_schema.row_stride)
        del eng
    wide, narrow = strides["0"][0], strides["1"][0]
    assert wide == strides["1"][1] and narrow < wide
    # the wide block is gone: the footprint drops by exactly the difference
    # (both blocks are multiples of the allocator's 512-B granule)
    assert (rows * wide) % 512 == 0 and (rows * narrow) % 512 == 0
    assert alloc["0"] - alloc["1"] == rows * (wide - narrow), (alloc, strides)
    assert_same_sequence(seqs["1"], seqs["0"], nan_payload=True)
