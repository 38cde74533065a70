"""Shuffle hot ops: gather-permute, pack, unpack — HIP on GPU, torch/numpy on
CPU.

GPU tensors dispatch to the gfx950 HIP kernels in ``_rsdl_hip``
(csrc/shuffle_kernels.hip). If the extension is missing on a GPU box the ops
raise immediately — there is deliberately NO eager/PyTorch fallback on GPU,
so a silent-slow path can't masquerade as the native one. CPU tensors use
torch/numpy implementations, which double as the fp32 oracle for the GPU
numerics tests.

Reference ops replaced here: ``pd.concat`` + ``df.sample(frac=1)``
(reference shuffle.py:192-194) -> :func:`gather_rows`;
``convert_to_tensor`` column cast/pack (reference torch_dataset.py:204-236)
-> :func:`unpack_permute`.
"""

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import os

import numpy as np
import torch

from ray_shuffling_data_loader_amd.utils.schema import (
    ColumnSpec,
    Schema,
    TORCH_TO_NUMPY_DTYPE,
)

_hip = None
_hip_err = None


def _load_hip():
    global _hip, _hip_err
    if _hip is None and _hip_err is None:
        try:
            from ray_shuffling_data_loader_amd import _rsdl_hip

            _hip = _rsdl_hip
        except ImportError as e:  # remember why, re-raise on GPU use
            _hip_err = e
    if _hip is None:
        raise RuntimeError(
            "ray_shuffling_data_loader_amd._rsdl_hip extension is not built "
            "but a GPU tensor was passed to a shuffle op. Build it with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH="
            f"gfx950). Original import error: {_hip_err}"
        )
    return _hip


_DT_CODE = None

# The column dtypes the HIP pack/unpack kernels know (DType in
# csrc/shuffle_kernels.hip). Schema also lays out int16, int8 and bool
# columns; those exist on the CPU paths only.
_KERNEL_DTYPES = (
    torch.float32,
    torch.float64,
    torch.int32,
    torch.int64,
    torch.float16,
    torch.bfloat16,
    torch.uint8,
)


def _dtype_code(dtype: torch.dtype) -> int:
    global _DT_CODE
    if dtype not in _KERNEL_DTYPES:
        raise TypeError(
            f"the HIP shuffle kernels have no column dtype {dtype}; they "
            "know " + ", ".join(str(d) for d in _KERNEL_DTYPES)
        )
    if _DT_CODE is None:
        hip = _load_hip()
        _DT_CODE = {
            torch.float32: hip.DT_F32,
            torch.float64: hip.DT_F64,
            torch.int32: hip.DT_I32,
            torch.int64: hip.DT_I64,
            torch.float16: hip.DT_F16,
            torch.bfloat16: hip.DT_BF16,
            torch.uint8: hip.DT_U8,
        }
    return _DT_CODE[dtype]


# ---------------------------------------------------------------------------
# gather_rows: out[i,:] = src[perm[i],:]  on a packed byte matrix.
# ---------------------------------------------------------------------------


def gather_rows(
    src: torch.Tensor,
    perm: torch.Tensor,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Row gather of a 2-D contiguous tensor. The reducer-side full row
    permutation (reference shuffle.py:194) fused with the implicit concat.

    ``perm`` (int64 or int32) may be any selection: a subset, repeats, or
    empty. With ``out`` (at least ``perm.numel()`` rows) the result is its
    leading rows and the rest of ``out`` is left alone. On the GPU the
    indices are NOT checked: one outside ``[0, len(src))`` reads out of
    bounds."""
    if src.is_cuda:
        hip = _load_hip()
        if out is not None:
            hip.gather_rows_out(src, perm, out)
            return out[: perm.numel()]
        return hip.gather_rows(src, perm)
    res = torch.index_select(src, 0, perm.to(torch.long))
    if out is not None:
        out[: perm.numel()] = res
        return out[: perm.numel()]
    return res


# ---------------------------------------------------------------------------
# pack / unpack between column tensors and a packed row-major byte matrix.
# ---------------------------------------------------------------------------


def _np_strided_view(
    packed_np: np.ndarray, schema: Schema, name: str, numel: int, np_dt
) -> np.ndarray:
    """Writable strided numpy view of one column inside a packed row buffer."""
    n = packed_np.shape[0]
    stride = packed_np.shape[1]
    itemsize = np_dt.itemsize
    return np.ndarray(
        shape=(n, numel),
        dtype=np_dt,
        buffer=packed_np,
        offset=schema.offsets[name],
        strides=(stride, itemsize),
    )


def pack_columns(
    columns: Dict[str, torch.Tensor],
    schema: Schema,
    perm: Optional[torch.Tensor] = None,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Interleave column tensors into packed rows (cast to the schema dtype
    per column). ``perm`` scatters row i of the input to row perm[i] of the
    output.

    GPU: a column keeps its dtype (any of float32/64, int32/64, float16,
    bfloat16, uint8: a byte copy) or is cast from float32/64 or int32/64 to
    one of those or to bfloat16; every other pair raises before the launch
    (the table is in docs/PARITY.md). Padding bytes are undefined. ``perm``
    must be a permutation of the rows: it is NOT checked, and an index
    outside ``[0, n)`` writes out of bounds."""
    first = next(iter(columns.values()))
    n = first.shape[0]
    if first.is_cuda:
        hip = _load_hip()
        cols, offs, codes = [], [], []
        for spec in schema.columns:
            t = columns[spec.name]
            cols.append(t.contiguous())
            offs.append(schema.offsets[spec.name])
            codes.append(_dtype_code(spec.dtype))
        if perm is None:
            # LDS-tiled transpose pack: coalesced column reads + one
            # contiguous row-major store stream (optionally in place).
            return hip.pack_columns_tiled(
                cols, offs, codes, schema.row_stride, out
            )
        return hip.pack_columns(
            cols, offs, codes, schema.row_stride, perm
        )
    packed = (
        out
        if out is not None
        else torch.zeros(n, schema.row_stride, dtype=torch.uint8)
    )
    packed_np = packed.numpy()
    perm_np = perm.cpu().numpy() if perm is not None else None
    for spec in schema.columns:
        t = columns[spec.name].detach()
        np_dt = TORCH_TO_NUMPY_DTYPE[spec.dtype]
        view = _np_strided_view(packed_np, schema, spec.name, spec.numel, np_dt)
        src = t.cpu().numpy().reshape(n, spec.numel).astype(np_dt, copy=False)
        if perm_np is not None:
            view[perm_np] = src
        else:
            view[:] = src
    return packed


class AffineTable:
    """Per-element (shift, scale) of the standardized columns of one schema,
    validated once and, for a GPU device, uploaded once as the interleaved
    float64 ``[elems, 2]`` table the affine unpack kernel reads. Build it
    with :func:`make_affine_table`; :func:`unpack_permute` also accepts the
    plain ``{name: (shift, scale)}`` dict and builds one per call."""

    def __init__(self, entries, base, table):
        self.entries = entries  # name -> (shift[numel], scale[numel]) cpu f64
        self.base = base  # name -> index of element 0 in ``table``
        self.table = table  # float64 [elems, 2] on the device, or None (CPU)


def make_affine_table(
    affine: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
    schema: Schema,
    device=None,
) -> AffineTable:
    entries, base, rows = {}, {}, []
    n_elems = 0
    for name, (shift, scale) in affine.items():
        spec = schema.col(name)
        pair = []
        for t in (shift, scale):
            t = torch.as_tensor(t, dtype=torch.float64).detach().cpu()
            t = t.reshape(-1)
            if t.numel() == 1 and spec.numel > 1:
                t = t.expand(spec.numel)
            if t.numel() != spec.numel:
                raise ValueError(
                    f"affine entry for column {name!r} needs {spec.numel} "
                    f"elements, got {t.numel()}"
                )
            pair.append(t.contiguous())
        entries[name] = (pair[0], pair[1])
        base[name] = n_elems
        n_elems += spec.numel
        rows.append(torch.stack(pair, dim=1))
    table = None
    if device is not None and torch.device(device).type == "cuda":
        table = torch.cat(rows).contiguous().to(device)
    return AffineTable(entries, base, table)


def _np_storage_dtype(dtype: torch.dtype):
    """The numpy dtype a packed column is viewed as on the CPU paths. numpy
    has no bfloat16, so such a column moves as int16 (and is re-viewed)."""
    if dtype == torch.bfloat16:
        return np.dtype(np.int16)
    return TORCH_TO_NUMPY_DTYPE[dtype]


def _f64_to_bf16(t: torch.Tensor) -> torch.Tensor:
    """float64 -> bfloat16 in ONE rounding (nearest even), which is what the
    kernels' plain cast does (cast_elem<double, bf16> in
    csrc/shuffle_kernels.hip). torch's own ``.to(torch.bfloat16)`` rounds to
    float32 first and so differs wherever that float32 is a bf16 tie (about
    2^-17 of random inputs). Here the float32 step rounds to odd instead,
    after which the second rounding cannot go wrong."""
    f = t.float()
    back = f.double()
    fi = f.view(torch.int32)
    inexact = (back != t) & ~torch.isnan(t)
    even = (fi & 1) == 0
    one = torch.ones((), dtype=torch.int32)
    # toward the side the double lies on; for either sign the bit pattern
    # grows with the magnitude
    step = torch.where(t.abs() > back.abs(), one, -one)
    fi = torch.where(inexact & even, fi + step, fi)
    return fi.view(torch.float32).to(torch.bfloat16)


_SWEEP_MAX_COLS = 8  # RSDL_SWEEP_MAX_COLS in csrc/shuffle_kernels.hip


def row_sweep_ok(schema: Schema) -> bool:
    """Whether a same-dtype unpack of ``schema`` can run as one row-major
    sweep (``unpack_permute_sweep``): at most 8 columns, each made of whole
    8-B lanes of the packed row."""
    return 1 <= len(schema.columns) <= _SWEEP_MAX_COLS and all(
        schema.offsets[c.name] % 8 == 0 and c.row_bytes % 8 == 0
        for c in schema.columns
    )


def unpack_permute(
    packed: torch.Tensor,
    schema: Schema,
    perm: Optional[torch.Tensor] = None,
    out_dtypes: Optional[Dict[str, torch.dtype]] = None,
    affine: Union[
        None, AffineTable, Dict[str, Tuple[torch.Tensor, torch.Tensor]]
    ] = None,
    nan_fill: Optional[float] = None,
    row_sweep: bool = False,
) -> Dict[str, torch.Tensor]:
    """Fused gather-permute + per-column cast + pack into contiguous torch
    column tensors: out[name][i] = cast(packed[perm[i], off_name]).

    This single op replaces the reference's reduce-side
    concat+sample+convert_to_tensor chain (shuffle.py:192-194 +
    torch_dataset.py:204-236).

    ``affine`` (MI355X extension) maps a column name to float64
    ``(shift[numel], scale[numel])``; element e of such a column comes out as
    ``cast((float)((double(x) - shift[e]) * scale[e]))`` — standardized in
    fp64 BEFORE the narrowing cast, in the same kernel pass. With
    ``nan_fill``, a NaN source element of such a column becomes
    ``cast((float)nan_fill)``. Columns not named come out exactly as without
    the keyword; ``affine=None`` launches the plain kernel.

    A column whose dtype does not change is a byte copy, whatever the dtype
    (bf16/f16 columns of a block narrowed by :func:`narrow_rows` included).
    A column that does change goes from float32/64 or int32/64 to one of
    those or to bfloat16; on the GPU every other pair raises before the
    launch (docs/PARITY.md has the table). ``perm`` may be a subset or
    repeat rows; on the GPU its indices are NOT checked, and one outside the
    packed block reads out of bounds.
    ``row_sweep`` (GPU) asks for the one-pass row-major kernel where no
    column changes dtype and :func:`row_sweep_ok` holds; the outputs are the
    same."""
    out_dtypes = out_dtypes or {}
    n = perm.numel() if perm is not None else packed.shape[0]
    if affine is not None and not isinstance(affine, AffineTable):
        affine = make_affine_table(affine, schema, packed.device)
    if affine is not None and not affine.entries:
        affine = None
    if packed.is_cuda:
        hip = _load_hip()
        outs, offs, codes = [], [], []
        result: Dict[str, torch.Tensor] = {}
        for spec in schema.columns:
            dst_dt = out_dtypes.get(spec.name, spec.dtype)
            shape = (n,) if spec.numel == 1 else (n, spec.numel)
            o = torch.empty(shape, dtype=dst_dt, device=packed.device)
            outs.append(o)
            offs.append(schema.offsets[spec.name])
            codes.append(_dtype_code(spec.dtype))
            result[spec.name] = o
        if affine is None:
            if (
                row_sweep
                and row_sweep_ok(schema)
                and all(
                    o.dtype == spec.dtype
                    for o, spec in zip(outs, schema.columns)
                )
            ):
                hip.unpack_permute_sweep(packed, perm, outs, offs, codes)
                return result
            hip.unpack_permute(packed, perm, outs, offs, codes)
            return result
        table = affine.table
        if table is None or table.device != packed.device:
            table = make_affine_table(
                affine.entries, schema, packed.device
            ).table
        bases = [affine.base.get(spec.name, -1) for spec in schema.columns]
        hip.unpack_permute_affine(
            packed, perm, outs, offs, codes, table, bases, nan_fill
        )
        return result
    packed_np = packed.numpy()
    perm_np = perm.cpu().numpy() if perm is not None else None
    result = {}
    for spec in schema.columns:
        np_dt = _np_storage_dtype(spec.dtype)
        view = _np_strided_view(packed_np, schema, spec.name, spec.numel, np_dt)
        arr = view[perm_np] if perm_np is not None else np.ascontiguousarray(
            view
        )
        t = torch.from_numpy(arr)
        if t.dtype != spec.dtype:  # bf16 moved as int16
            t = t.view(spec.dtype)
        dst_dt = out_dtypes.get(spec.name, spec.dtype)
        if affine is not None and spec.name in affine.entries:
            # The bit-exact oracle of the affine kernel: fp64 subtract, fp64
            # multiply, round to fp32, then the fp32 -> dst conversion.
            shift, scale = affine.entries[spec.name]
            x = t.double()
            y = ((x - shift) * scale).float()
            if nan_fill is not None:
                y = torch.where(
                    torch.isnan(x),
                    torch.tensor(float(nan_fill), dtype=torch.float64)
                    .float(),
                    y,
                )
            t = y.to(dst_dt)
        elif dst_dt != spec.dtype:
            if spec.dtype == torch.float64 and dst_dt == torch.bfloat16:
                t = _f64_to_bf16(t)
            else:
                t = t.to(dst_dt)
        if spec.numel == 1:
            t = t.reshape(n)
        result[spec.name] = t
    return result


# ---------------------------------------------------------------------------
# Narrowed source block: the unpack's cast (and affine) done once.
# ---------------------------------------------------------------------------

# What the cast dispatch of the unpack kernels knows (csrc/shuffle_kernels.hip
# RSDL_DISPATCH_PAIR); a column that keeps its dtype is a byte copy.
_CAST_SRC_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)
_CAST_DST_DTYPES = _CAST_SRC_DTYPES + (torch.bfloat16,)


def narrow_schema(
    schema: Schema, out_dtypes: Optional[Dict[str, torch.dtype]] = None
) -> Schema:
    """The packed layout of ``schema``'s columns at their OUTPUT dtypes:
    same names, order and numel; the usual descending-size packing and 16-B
    stride rule apply."""
    out_dtypes = out_dtypes or {}
    return Schema(
        [
            ColumnSpec(c.name, out_dtypes.get(c.name, c.dtype), c.numel)
            for c in schema.columns
        ]
    )


def narrow_supported(
    schema: Schema, narrow: Schema, affine_names: Sequence[str] = ()
) -> bool:
    """Whether :func:`narrow_rows` can produce every column of ``narrow``
    from ``schema``: the dtype stays (a copy), or the pair is one the cast
    kernels know. A standardized column always goes through the cast."""
    for spec in schema.columns:
        dst = narrow.col(spec.name).dtype
        if spec.dtype == dst and spec.name not in affine_names:
            continue
        if spec.dtype not in _CAST_SRC_DTYPES or dst not in _CAST_DST_DTYPES:
            return False
    return True


def narrow_rows(
    packed: torch.Tensor,
    schema: Schema,
    narrow: Schema,
    affine: Union[
        None, AffineTable, Dict[str, Tuple[torch.Tensor, torch.Tensor]]
    ] = None,
    nan_fill: Optional[float] = None,
) -> torch.Tensor:
    """Wide packed rows -> packed rows of ``narrow`` (see
    :func:`narrow_schema`), identity row order, padding bytes zero.

    Per column this is exactly what :func:`unpack_permute` does with
    ``out_dtypes`` / ``affine`` / ``nan_fill``, so for any ``perm``

        unpack_permute(narrow_rows(packed, ...), narrow, perm)
        == unpack_permute(packed, schema, perm, out_dtypes, affine, nan_fill)

    bit for bit: the per-element cast commutes with the row gather. GPU: one
    launch of ``narrow_rows_kernel``. CPU: the numpy mirror built on the CPU
    path of :func:`unpack_permute` (the oracle)."""
    if affine is not None and not isinstance(affine, AffineTable):
        affine = make_affine_table(affine, schema, packed.device)
    if affine is not None and not affine.entries:
        affine = None
    aff_names = tuple(affine.entries) if affine is not None else ()
    if [c.name for c in narrow.columns] != schema.names:
        raise ValueError("narrow schema must list the same columns")
    if not narrow_supported(schema, narrow, aff_names):
        raise TypeError("narrow_rows: unsupported column dtype pair")
    n = packed.shape[0]
    if packed.is_cuda:
        hip = _load_hip()
        table = None
        if affine is not None:
            table = affine.table
            if table is None or table.device != packed.device:
                table = make_affine_table(
                    affine.entries, schema, packed.device
                ).table
        return hip.narrow_rows(
            packed,
            narrow.row_stride,
            narrow.payload_bytes,
            [schema.offsets[c.name] for c in schema.columns],
            [_dtype_code(c.dtype) for c in schema.columns],
            [narrow.offsets[c.name] for c in schema.columns],
            [_dtype_code(narrow.col(c.name).dtype) for c in schema.columns],
            [c.numel for c in schema.columns],
            table,
            [
                affine.base.get(c.name, -1) if affine is not None else -1
                for c in schema.columns
            ],
            nan_fill,
        )
    cols = unpack_permute(
        packed,
        schema,
        None,
        out_dtypes={c.name: c.dtype for c in narrow.columns},
        affine=affine,
        nan_fill=nan_fill,
    )
    out = torch.zeros(n, narrow.row_stride, dtype=torch.uint8)
    out_np = out.numpy()
    for spec in narrow.columns:
        np_dt = _np_storage_dtype(spec.dtype)
        view = _np_strided_view(out_np, narrow, spec.name, spec.numel, np_dt)
        t = cols[spec.name].reshape(n, spec.numel).contiguous()
        if spec.dtype == torch.bfloat16:
            t = t.view(torch.int16)
        view[:] = t.numpy()
    return out


# ---------------------------------------------------------------------------
# Column statistics: the fit behind ShuffleEngine(normalize=...).
# ---------------------------------------------------------------------------


class ColumnStats(NamedTuple):
    """Per-element statistics of one column over its finite values:
    ``count`` int64, ``mean`` and population ``std`` (ddof=0) float64, each
    of shape ``[numel]`` (host tensors)."""

    count: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor


_STATS_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)
_STATS_PIVOT_ROWS = 64  # RSDL_STATS_PIVOT_ROWS in csrc/shuffle_kernels.hip


def _finish_stats(count, s, ss, pivot) -> ColumnStats:
    """(count, sum(x-p), sum((x-p)^2), p) -> ColumnStats, fp64 on the host.
    Shared by the CPU and GPU paths."""
    count = count.to(torch.int64)
    nz = count > 0
    cnt = count.clamp(min=1).double()
    dmean = s / cnt
    var = (ss / cnt - dmean * dmean).clamp_(min=0.0)
    zero = torch.zeros_like(dmean)
    mean = torch.where(nz, pivot + dmean, zero)
    std = torch.where(nz, var.sqrt(), zero)
    return ColumnStats(count, mean, std)


def column_stats(
    packed: torch.Tensor,
    schema: Schema,
    columns: Optional[Sequence[str]] = None,
) -> Dict[str, ColumnStats]:
    """Per-element count / mean / population std of packed columns, skipping
    non-finite values, accumulated in fp64 about a per-element pivot (the
    first finite value, row 0 as a rule): a constant column has std exactly 0 and a ``1e9 + noise``
    column does not cancel. Integer columns accumulate as double.

    GPU: one read-only pass of the ``column_stats`` HIP kernel with a fixed
    grid and a block-ordered partial fold — no float atomics, so the same
    block gives the same bits on every call. CPU: numpy fp64 over the
    strided column views (the oracle). Results are host tensors."""
    names = list(columns) if columns is not None else [
        c.name for c in schema.columns if c.dtype in _STATS_DTYPES
    ]
    specs = [schema.col(nm) for nm in names]
    for spec in specs:
        if spec.dtype not in _STATS_DTYPES:
            raise TypeError(
                f"column_stats: unsupported dtype {spec.dtype} for column "
                f"{spec.name!r}"
            )
    n = packed.shape[0]
    if n == 0 or not specs:
        return {
            spec.name: ColumnStats(
                torch.zeros(spec.numel, dtype=torch.int64),
                torch.zeros(spec.numel, dtype=torch.float64),
                torch.zeros(spec.numel, dtype=torch.float64),
            )
            for spec in specs
        }
    if packed.is_cuda:
        hip = _load_hip()
        result = {}
        # RSDL_MAX_COLS columns per launch, as the ColTable ops.
        for lo in range(0, len(specs), 128):
            chunk = specs[lo : lo + 128]
            cnt, s, ss, piv = hip.column_stats(
                packed,
                [schema.offsets[c.name] for c in chunk],
                [_dtype_code(c.dtype) for c in chunk],
                [c.numel for c in chunk],
            )
            cnt, s, ss, piv = cnt.cpu(), s.cpu(), ss.cpu(), piv.cpu()
            e0 = 0
            for c in chunk:
                sl = slice(e0, e0 + c.numel)
                result[c.name] = _finish_stats(
                    cnt[sl], s[sl], ss[sl], piv[sl]
                )
                e0 += c.numel
        return result
    packed_np = packed.numpy()
    result = {}
    for spec in specs:
        np_dt = TORCH_TO_NUMPY_DTYPE[spec.dtype]
        x = _np_strided_view(
            packed_np, schema, spec.name, spec.numel, np_dt
        ).astype(np.float64)
        fin = np.isfinite(x)
        # Pivot: the first finite value among the leading rows (row 0 as a
        # rule), 0.0 if there is none — the kernel's rule.
        head = fin[:_STATS_PIVOT_ROWS]
        first = head.argmax(0)
        piv = np.where(
            head.any(0), x[first, np.arange(x.shape[1])], 0.0
        )
        d = np.where(fin, x - piv, 0.0)
        result[spec.name] = _finish_stats(
            torch.from_numpy(fin.sum(0)),
            torch.from_numpy(d.sum(0)),
            torch.from_numpy((d * d).sum(0)),
            torch.from_numpy(piv),
        )
    return result


def merge_column_stats(
    stats_list: Sequence[Dict[str, ColumnStats]],
) -> Dict[str, ColumnStats]:
    """Pairwise (Chan) merge of per-shard statistics as (count, mean, M2) in
    fp64, folded in list order — every caller that merges the same list gets
    the same bits. Empty shards (count 0) are neutral."""
    merged: Dict[str, ColumnStats] = {}
    if not stats_list:
        return merged
    for name in stats_list[0]:
        n_a = m_a = m2_a = None
        for st in stats_list:
            c = st[name]
            n_b = c.count.to(torch.int64)
            m_b = c.mean.double()
            m2_b = c.std.double() ** 2 * n_b.double()
            if n_a is None:
                n_a, m_a, m2_a = n_b.clone(), m_b.clone(), m2_b.clone()
                continue
            n = n_a + n_b
            nd = n.clamp(min=1).double()
            delta = m_b - m_a
            w_b = n_b.double() / nd
            # An empty side contributes nothing (and must not move the mean
            # by a rounding of delta * 0).
            m = torch.where(n_b == 0, m_a, torch.where(
                n_a == 0, m_b, m_a + delta * w_b))
            m2 = m2_a + m2_b + delta * delta * (n_a.double() * w_b)
            m2 = torch.where(n_b == 0, m2_a, torch.where(
                n_a == 0, m2_b, m2))
            n_a, m_a, m2_a = n, m, m2
        nz = n_a > 0
        nd = n_a.clamp(min=1).double()
        zero = torch.zeros_like(m_a)
        merged[name] = ColumnStats(
            n_a,
            torch.where(nz, m_a, zero),
            torch.where(nz, (m2_a / nd).clamp(min=0.0).sqrt(), zero),
        )
    return merged


def stats_to_affine(
    stats: Dict[str, ColumnStats],
) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """ColumnStats -> (shift, scale) with scale = 1/std in fp64 on the host,
    or 1.0 where std == 0 or count == 0 (the StandardScaler convention: a
    constant column becomes 0). The kernel never divides."""
    out = {}
    for name, st in stats.items():
        std = st.std.double()
        ok = (std > 0) & (st.count > 0)
        scale = torch.where(
            ok, 1.0 / torch.where(ok, std, torch.ones_like(std)),
            torch.ones_like(std),
        )
        out[name] = (st.mean.double().clone(), scale)
    return out


# ---------------------------------------------------------------------------
# Row partition by destination (map-side scatter; reference shuffle.py:156-161
# boolean-mask loop). v1: stable sort + native gather; the sort keys are tiny
# (uint8-range dest ids) so torch's radix sort is cheap next to the row move.
# ---------------------------------------------------------------------------


def partition_rows(
    packed: torch.Tensor,
    dest: torch.Tensor,
    num_dests: int,
):
    """Group packed rows by destination id. Returns (regrouped rows, counts
    per destination).

    GPU: fused histogram -> scan -> rank/scatter builds the gather
    permutation in two O(N) index passes (no radix sort); the row move is
    the roofline gather. Order within a destination is block-local (a full
    random permutation is applied downstream either way). CPU: stable
    argsort (order matches the reference's boolean-mask partition).

    ``dest`` is int64 or int32 and ``num_dests`` at most 1024 on the GPU,
    where the ids are NOT checked: one outside ``[0, num_dests)`` indexes
    the kernels' LDS counters out of bounds."""
    if packed.is_cuda:
        hip = _load_hip()
        perm, counts = hip.partition_build_perm(dest, num_dests)
        grouped = gather_rows(packed, perm)
        return grouped, counts
    counts = torch.bincount(dest, minlength=num_dests)
    order = torch.argsort(dest, stable=True)
    grouped = gather_rows(packed, order)
    return grouped, counts


# ---------------------------------------------------------------------------
# MFMA split-M weight gradient (trainer-side hot op; csrc/wgrad_kernel.hip).
# ---------------------------------------------------------------------------


def wgrad(dy: torch.Tensor, x: torch.Tensor, with_bias: bool = True):
    """dW = dy^T @ x (fp32) and db = dy.sum(0) in one fused MFMA kernel
    (bf16 inputs, split-M atomic reduction). CPU / non-bf16 fallback uses
    plain matmul."""
    if dy.is_cuda and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16:
        hip = _load_hip()
        dw, db = hip.wgrad_bf16(dy.contiguous(), x.contiguous(), with_bias)
        return dw, (db if with_bias else None)
    dw = dy.t().float() @ x.float()
    db = dy.float().sum(0) if with_bias else None
    return dw, db


# pi16 intra-chunk M-permutation: position p <-> row with bits 2 and 3
# of the 4-bit within-chunk index swapped (an involution). Under it each
# MFMA half-wave's own packed pairs are already contiguous 8-element
# runs, so the chain kernels' emission needs no cross-lane exchange; dW
# is invariant because M is the contraction dim of every consumer.
_PI16_IDX = [(p & 3) | ((p & 4) << 1) | ((p & 8) >> 1) for p in range(16)]


def t_frag_swizzle(t: torch.Tensor, pi16: bool = False) -> torch.Tensor:
    """[M, C] -> fragment-major layout of t^T: flat [C/32][Mp/16][2][32][8]
    (Mp = M padded to a 16-multiple with zero rows). This is the input
    layout of the fragment-major wgrad kernel (csrc/wgrad_frag.hip); the
    hot producers (bwd_chain dz^T, fwd_chain a^T) emit it directly — this
    torch implementation is the oracle/fallback. ``pi16`` applies the
    pi16 intra-chunk M-permutation (must match the producers' flag)."""
    m, c = t.shape
    mp = (m + 15) // 16 * 16
    if mp != m:
        t = torch.nn.functional.pad(t, (0, 0, 0, mp - m))
    v = t.reshape(mp // 16, 16, c)
    if pi16:
        v = v[:, _PI16_IDX]
    v = v.reshape(mp // 16, 2, 8, c // 32, 32)
    return v.permute(3, 0, 1, 4, 2).contiguous().reshape(-1)


_WGRAD_FRAG_CFG = {
    # (N, K) -> (nt_w, kt_w); see csrc/wgrad_frag.hip launch configs
    (512, 128): (2, 4),
    (256, 512): (1, 8),
    (128, 256): (1, 8),
}
# RSDL_WGRAD_SMALL_TILES=1: (1,4) tiles for the (1,8) shapes — 64 acc
# regs (3 waves/SIMD), and the depth-3 fenced loop when RSDL_WGRAD_SCHED
# is also on (csrc/wgrad_frag.hip launch configs).
_WGRAD_FRAG_SMALL = {
    (512, 128): (2, 4),
    (256, 512): (1, 4),
    (128, 256): (1, 4),
}


def wgrad_frag(at_frag: torch.Tensor, bt_frag: torch.Tensor, n: int,
               k: int, mchunks: int, variant: int = 0) -> torch.Tensor:
    """dW = dz^T @ src from pre-swizzled fragment inputs (fp32 [N,K]).
    ``variant``: 0 = the extension's default (RSDL_WGRAD_LDS, then the
    per-shape default), 1 = the direct kernel, 2 = the LDS-ring kernel
    (csrc/wgrad_frag.hip). Passed on only when non-zero, so stand-ins
    that predate the argument stay callable."""
    cfg = (
        _WGRAD_FRAG_SMALL
        if os.environ.get("RSDL_WGRAD_SMALL_TILES", "0") == "1"
        else _WGRAD_FRAG_CFG
    )
    nt_w, kt_w = cfg[(n, k)]
    hip = _load_hip()
    kw = {"variant": variant} if variant else {}
    return hip.wgrad_frag_bf16(at_frag, bt_frag, n, k, mchunks, nt_w, kt_w,
                               **kw)


def t_frag_unswizzle(
    flat: torch.Tensor, m: int, c: int, pi16: bool = False
) -> torch.Tensor:
    """Inverse of :func:`t_frag_swizzle`: fragment-major transposed flat
    tensor -> row-major [m, c] (pad rows dropped)."""
    mchunks = flat.numel() // (c * 16)
    v = flat.reshape(c // 32, mchunks, 2, 32, 8)
    v = v.permute(1, 2, 4, 0, 3).reshape(mchunks, 16, c)
    if pi16:
        v = v[:, _PI16_IDX]  # involution: same index recovers rows
    return v.reshape(mchunks * 16, c)[:m].contiguous()


def relu_mask_words(a: torch.Tensor) -> torch.Tensor:
    """[M, N] activations -> [ceil(M/32), N] int32 relu-mask words (bit i
    of word (t, n) = a[t*32+i, n] > 0; pad rows 0). Torch oracle for the
    mask layout the forward chain kernel emits."""
    m, n = a.shape
    mt = (m + 31) // 32
    pad = mt * 32 - m
    bits = a > 0
    if pad:
        bits = torch.cat(
            [bits, torch.zeros(pad, n, dtype=torch.bool, device=a.device)]
        )
    bits = bits.view(mt, 32, n).long()
    weights = (1 << torch.arange(32, device=a.device, dtype=torch.long))
    words = (bits * weights.view(1, 32, 1)).sum(1)
    return (words & 0xFFFFFFFF).to(torch.int32) if False else (
        words - ((words >> 31) & 1) * (1 << 32)
    ).to(torch.int32)
