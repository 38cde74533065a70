"""Shared inputs and checks for tests/test_normalize.py (CPU) and
tests/test_normalize_gpu.py (GPU): packed blocks with awkward columns, the
numpy fp64 reference statistics and the tolerances.

Tolerance for statistics (against numpy, and GPU against CPU):

    |dmean| <= 1e-12 * |mean| + 1e-10 * std        |dstd| <= 1e-10 * std

n <= 4099 fp64 additions carry at most n * 2^-53 ~ 4.6e-13 relative error on
sum|x - p|; the bounds leave about two orders of margin over that and over
numpy's own pairwise-sum error.
"""

import numpy as np
import torch

from ray_shuffling_data_loader_amd.ops import shuffle_ops
from ray_shuffling_data_loader_amd.utils.schema import Schema

ROW_COUNTS = (1, 63, 64, 65, 4099)

# bf16 keeps 8 significant bits: half an ulp (2^-8 relative at worst, just
# above a power of two) plus the fp32 rounding before it.
BF16_REL_BOUND = 2.0 ** -8 + 2.0 ** -23


def _sprinkle_nan(t: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    """About 1 % NaN, a few +-inf."""
    u = torch.rand(t.shape, generator=gen)
    t = t.clone()
    t[u < 0.01] = float("nan")
    t[(u >= 0.01) & (u < 0.012)] = float("inf")
    t[(u >= 0.012) & (u < 0.014)] = float("-inf")
    return t


def mixed_columns(n: int, seed: int = 0):
    """i64x1, f64x1, f32x1, f32x4, i32x1, a constant column, a
    ``1e9 + N(0,1)`` column and an all-NaN column."""
    g = torch.Generator().manual_seed(seed * 7919 + n)
    return {
        "k": torch.randint(-500, 1000, (n,), generator=g, dtype=torch.int64),
        "d": _sprinkle_nan(
            5.0 + 3.0 * torch.randn(n, generator=g, dtype=torch.float64), g
        ),
        "s": _sprinkle_nan(torch.randn(n, generator=g) * 0.25 - 2.0, g),
        "v": _sprinkle_nan(torch.randn(n, 4, generator=g) * 10.0, g),
        "j": torch.randint(0, 50, (n,), generator=g, dtype=torch.int32),
        "const": torch.full((n,), 3.25, dtype=torch.float64),
        "big": _sprinkle_nan(
            1e9 + torch.randn(n, generator=g, dtype=torch.float64), g
        ),
        "allnan": torch.full((n,), float("nan"), dtype=torch.float32),
    }


def wide_columns(n: int, with_key: bool, seed: int = 0):
    """A wide f64x100 feature matrix at packed offset 0, or behind an int64
    key at offset 8 (the include_key=True layout), plus f64x1, f32x8, f32x3,
    i32x1 and a label."""
    g = torch.Generator().manual_seed(seed * 104729 + n + int(with_key))
    cols = {}
    if with_key:
        cols["key"] = torch.randperm(n, generator=g).to(torch.int64) + 10**6
    scale = torch.logspace(-3, 6, 100, dtype=torch.float64)
    offset = torch.linspace(-1e6, 1e6, 100, dtype=torch.float64)
    cols["w"] = _sprinkle_nan(
        torch.randn(n, 100, generator=g, dtype=torch.float64) * scale
        + offset,
        g,
    )
    cols["d"] = _sprinkle_nan(
        1e6 + torch.randn(n, generator=g, dtype=torch.float64), g
    )
    cols["v8"] = _sprinkle_nan(torch.randn(n, 8, generator=g) + 100.0, g)
    cols["v3"] = _sprinkle_nan(torch.randn(n, 3, generator=g) * 1e-3, g)
    cols["j"] = torch.randint(-7, 900, (n,), generator=g, dtype=torch.int32)
    cols["lab"] = torch.rand(n, generator=g)
    return cols


def pack(cols):
    """(packed uint8 [n, row_stride] on the CPU, schema)."""
    schema = Schema.from_columns(cols)
    return shuffle_ops.pack_columns(cols, schema), schema


def numpy_stats(col: torch.Tensor):
    """(count, mean, std) per element in numpy fp64 over the finite values:
    np.nanmean / np.nanstd on values masked to finite."""
    x = col.reshape(col.shape[0], -1).numpy().astype(np.float64)
    x = np.where(np.isfinite(x), x, np.nan)
    count = np.isfinite(x).sum(0)
    mean = np.zeros(x.shape[1])
    std = np.zeros(x.shape[1])
    ok = count > 0
    if ok.any():
        mean[ok] = np.nanmean(x[:, ok], axis=0)
        std[ok] = np.nanstd(x[:, ok], axis=0)
    return count, mean, std


def assert_stats_close(got, count, mean, std, what=""):
    """``got`` is a ColumnStats; counts exact, mean/std within the module
    tolerance of the reference arrays."""
    assert got.count.dtype == torch.int64, what
    assert got.mean.dtype == torch.float64, what
    assert got.std.dtype == torch.float64, what
    g_count = got.count.numpy()
    g_mean = got.mean.numpy()
    g_std = got.std.numpy()
    count = np.asarray(count).reshape(-1)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    std = np.asarray(std, dtype=np.float64).reshape(-1)
    assert g_count.shape == count.shape, (what, g_count.shape, count.shape)
    assert (g_count == count).all(), (what, g_count, count)
    d_mean = np.abs(g_mean - mean)
    d_std = np.abs(g_std - std)
    tol_mean = 1e-12 * np.abs(mean) + 1e-10 * std
    tol_std = 1e-10 * std
    assert (d_mean <= tol_mean).all(), (
        what, "mean", float((d_mean - tol_mean).max()))
    assert (d_std <= tol_std).all(), (
        what, "std", float((d_std - tol_std).max()))


def assert_bits_equal(a: torch.Tensor, b: torch.Tensor, what=""):
    """Bit equality that can see NaN: torch.equal is False for any tensor
    holding a NaN, so the NaN positions must match and everything else must
    match bit for bit (so -0.0 != 0.0 here)."""
    a, b = a.cpu(), b.cpu()
    assert a.dtype == b.dtype and a.shape == b.shape, (
        what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.is_floating_point:
        na, nb = torch.isnan(a), torch.isnan(b)
        assert torch.equal(na, nb), (what, "NaN positions differ")
        ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[
            a.element_size()]
        zero = torch.zeros((), dtype=a.dtype)
        a = torch.where(na, zero, a).contiguous().view(ints)
        b = torch.where(nb, zero, b).contiguous().view(ints)
    assert torch.equal(a, b), (what, int((a != b).sum()))


__all__ = [
    "BF16_REL_BOUND",
    "ROW_COUNTS",
    "assert_bits_equal",
    "assert_stats_close",
    "mixed_columns",
    "numpy_stats",
    "pack",
    "wide_columns",
]
