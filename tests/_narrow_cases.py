"""Shared inputs and checks for tests/test_narrow_cache.py (CPU) and
tests/test_narrow_cache_gpu.py (GPU): bit comparisons, a consumer that
records what the engine hands it, small Parquet shards and the packed
layouts the narrowing kernels are checked on."""

import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

from ray_shuffling_data_loader_amd.ops import shuffle_ops
from ray_shuffling_data_loader_amd.utils.schema import Schema

CPU = torch.device("cpu")

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def assert_same_bits(a, b, what="", nan_payload=False):
    """``a`` and ``b`` map column names to tensors; compared as integer
    views, so -0.0 != 0.0 and a NaN only equals a NaN.

    ``nan_payload=False`` leaves the payload of a NaN out: torch's CPU
    float -> bf16 cast writes 0xFFFF in its vector body and 0x7FC0 in its
    scalar tail, so the payload the CPU oracle gives depends on where in the
    array the element sits. Two GPU results are compared with
    ``nan_payload=True``: there the cast is per element and every bit must
    agree."""
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for name in a:
        x, y = a[name].cpu(), b[name].cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, (
            what, name, x.dtype, y.dtype, x.shape, y.shape)
        bx, by = bits(x), bits(y)
        if x.dtype.is_floating_point and not nan_payload:
            nx, ny = torch.isnan(x), torch.isnan(y)
            assert torch.equal(nx, ny), (what, name, "NaN positions")
            bx = torch.where(nx, torch.zeros_like(bx), bx)
            by = torch.where(ny, torch.zeros_like(by), by)
        assert torch.equal(bx, by), (what, name, int((bx != by).sum()))


def typed_columns(block: torch.Tensor, schema: Schema):
    """The columns of a packed block in identity order, as typed tensors."""
    return shuffle_ops.unpack_permute(block.cpu(), schema, None)


def random_affine(cols, names, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for nm in names:
        k = 1 if cols[nm].dim() == 1 else cols[nm].shape[1]
        out[nm] = (
            torch.randn(k, generator=g, dtype=torch.float64) * 10.0,
            torch.rand(k, generator=g, dtype=torch.float64) + 0.5,
        )
    return out


# ----- engine -----------------------------------------------------------------


class Recorder:
    """A consumer that keeps every partition, in arrival order."""

    def __init__(self):
        self.parts = {}

    def wait_until_ready(self, epoch):
        pass

    def consume(self, trainer, epoch, parts):
        self.parts.setdefault((trainer, epoch), []).extend(parts)

    def producer_done(self, trainer, epoch):
        pass

    def wait_until_all_epochs_done(self):
        pass

    def columns(self):
        return {
            key: [{name: p[name].cpu() for name in p.columns} for p in parts]
            for key, parts in self.parts.items()
        }


FEATS = [f"f{i}" for i in range(12)]


def write_files(dirname, num_files=3, rows=400, seed=23, width=12):
    """key, ``width`` float64 features at different levels with a few NaN,
    an int32 count and a label."""
    rng = np.random.default_rng(seed)
    names = []
    for f in range(num_files):
        cols = {"key": np.arange(f * rows, (f + 1) * rows, dtype=np.int64)}
        for i in range(width):
            x = 1e3 * (i + 1) + 7.0 * rng.standard_normal(rows)
            x[rng.random(rows) < 0.02] = np.nan
            cols[f"f{i}"] = x
        cols["cnt"] = rng.integers(0, 1000, rows, dtype=np.int32)
        cols["label"] = rng.random(rows)
        path = os.path.join(dirname, f"part_{f}.parquet")
        pq.write_table(pa.table(cols), path)
        names.append(path)
    return names


def run_engine(monkeypatch, knob, filenames, device=CPU, num_epochs=2, **kw):
    """Run a ShuffleEngine to the end on this thread with
    RSDL_NARROW_CACHE=``knob``; returns (recorder, engine)."""
    from ray_shuffling_data_loader_amd.engine import ShuffleEngine

    monkeypatch.setenv("RSDL_NARROW_CACHE", knob)
    rec = Recorder()
    eng = ShuffleEngine(
        filenames, rec, num_epochs=num_epochs,
        num_reducers=kw.pop("num_reducers", 4),
        num_trainers=kw.pop("num_trainers", 1), device=device,
        seed=kw.pop("seed", 9), **kw,
    )
    eng.run()
    return rec, eng


def assert_same_sequence(a, b, nan_payload=False):
    assert sorted(a) == sorted(b)
    for key in a:
        assert len(a[key]) == len(b[key]), key
        for i, (pa_, pb_) in enumerate(zip(a[key], b[key])):
            assert_same_bits(pa_, pb_, (key, i), nan_payload)


# ----- kernel layouts ---------------------------------------------------------


def _awkward(t: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    """NaN, +-Inf, -0.0, subnormals and magnitudes above the bf16 maximum
    (3.39e38), a few per cent of each."""
    u = torch.rand(t.shape, generator=gen)
    t = t.clone()
    tiny = 1e-310 if t.dtype == torch.float64 else 1e-41
    over = 1e39 if t.dtype == torch.float64 else 3.4e38  # -> Inf in bf16
    for lo, val in (
        (0.00, float("nan")), (0.02, float("inf")), (0.03, float("-inf")),
        (0.04, -0.0), (0.06, tiny), (0.07, -tiny), (0.08, over),
        (0.09, -over), (0.10, 1e300 if t.dtype == torch.float64 else 1e-45),
    ):
        t[(u >= lo) & (u < lo + 0.01)] = val
    return t


def layout_columns(layout: str, n: int):
    """(columns, out_dtypes, standardized names) of one test layout:

    a  100 f64 features + f64 label -> bf16: the flagship row, 816 -> 208 B
    b  int64 key + 100 f64 features: the features at 8 mod 16 in the wide row
    c  f32 sources of numel 7 (scalar path) and 12 (vector path) -> bf16
    d  a mix (f64 -> f32, f32 at 8 mod 16, f64 x 7) with an int32 column
       standardized to float32
    """
    g = torch.Generator().manual_seed(n * 31 + ord(layout))
    f64 = dict(generator=g, dtype=torch.float64)
    if layout == "a":
        cols = {
            "features": _awkward(torch.randn(n, 100, **f64) * 50.0 + 3.0, g),
            "labels": torch.rand(n, **f64),
        }
        return cols, {"features": torch.bfloat16}, ("features",)
    if layout == "b":
        cols = {
            "key": torch.randperm(n, generator=g) + 10**12,
            "features": _awkward(torch.randn(n, 100, **f64) * 1e3, g),
        }
        return cols, {"features": torch.bfloat16}, ("features",)
    if layout == "c":
        # wide: v12 at 0 (16-B loads), v7 at 48; narrow: lab 0, wt 4, v12 at
        # 8 (8-B stores), v7 at 32, 46 B of payload in a 48-B row
        cols = {
            "v12": _awkward(torch.randn(n, 12, generator=g) - 4.0, g),
            "v7": _awkward(torch.randn(n, 7, generator=g) * 9.0, g),
            "lab": torch.rand(n, generator=g),
            "wt": torch.rand(n, generator=g),
        }
        return (
            cols,
            {"v7": torch.bfloat16, "v12": torch.bfloat16},
            ("v7", "v12"),
        )
    if layout == "d":
        # wide: k 0, lab 8, x 16 (f64, 16-B loads), w 48 (f64 x 7, scalar),
        # t 104 (f32 at 8 mod 16: 8-B loads), s 120, j 140, j2 144
        # narrow: k 0, lab 8, x 16 (16-B stores), j 32, j2 36, t 40 (8-B
        # stores), w 48, s 62; 72 B of payload in an 80-B row
        cols = {
            "k": torch.randint(-500, 1000, (n,), generator=g,
                               dtype=torch.int64),
            "lab": torch.rand(n, **f64),
            "x": _awkward(torch.randn(n, 4, **f64), g),
            "t": _awkward(torch.randn(n, 4, generator=g) * 3.0, g),
            "w": _awkward(torch.randn(n, 7, **f64) * 1e4, g),
            "s": _awkward(torch.randn(n, 5, generator=g), g),
            "j": torch.randint(0, 50, (n,), generator=g, dtype=torch.int32),
            "j2": torch.randint(-9, 9, (n,), generator=g, dtype=torch.int32),
        }
        return (
            cols,
            {"x": torch.float32, "t": torch.bfloat16, "w": torch.bfloat16,
             "s": torch.bfloat16, "j": torch.float32},
            ("x", "t", "w", "j"),
        )
    raise KeyError(layout)


LAYOUTS = ("a", "b", "c", "d")
