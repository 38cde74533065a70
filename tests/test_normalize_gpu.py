"""In-kernel feature standardization on the GPU: the column_stats HIP kernel
and the affine fused unpack against their CPU oracles, and the loader end to
end. Inputs, tolerances and the bit-equality check (which has to see through
NaN) are shared with the CPU tests in tests/_normalize_cases.py.
"""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from _normalize_cases import (
    BF16_REL_BOUND,
    ROW_COUNTS,
    assert_bits_equal,
    assert_stats_close,
    mixed_columns,
    pack,
    wide_columns,
)
from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
    column_stats,
    stats_to_affine,
    unpack_permute,
)

pytestmark = pytest.mark.gpu

GPU_ROW_COUNTS = ROW_COUNTS + (257,)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _blocks(n):
    """name -> (columns, packed cpu block, schema) for the three layouts."""
    out = {}
    for name, cols in (
        ("mixed", mixed_columns(n)),
        ("wide_off0", wide_columns(n, with_key=False)),
        ("wide_off8", wide_columns(n, with_key=True)),
    ):
        packed, schema = pack(cols)
        out[name] = (cols, packed, schema)
    assert out["wide_off0"][2].offsets["w"] == 0
    assert out["wide_off8"][2].offsets["w"] == 8
    return out


_BLOCK_CACHE = {}


def _cached_blocks(n):
    if n not in _BLOCK_CACHE:
        _BLOCK_CACHE[n] = _blocks(n)
    return _BLOCK_CACHE[n]


# ----- 1./2. column_stats -----------------------------------------------------


@pytest.mark.parametrize("n", GPU_ROW_COUNTS)
def test_column_stats_gpu_matches_cpu(dev, n):
    for layout, (cols, packed, schema) in _cached_blocks(n).items():
        want = column_stats(packed, schema)
        got = column_stats(packed.to(dev), schema)
        assert list(got) == list(want)
        for name in want:
            assert_stats_close(
                got[name], want[name].count.numpy(), want[name].mean.numpy(),
                want[name].std.numpy(), what=(n, layout, name))
        if layout == "mixed":
            assert got["const"].std.item() == 0.0
            assert got["const"].mean.item() == 3.25
            assert got["allnan"].count.item() == 0
            assert got["allnan"].mean.item() == 0.0


def test_column_stats_gpu_is_bitwise_reproducible(dev):
    # No float atomics: the same block gives the same bits on every call.
    for layout, (cols, packed, schema) in _cached_blocks(4099).items():
        block = packed.to(dev)
        a = column_stats(block, schema)
        b = column_stats(block, schema)
        for name in a:
            for x, y in zip(a[name], b[name]):
                assert_bits_equal(x, y, what=(layout, name))


# ----- 3. affine unpack -------------------------------------------------------

# layout -> (affine columns -> dst dtype); "lab" is never in affine.
_AFFINE_CASES = {
    "f64x100_bf16": ("wide_off0", {"w": torch.bfloat16}),
    "f64x100_f32": ("wide_off0", {"w": torch.float32}),
    "f32x8_aligned_bf16": ("wide_off0", {"v8": torch.bfloat16}),
    "key_f64x100_bf16_and_scalars": (
        "wide_off8",
        {
            "w": torch.bfloat16,  # offset 8: the misaligned case
            "key": torch.float32,  # i64x1 -> f32
            "d": torch.float32,  # f64x1 -> f32
            "v8": torch.bfloat16,  # f32x8 -> bf16
            "v3": torch.float32,  # f32x3 -> f32
            "j": torch.bfloat16,  # i32x1 -> bf16
        },
    ),
    "key_f64x100_f32": ("wide_off8", {"w": torch.float32}),
}


@pytest.mark.parametrize("nan_fill", [None, 0.5])
@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("case", sorted(_AFFINE_CASES))
def test_affine_unpack_gpu_bit_equal_to_cpu(dev, case, n, with_perm, nan_fill):
    layout, dst = _AFFINE_CASES[case]
    cols, packed, schema = _cached_blocks(n)[layout]
    stats = column_stats(packed, schema, columns=list(dst))
    affine = stats_to_affine(stats)
    perm = None
    if with_perm:
        g = torch.Generator().manual_seed(n)
        perm = torch.randperm(n, generator=g)[: n // 3 + 1]
    want = unpack_permute(
        packed, schema, perm=perm, out_dtypes=dst, affine=affine,
        nan_fill=nan_fill)
    block = packed.to(dev)
    perm_d = perm.to(dev) if perm is not None else None
    got = unpack_permute(
        block, schema, perm=perm_d, out_dtypes=dst, affine=affine,
        nan_fill=nan_fill)
    for name in want:
        assert got[name].is_cuda
        assert_bits_equal(got[name], want[name], what=(case, name))
    # Columns outside ``affine`` come out exactly as the plain kernel
    # gives them.
    plain = unpack_permute(block, schema, perm=perm_d)
    for name in schema.names:
        if name not in dst:
            assert_bits_equal(got[name], plain[name], what=(case, name))
    if nan_fill is not None:
        for name in dst:
            src = cols[name] if perm is None else cols[name][perm]
            if src.dtype.is_floating_point and torch.isnan(src).any():
                filled = got[name].cpu()[torch.isnan(src)].float()
                assert (filled == nan_fill).all(), (case, name)


def test_affine_none_launches_plain_kernel(dev):
    cols, packed, schema = _cached_blocks(257)["wide_off8"]
    block = packed.to(dev)
    dst = {"w": torch.bfloat16}
    a = unpack_permute(block, schema, out_dtypes=dst)
    b = unpack_permute(block, schema, out_dtypes=dst, affine=None,
                       nan_fill=None)
    for name in a:
        assert_bits_equal(a[name], b[name], what=name)


# ----- 4./5. the loader -------------------------------------------------------

_NUM_FEATS = 100
_LOADER_STATS = {}  # "local": the statistics of the non-collective run


@pytest.fixture(scope="module")
def loader_files(tmp_path_factory):
    """2 files x 3000 rows: key + 100 f64 features + label."""
    d = tmp_path_factory.mktemp("normalize_gpu")
    rng = np.random.default_rng(21)
    rows, names, feats, labels = 3000, [], [], []
    level = np.linspace(-1e6, 1e6, _NUM_FEATS)
    spread = np.logspace(-2, 3, _NUM_FEATS)
    for f in range(2):
        x = level + spread * rng.standard_normal((rows, _NUM_FEATS))
        lab = rng.random(rows)
        cols = {"key": np.arange(f * rows, (f + 1) * rows, dtype=np.int64)}
        cols.update({f"f{i}": x[:, i] for i in range(_NUM_FEATS)})
        cols["labels"] = lab
        path = str(d / f"part_{f}.parquet")
        pq.write_table(pa.table(cols), path)
        names.append(path)
        feats.append(x)
        labels.append(lab)
    return names, np.concatenate(feats), np.concatenate(labels)


def _run_loader(dev, filenames, num_epochs=2):
    """Epoch -> (keys, bf16 features, labels) through the engine with the
    fused feature matrix standardized in the kernel, plus the statistics."""
    from ray_shuffling_data_loader_amd.dataset import ShufflingDataset

    ds = ShufflingDataset(
        filenames, num_epochs, num_trainers=1, batch_size=1000, rank=0,
        num_reducers=2, device=dev, seed=13,
        feature_matrix=("__features__",
                        [f"f{i}" for i in range(_NUM_FEATS)]),
        out_dtypes={"__features__": torch.bfloat16},
        normalize=["__features__"],
    )
    epochs = {}
    for epoch in range(num_epochs):
        ds.set_epoch(epoch)
        batches = list(ds)
        epochs[epoch] = tuple(
            torch.cat([b[name] for b in batches]).cpu()
            for name in ("key", "__features__", "labels"))
    return epochs, ds.column_stats(timeout=60)


def _check_epochs(epochs, stats, feats, labels):
    n = feats.shape[0]
    st = stats["__features__"]
    assert st.count.tolist() == [n] * _NUM_FEATS
    mean, std = st.mean.numpy(), st.std.numpy()
    for epoch, (keys, y, lab) in epochs.items():
        assert sorted(keys.tolist()) == list(range(n)), epoch
        assert y.dtype == torch.bfloat16
        # fp64 reference rebuilt from key -> source row and the loader's
        # own statistics.
        ref = (feats[keys.numpy()] - mean) * (1.0 / std)
        err = np.abs(y.double().numpy() - ref)
        assert (err <= BF16_REL_BOUND * np.abs(ref)).all(), (
            epoch, float((err / np.abs(ref)).max()))
        assert lab.dtype == torch.float64
        assert torch.equal(lab, torch.from_numpy(labels)[keys]), epoch


def test_loader_standardizes_feature_matrix_on_gpu(dev, loader_files):
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    filenames, feats, labels = loader_files
    epochs, stats = _run_loader(dev, filenames)
    _check_epochs(epochs, stats, feats, labels)
    _LOADER_STATS["local"] = stats  # shared with the collective test
    # The statistics are the source data's.
    count = np.full(_NUM_FEATS, feats.shape[0])
    assert_stats_close(
        stats["__features__"], count, feats.mean(0), feats.std(0))

    # The public wrapper: feature_matrix=True, bf16, normalize_features.
    ds = TorchShufflingDataset(
        filenames, 1, 1, 1000, 0, num_reducers=2,
        feature_columns=[f"f{i}" for i in range(_NUM_FEATS)],
        feature_types=[torch.bfloat16] * _NUM_FEATS,
        label_column="labels", label_type=torch.float64,
        feature_matrix=True, normalize_features=True, device=dev, seed=13,
    )
    ds.set_epoch(0)
    xs, labs = zip(*[(d[0], lab) for d, lab in ds])
    x = torch.cat(xs).cpu()
    lab = torch.cat(labs).reshape(-1).cpu()
    assert x.dtype == torch.bfloat16 and x.shape == feats.shape
    fs = ds.feature_stats(timeout=60)
    assert list(fs) == ["__features__"]
    for a, b in zip(fs["__features__"], stats["__features__"]):
        assert torch.equal(a, b)
    # Same seed, same statistics: the wrapper's epoch 0 is the engine's.
    assert_bits_equal(x, epochs[0][1])
    assert torch.equal(lab, epochs[0][2])


def test_loader_standardizes_on_collective_path(dev, loader_files,
                                                monkeypatch):
    # The multi-GPU code path on one GPU: the statistics all-gather runs
    # over RCCL at world 1 and must give the local path's statistics.
    import torch.distributed as dist

    from ray_shuffling_data_loader_amd.parallel import fabric

    filenames, feats, labels = loader_files
    if "local" not in _LOADER_STATS:
        _LOADER_STATS["local"] = _run_loader(dev, filenames, num_epochs=1)[1]
    monkeypatch.setenv("RSDL_FORCE_COLLECTIVE", "1")
    dist.init_process_group(
        "nccl", init_method="tcp://127.0.0.1:29431", rank=0, world_size=1)
    try:
        epochs, stats = _run_loader(dev, filenames)
    finally:
        dist.destroy_process_group()
        fabric._shuffle_group = None
    _check_epochs(epochs, stats, feats, labels)
    # Count and mean cross the all-gather untouched; std travels as M2
    # (std^2 * n) and comes back through a square root.
    local = _LOADER_STATS["local"]["__features__"]
    assert torch.equal(stats["__features__"].count, local.count)
    assert torch.equal(stats["__features__"].mean, local.mean)
    assert_stats_close(
        stats["__features__"], local.count.numpy(), local.mean.numpy(),
        local.std.numpy())
