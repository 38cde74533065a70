"""In-kernel feature standardization, CPU paths: the column_stats fit, the
Chan merge, the affine unpack oracle, and the engine / dataset plumbing
(normalize=, nan_fill=, normalize_features=, column_stats()).

The CPU implementations are the oracles the GPU kernels are held to in
tests/test_normalize_gpu.py. Statistics tolerances are derived in
tests/_normalize_cases.py.
"""

import os
import tempfile

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
    numpy_stats,
    pack,
)
from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
    ColumnStats,
    column_stats,
    merge_column_stats,
    stats_to_affine,
    unpack_permute,
)

CPU = torch.device("cpu")


# ----- 1. column_stats vs numpy ----------------------------------------------


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_column_stats_matches_numpy(n):
    cols = mixed_columns(n)
    packed, schema = pack(cols)
    stats = column_stats(packed, schema)
    assert set(stats) == set(cols)
    for name, col in cols.items():
        count, mean, std = numpy_stats(col)
        assert_stats_close(stats[name], count, mean, std, what=(n, name))
        numel = 1 if col.dim() == 1 else col.shape[1]
        assert stats[name].mean.shape == (numel,)
    # Exact cases: a constant column and an all-NaN column.
    assert stats["const"].std.item() == 0.0
    assert stats["const"].mean.item() == 3.25
    assert stats["allnan"].count.item() == 0
    assert stats["allnan"].mean.item() == 0.0
    assert stats["allnan"].std.item() == 0.0
    assert stats["k"].count.item() == n  # integers are always finite


def test_column_stats_column_subset_and_empty_block():
    packed, schema = pack(mixed_columns(65))
    sub = column_stats(packed, schema, columns=["v", "big"])
    assert list(sub) == ["v", "big"]
    full = column_stats(packed, schema)
    for name in sub:
        for a, b in zip(sub[name], full[name]):
            assert torch.equal(a, b)
    empty = column_stats(packed[:0], schema, columns=["v"])
    assert empty["v"].count.tolist() == [0, 0, 0, 0]
    assert empty["v"].std.tolist() == [0.0] * 4


# ----- 2. merge ---------------------------------------------------------------


def test_merge_column_stats_uneven_shards():
    n = 4099
    cols = mixed_columns(n, seed=3)
    packed, schema = pack(cols)
    shards = [packed[:37], packed[37:37], packed[37:]]  # one empty
    merged = merge_column_stats([column_stats(s, schema) for s in shards])
    for name, col in cols.items():
        count, mean, std = numpy_stats(col)
        assert_stats_close(merged[name], count, mean, std, what=name)
    assert merged["const"].std.item() == 0.0
    assert merged["allnan"].count.item() == 0
    # Merging is a pure function of the list: same list, same bits.
    again = merge_column_stats([column_stats(s, schema) for s in shards])
    for name in merged:
        for a, b in zip(merged[name], again[name]):
            assert torch.equal(a, b)


# ----- 3. the plain path does not move ---------------------------------------


@pytest.mark.parametrize("with_perm", [False, True])
def test_unpack_affine_none_is_plain(with_perm):
    n = 257
    packed, schema = pack(mixed_columns(n))
    perm = torch.randperm(n)[: n // 3 + 1] if with_perm else None
    out_dtypes = {"d": torch.bfloat16, "v": torch.bfloat16}
    plain = unpack_permute(packed, schema, perm=perm, out_dtypes=out_dtypes)
    kw = unpack_permute(
        packed, schema, perm=perm, out_dtypes=out_dtypes, affine=None,
        nan_fill=None,
    )
    for name in plain:
        assert_bits_equal(plain[name], kw[name], what=name)


def test_unpack_affine_formula_and_untouched_columns():
    n = 4099
    cols = mixed_columns(n, seed=5)
    packed, schema = pack(cols)
    stats = column_stats(packed, schema)
    affine = stats_to_affine({k: stats[k] for k in ("d", "v", "k", "big")})
    perm = torch.randperm(n)[:1000]
    out_dtypes = {"d": torch.bfloat16, "k": torch.float32,
                  "big": torch.bfloat16}
    plain = unpack_permute(packed, schema, perm=perm, out_dtypes=out_dtypes)
    got = unpack_permute(
        packed, schema, perm=perm, out_dtypes=out_dtypes, affine=affine,
        nan_fill=0.5,
    )
    for name in ("s", "j", "const", "allnan"):  # not in affine
        assert_bits_equal(plain[name], got[name], what=name)
    for name in affine:
        shift, scale = affine[name]
        x = cols[name][perm].double()
        want = ((x - shift) * scale).float()
        want = torch.where(torch.isnan(x), torch.tensor(0.5), want)
        want = want.to(out_dtypes.get(name, cols[name].dtype))
        assert_bits_equal(got[name], want, what=name)
    # scale follows the StandardScaler convention.
    const = stats_to_affine({"const": stats["const"],
                             "allnan": stats["allnan"]})
    assert const["const"][1].item() == 1.0
    assert const["allnan"][1].item() == 1.0
    # Without nan_fill a NaN stays a NaN.
    keep = unpack_permute(packed, schema, affine={"d": affine["d"]})
    assert torch.equal(torch.isnan(keep["d"]), torch.isnan(cols["d"]))
    # The 1e9 column survives the bf16 cast only because it was centred
    # first: many distinct values instead of one.
    assert plain["big"][torch.isfinite(plain["big"])].unique().numel() == 1
    assert got["big"][torch.isfinite(got["big"])].unique().numel() > 50


# ----- engine / dataset -------------------------------------------------------


def _write_files(dirname, num_files=4, rows=500, seed=11, file_shift=0.0):
    """key, an offset float column, an int column and a label. With
    ``file_shift`` each file's float column sits at a different level, so a
    shard's statistics differ from the global ones."""
    rng = np.random.default_rng(seed)
    names, tables = [], []
    for f in range(num_files):
        cols = {
            "key": np.arange(f * rows, (f + 1) * rows, dtype=np.int64),
            "off": 1e6 + f * file_shift + 25.0 * rng.standard_normal(rows),
            "cnt": rng.integers(0, 1000, rows, dtype=np.int64),
            "label": rng.random(rows),
        }
        path = os.path.join(dirname, f"part_{f}.parquet")
        pq.write_table(pa.table(cols), path)
        names.append(path)
        tables.append(cols)
    whole = {k: np.concatenate([t[k] for t in tables]) for k in tables[0]}
    return names, whole


def _run_epochs(filenames, num_epochs=2, start_epoch=0, **kw):
    from ray_shuffling_data_loader_amd.dataset import ShufflingDataset

    ds = ShufflingDataset(
        filenames, num_epochs, num_trainers=1, batch_size=300, rank=0,
        num_reducers=2, device=CPU, seed=kw.pop("seed", 7),
        start_epoch=start_epoch, **kw,
    )
    epochs, stats = {}, {}
    for epoch in range(start_epoch, num_epochs):
        ds.set_epoch(epoch)
        batches = list(ds)
        epochs[epoch] = {
            name: torch.cat([b[name] for b in batches])
            for name in batches[0].columns
        }
        if kw.get("normalize") is not None:
            stats[epoch] = ds.column_stats(timeout=60)
    return epochs, stats


def test_engine_standardizes_end_to_end(tmp_path):
    filenames, whole = _write_files(str(tmp_path))
    n = len(whole["key"])
    epochs, stats = _run_epochs(filenames, normalize=["off", "cnt"])
    for epoch, cols in epochs.items():
        keys = cols["key"]
        assert sorted(keys.tolist()) == list(range(n)), epoch
        # Labels (and keys) are not standardized: bit-equal to the source.
        assert cols["label"].dtype == torch.float64
        assert torch.equal(
            cols["label"], torch.from_numpy(whole["label"])[keys])
        for name in ("off", "cnt"):
            y = cols[name]
            # a standardized integer column comes out as float32
            assert y.dtype == (
                torch.float64 if name == "off" else torch.float32)
            y = y.float().double()
            # fp32 outputs: 2000 values each rounded at 2^-24 cannot move
            # either moment by more than about 1e-6.
            assert abs(y.mean().item()) <= 1e-5, (epoch, name)
            assert abs(y.std(unbiased=False).item() - 1.0) <= 1e-5, (
                epoch, name)
    for name in ("off", "cnt"):
        count, mean, std = numpy_stats(torch.from_numpy(whole[name]))
        assert_stats_close(stats[0][name], count, mean, std, what=name)
    # Frozen: identical across epochs.
    for name in stats[0]:
        for a, b in zip(stats[0][name], stats[1][name]):
            assert torch.equal(a, b)
    # Different epochs are different shuffles of the same values.
    assert not torch.equal(epochs[0]["key"], epochs[1]["key"])

    # Same seed, independent run: bit-identical batches and statistics.
    epochs2, stats2 = _run_epochs(filenames, normalize=["off", "cnt"])
    for epoch in epochs:
        for name in epochs[epoch]:
            assert_bits_equal(
                epochs[epoch][name], epochs2[epoch][name], what=(epoch, name))
    for name in stats[0]:
        for a, b in zip(stats[0][name], stats2[0][name]):
            assert torch.equal(a, b)
    # A resumed run (start_epoch=1) rebuilds epoch 1 bit for bit.
    resumed, _ = _run_epochs(
        filenames, start_epoch=1, normalize=["off", "cnt"])
    for name in epochs[1]:
        assert_bits_equal(epochs[1][name], resumed[1][name], what=name)


def test_engine_standard_fits_every_numeric_column(tmp_path):
    filenames, whole = _write_files(str(tmp_path), num_files=2, rows=200)
    epochs, stats = _run_epochs(
        filenames, num_epochs=1, normalize="standard", source_cache="none")
    assert set(stats[0]) == {"key", "off", "cnt", "label"}
    for name, y in epochs[0].items():
        y = y.double()
        assert abs(y.mean().item()) <= 1e-5, name
        assert abs(y.std(unbiased=False).item() - 1.0) <= 1e-5, name


def test_engine_default_is_unchanged(tmp_path):
    # normalize=None: nothing changes anywhere, and there are no statistics.
    from ray_shuffling_data_loader_amd.dataset import ShufflingDataset

    filenames, whole = _write_files(str(tmp_path), num_files=2, rows=200)
    epochs, _ = _run_epochs(filenames, num_epochs=1)
    keys = epochs[0]["key"]
    assert torch.equal(epochs[0]["off"], torch.from_numpy(whole["off"])[keys])
    assert epochs[0]["cnt"].dtype == torch.int64
    ds = ShufflingDataset(filenames, 1, 1, 300, 0, num_reducers=2,
                          device=CPU, seed=7)
    with pytest.raises(RuntimeError, match="normalize"):
        ds.column_stats(timeout=10)
    ds.set_epoch(0)
    list(ds)


# ----- 4. precomputed statistics ---------------------------------------------


def test_engine_precomputed_stats_applied_as_given(tmp_path):
    filenames, whole = _write_files(str(tmp_path), num_files=2, rows=200)
    mean, std = 999_990.0, 12.5
    epochs, stats = _run_epochs(
        filenames, num_epochs=1,
        normalize={"off": (mean, std), "cnt": (0.0, 0.0)},
        out_dtypes={"off": torch.float32},
    )
    keys = epochs[0]["key"]
    x = torch.from_numpy(whole["off"])[keys]
    want = ((x - mean) * (1.0 / std)).float()
    assert_bits_equal(epochs[0]["off"], want)
    # std == 0 -> scale 1 (StandardScaler convention); int -> float32.
    want_cnt = torch.from_numpy(whole["cnt"])[keys].double().float()
    assert_bits_equal(epochs[0]["cnt"], want_cnt)
    # Reported exactly as given; no fit happened (count -1).
    assert stats[0]["off"].mean.item() == mean
    assert stats[0]["off"].std.item() == std
    assert stats[0]["off"].count.item() == -1


def test_engine_normalize_argument_errors(tmp_path):
    from ray_shuffling_data_loader_amd.engine import ShuffleEngine

    filenames, _ = _write_files(str(tmp_path), num_files=1, rows=10)
    common = dict(consumer=None, num_epochs=1, num_reducers=1,
                  num_trainers=1, device=CPU)
    with pytest.raises(ValueError, match="not a column"):
        ShuffleEngine(filenames, normalize=["nope"], **common)
    with pytest.raises(ValueError, match="standard"):
        ShuffleEngine(filenames, normalize="minmax", **common)
    with pytest.raises(ValueError, match="nan_fill"):
        ShuffleEngine(filenames, nan_fill=0.0, **common)


def test_column_stats_raises_when_engine_failed(tmp_path):
    # A failed engine must not block column_stats() forever.
    from ray_shuffling_data_loader_amd.dataset import ShufflingDataset
    from ray_shuffling_data_loader_amd.utils.schema import (
        ColumnSpec,
        Schema,
    )

    ds = ShufflingDataset(
        [str(tmp_path / "missing.parquet")], 1, 1, 10, 0, num_reducers=1,
        device=CPU, normalize=["x"],
        schema=Schema([ColumnSpec("x", torch.float64)]),
    )
    with pytest.raises(RuntimeError, match="failed"):
        ds.column_stats(timeout=60)


def test_column_stats_needs_an_engine():
    # A worker that only connects to rank 0's queue has no engine.
    from ray_shuffling_data_loader_amd.dataset import ShufflingDataset

    ds = object.__new__(ShufflingDataset)
    ds._engine = None
    with pytest.raises(RuntimeError, match="only available in the process"):
        ds.column_stats()


# ----- 6. the bf16 case -------------------------------------------------------


def _bf16_features(filenames, n, **kw):
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    ds = TorchShufflingDataset(
        filenames, 1, 1, 1024, 0, num_reducers=2,
        feature_columns=["x"], feature_types=[torch.bfloat16],
        label_column="row", device=CPU, seed=3, **kw,
    )
    ds.set_epoch(0)
    feats, rows = [], []
    for data, label in ds:
        assert data[0].dtype == torch.bfloat16
        feats.append(data[0].reshape(-1))
        rows.append(label.reshape(-1).long())
    feats, rows = torch.cat(feats), torch.cat(rows)
    assert sorted(rows.tolist()) == list(range(n))
    return ds, feats, rows


def test_bf16_features_survive_only_when_standardized(tmp_path):
    n = 4099
    rng = np.random.default_rng(5)
    x = 1e6 + rng.standard_normal(n)
    path = str(tmp_path / "x.parquet")
    # The label is the source row number (exact in float32).
    pq.write_table(
        pa.table({"x": x, "row": np.arange(n, dtype=np.float64)}), path)

    ds, feats, rows = _bf16_features([path], n, normalize_features=True)
    st = ds.feature_stats(timeout=60)
    assert list(st) == ["x"]  # never the label
    mean, std = st["x"].mean.item(), st["x"].std.item()
    ref = (x[rows.numpy()] - mean) * (1.0 / std)  # fp64
    err = np.abs(feats.double().numpy() - ref)
    assert (err <= BF16_REL_BOUND * np.abs(ref)).all(), float(
        (err / np.abs(ref)).max())
    assert np.corrcoef(feats.double().numpy(), ref)[0, 1] > 0.9999

    # The contrast: the same column through the same loader without
    # standardization collapses to ONE bf16 value.
    _, raw, _ = _bf16_features([path], n)
    assert raw.unique().numel() == 1


def test_normalize_features_with_feature_matrix(tmp_path):
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    n, c = 600, 8
    rng = np.random.default_rng(9)
    feats = 1e5 * np.arange(1, c + 1) + rng.standard_normal((n, c))
    cols = {"key": np.arange(n, dtype=np.int64)}
    cols.update({f"f{i}": feats[:, i] for i in range(c)})
    cols["labels"] = np.arange(n, dtype=np.float64)
    path = str(tmp_path / "m.parquet")
    pq.write_table(pa.table(cols), path)
    ds = TorchShufflingDataset(
        [path], 1, 1, 256, 0, num_reducers=2,
        feature_columns=[f"f{i}" for i in range(c)],
        feature_types=[torch.bfloat16] * c, label_column="labels",
        feature_matrix=True, normalize_features=True, device=CPU, seed=1,
    )
    ds.set_epoch(0)
    got, rows = [], []
    for data, label in ds:
        assert data[0].dtype == torch.bfloat16 and data[0].shape[1] == c
        got.append(data[0])
        rows.append(label.reshape(-1).long())
    got, rows = torch.cat(got).double().numpy(), torch.cat(rows).numpy()
    st = ds.feature_stats(timeout=60)
    assert list(st) == ["__features__"]
    mean, std = st["__features__"].mean.numpy(), st["__features__"].std.numpy()
    ref = (feats[rows] - mean) * (1.0 / std)
    assert (np.abs(got - ref) <= BF16_REL_BOUND * np.abs(ref)).all()


# ----- 7. gloo world 2 --------------------------------------------------------


def _stats_rank(rank, world, init_method, filenames, result_q):
    try:
        import torch.distributed as dist

        dist.init_process_group(
            "gloo", init_method=init_method, rank=rank, world_size=world
        )
        from ray_shuffling_data_loader_amd.dataset import ShufflingDataset

        ds = ShufflingDataset(
            filenames, 1, num_trainers=world, batch_size=500, rank=rank,
            num_reducers=2, seed=42, normalize=["off", "cnt"],
        )
        ds.set_epoch(0)
        batches = list(ds)
        st = ds.column_stats(timeout=120)
        out = {
            "stats": {k: tuple(t.tolist() for t in v) for k, v in st.items()},
            "keys": torch.cat([b["key"] for b in batches]).tolist(),
            "off": torch.cat([b["off"] for b in batches]).tolist(),
        }
        result_q.put((rank, out))
        dist.destroy_process_group()
    except Exception as e:  # surface to the parent
        import traceback

        result_q.put((rank, f"ERROR: {e}\n{traceback.format_exc()}"))


def test_distributed_stats_are_global(tmp_path, mp_spawn_context):
    # Each file sits at its own level, and rank r maps files r, r+2: a
    # shard's mean is ~1000 away from the global one.
    filenames, whole = _write_files(str(tmp_path), file_shift=1000.0)
    world = 2
    port_file = tempfile.NamedTemporaryFile(delete=False)
    init_method = f"file://{port_file.name}"
    os.unlink(port_file.name)
    ctx = mp_spawn_context
    result_q = ctx.Queue()
    procs = [
        ctx.Process(
            target=_stats_rank,
            args=(r, world, init_method, filenames, result_q),
        )
        for r in range(world)
    ]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, out = result_q.get(timeout=180)
        assert not isinstance(out, str), out
        results[rank] = out
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # Both ranks hold the same statistics, bit for bit ...
    assert results[0]["stats"] == results[1]["stats"]
    # ... and they are the global dataset's, not the shard's.
    for name in ("off", "cnt"):
        count, mean, std = numpy_stats(torch.from_numpy(whole[name]))
        c, m, s = results[0]["stats"][name]
        got = ColumnStats(
            torch.tensor(c), torch.tensor(m, dtype=torch.float64),
            torch.tensor(s, dtype=torch.float64))
        assert_stats_close(got, count, mean, std, what=name)
    keys = results[0]["keys"] + results[1]["keys"]
    assert sorted(keys) == list(range(len(whole["key"])))
    y = np.array(results[0]["off"] + results[1]["off"])
    assert abs(y.mean()) <= 1e-5 and abs(y.std() - 1.0) <= 1e-5
