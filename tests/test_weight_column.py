"""``weight_column`` of TorchShufflingDataset on the CPU engine: a per-row
sample weight travels through the shuffle attached to its row, arrives as
the third member of every batch in fp32, and is neither standardized nor
part of the fused feature matrix."""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

CPU = torch.device("cpu")
N, C = 700, 6


def _weight_of(key):
    """The known function of the key column: multiples of 1/8 in [0, 4],
    exact in every float format on the way."""
    return (key % 33) / 8.0


def _write(tmp_path, num_files=2):
    rng = np.random.default_rng(13)
    paths = []
    per = N // num_files
    for f in range(num_files):
        key = np.arange(f * per, (f + 1) * per, dtype=np.int64)
        cols = {"key": key}
        feats = 1e3 * np.arange(1, C + 1) + rng.standard_normal((per, C))
        cols.update({f"f{i}": feats[:, i] for i in range(C)})
        # the label carries the key (exact in fp32) so a batch shows which
        # source row each of its rows is
        cols["labels"] = key.astype(np.float64)
        cols["w"] = _weight_of(key).astype(np.float64)
        path = str(tmp_path / f"part{f}.parquet")
        pq.write_table(pa.table(cols), path)
        paths.append(path)
    return paths


def _dataset(paths, num_epochs=2, **kw):
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    return TorchShufflingDataset(
        paths, num_epochs, 1, 256, 0, num_reducers=2,
        feature_columns=[f"f{i}" for i in range(C)],
        feature_types=[torch.bfloat16] * C, label_column="labels",
        feature_matrix=True, normalize_features=True, device=CPU, seed=1,
        **kw,
    )


def test_weight_column_rides_with_its_row(tmp_path):
    paths = _write(tmp_path)
    ds = _dataset(paths, weight_column="w")
    orders = []
    for epoch in range(2):
        ds.set_epoch(epoch)
        keys = []
        for batch in ds:
            assert isinstance(batch, tuple) and len(batch) == 3
            data, label, weight = batch
            b = label.shape[0]
            assert data[0].shape == (b, C)
            assert data[0].dtype == torch.bfloat16
            assert label.shape == (b, 1)
            # fp32 out of the unpack (the source column is fp64), [B]
            assert weight.dtype == torch.float32 and weight.shape == (b,)
            k = label.reshape(-1).long()
            # attached to its row, and raw: not standardized
            assert torch.equal(weight, _weight_of(k).float())
            keys.append(k)
        keys = torch.cat(keys)
        assert sorted(keys.tolist()) == list(range(N))
        orders.append(keys)
    # it was a shuffle, and a different one per epoch
    assert not torch.equal(orders[0], torch.arange(N))
    assert not torch.equal(orders[0], orders[1])
    # the statistics are the feature matrix's alone
    st = ds.feature_stats(timeout=60)
    assert list(st) == ["__features__"]
    assert st["__features__"].mean.numel() == C
    assert (st["__features__"].mean > 500).all()


def test_weight_column_without_feature_matrix(tmp_path):
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    paths = _write(tmp_path, num_files=1)
    ds = TorchShufflingDataset(
        paths, 1, 1, 256, 0, num_reducers=2,
        feature_columns=["f0", "f1"], label_column="labels",
        normalize_features=True, weight_column="w", device=CPU, seed=2,
    )
    ds.set_epoch(0)
    seen = 0
    for data, label, weight in ds:
        assert len(data) == 2 and weight.dtype == torch.float32
        k = label.reshape(-1).long()
        assert torch.equal(weight, _weight_of(k).float())
        seen += k.numel()
    assert seen == N
    assert sorted(ds.feature_stats(timeout=60)) == ["f0", "f1"]


def test_weight_type_is_honoured(tmp_path):
    paths = _write(tmp_path, num_files=1)
    ds = _dataset(paths, num_epochs=1, weight_column="w",
                  weight_type=torch.float64)
    ds.set_epoch(0)
    for _, label, weight in ds:
        assert weight.dtype == torch.float64
        assert torch.equal(weight, _weight_of(label.reshape(-1).long()))


def test_weight_column_among_features_raises(tmp_path):
    paths = _write(tmp_path, num_files=1)
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    with pytest.raises(ValueError, match="also listed in feature_columns"):
        TorchShufflingDataset(
            paths, 1, 1, 256, 0, num_reducers=2,
            feature_columns=["f0", "w"], label_column="labels",
            weight_column="w", device=CPU, seed=1,
        )


def test_without_weight_column_batches_are_pairs(tmp_path):
    paths = _write(tmp_path, num_files=1)
    ds = _dataset(paths, num_epochs=1)
    ds.set_epoch(0)
    n = 0
    for batch in ds:
        assert isinstance(batch, tuple) and len(batch) == 2
        data, label = batch
        assert data[0].shape[1] == C
        n += label.shape[0]
    assert n == N


def test_convert_to_tensor_factory_carries_the_weight():
    import pandas as pd

    from ray_shuffling_data_loader_amd.torch_dataset import (
        rowblock_to_tensor_factory,
    )

    df = pd.DataFrame({"a": [1.0, 2.0, 3.0], "y": [0.0, 1.0, 0.0],
                       "w": [0.5, 0.0, 2.0]})
    conv = rowblock_to_tensor_factory(
        feature_columns=["a"], label_column="y", weight_column="w")
    feats, label, weight = conv(df)
    assert feats[0].shape == (3, 1) and label.shape == (3, 1)
    assert weight.dtype == torch.float32
    assert weight.tolist() == [0.5, 0.0, 2.0]
    assert len(rowblock_to_tensor_factory(
        feature_columns=["a"], label_column="y")(df)) == 2
