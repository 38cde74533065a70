"""GPU tests of the forward-only evaluation path: eval_chain_kernel
(csrc/fwd_chain.hip), eval_accumulate (csrc/step_glue.hip), their
bindings and models/fused_eval.py.

The eval chain runs the training forward's three MFMA layers and head
without the emissions, so its head value must be the training kernel's
bit for bit: the bf16 rounding of ``pred`` equals ``out`` and column 0 of
the partials equals ``loss_part`` of ``fwd_chain_bf16`` (same build, same
target, same ``rows``; that kernel is the parent's, unchanged). A second
test compares against the eager fp32 reference and leans on no sibling
kernel.

Shapes: the smallest that cover a partial first m-tile, a partial second
m-tile, an odd tile count whose last 64-row workgroup has no second
m-tile, and a single row, at both slab sizes.

Bound for regrouped reductions (columns 1-3 of the partials, the
evaluator's metrics): the project's figure 1e-5 * max|ref| + 1e-5
(profiles/PERF.md round 3, as in tests/test_chain_rows64_gpu.py). The
terms are fp32 values summed in fp32 over at most 64 rows and then in
fp64, off from an fp64 sum by about 64 * 2^-24 relative at worst.
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [1, 31, 32, 33, 64, 65, 96, 97, 161]
ROWS = (32, 64)
M_MAX = max(SHAPES)
BATCHES = [64, 33, 1, 161]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    return shuffle_ops._load_hip()


@pytest.fixture(scope="module")
def data(dev, hip):
    """Seeded bf16-exact weights (fp32 masters for step_prep, the same
    values in bf16 for fwd_chain_bf16), fp32 biases, and the largest
    batch; smaller shapes take its leading rows."""
    g = torch.Generator(device="cpu").manual_seed(64)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    Wb = [
        (rn(512, 100) / 10).bfloat16(),
        (rn(256, 512) / 22).bfloat16(),
        (rn(128, 256) / 16).bfloat16(),
        (rn(1, 128) / 11).bfloat16(),
    ]
    bs = [(rn(n) / 4).bfloat16().float() for n in (512, 256, 128, 1)]
    st = hip.step_prep([w.float() for w in Wb])
    return {
        "Wb": Wb,
        "bs": bs,
        "stage": [st[0], st[1], st[2], st[5]],
        "x": rn(M_MAX, 100).bfloat16(),
        "tgt": rn(M_MAX),
    }


@pytest.fixture(scope="module")
def run(hip, data):
    """(M, rows) -> dict(pred, part, out, loss_part): the eval chain and
    the training forward on the same inputs, computed once per key."""
    cache = {}

    def get(M, rows):
        if (M, rows) not in cache:
            Wb, bs = data["Wb"], data["bs"]
            x = data["x"][:M].contiguous()
            tgt = data["tgt"][:M].contiguous()
            f = hip.fwd_chain_bf16(
                x, Wb[0], bs[0], Wb[1], bs[1], Wb[2], bs[2],
                Wb[3].flatten(), bs[3], target=tgt, rows=rows,
            )
            pred, part = hip.eval_chain_bf16(
                x, data["stage"], bs, target=tgt, rows=rows)
            cache[(M, rows)] = {
                "pred": pred, "part": part, "out": f[5], "loss_part": f[7],
            }
        return cache[(M, rows)]

    return get


def _bound(ref):
    return 1e-5 * ref.abs().max().item() + 1e-5


def _metrics(pred, tgt):
    p = pred.reshape(-1).double()
    t = tgt.reshape(-1).float().double()
    n = t.numel()
    sse = ((p - t) ** 2).sum().item()
    return {
        "rows": n,
        "mse": sse / n,
        "mae": (p - t).abs().sum().item() / n,
        "r2": 1.0 - sse / ((t * t).sum().item() - t.sum().item() ** 2 / n),
    }


def _check_metrics(got, want):
    assert got["rows"] == want["rows"]
    for k in ("mse", "mae", "r2"):
        bound = 1e-5 * abs(want[k]) + 1e-5
        print(f"{k}: got {got[k]!r} want {want[k]!r} bound {bound:.3e}")
        assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k])
    assert got["rmse"] == math.sqrt(got["mse"])


# 1. eval chain against the training forward
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", SHAPES)
def test_eval_chain_matches_training_forward(run, data, M, rows):
    r = run(M, rows)
    pred, part = r["pred"], r["part"]
    assert pred.dtype == torch.float32 and pred.shape == (M,)
    assert torch.equal(pred.bfloat16(), r["out"].flatten())
    nwg = (M + rows - 1) // rows
    assert part.shape == (nwg, 4) and part.dtype == torch.float32
    assert torch.equal(part[:, 0], r["loss_part"])
    # columns 1-3: fp64 sums per workgroup, rebuilt from pred and the
    # fp32 target
    p = pred.double()
    t = data["tgt"][:M].double()
    pad = nwg * rows - M
    terms = torch.stack([(p - t).abs(), t, t * t], 1)
    terms = torch.nn.functional.pad(terms, (0, 0, 0, pad))
    ref = terms.view(nwg, rows, 3).sum(1)
    for c, name in enumerate(["sae", "sum_t", "sum_tt"]):
        err = (part[:, 1 + c].double() - ref[:, c]).abs().max().item()
        b = _bound(ref[:, c])
        print(f"M={M} rows={rows} {name}: err {err:.3e} bound {b:.3e}")
        assert err <= b, (name, M, rows, err, b)


# 2. nothing is written past M
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", SHAPES)
def test_eval_chain_writes_nothing_past_m(hip, run, data, dev, M, rows):
    r = run(M, rows)
    canary = -12345.5
    big = torch.full((8 + M + 8,), canary, dtype=torch.float32, device=dev)
    x = data["x"][:M].contiguous()
    tgt = data["tgt"][:M].contiguous()
    pred, part = hip.eval_chain_bf16(
        x, data["stage"], data["bs"], target=tgt, pred_out=big[8:8 + M],
        rows=rows)
    assert pred.data_ptr() == big[8:8 + M].data_ptr()
    assert torch.equal(big[8:8 + M], r["pred"])
    assert bool((big[:8] == canary).all()) and bool(
        (big[8 + M:] == canary).all())
    assert torch.equal(part, r["part"])
    none, part2 = hip.eval_chain_bf16(
        x, data["stage"], data["bs"], target=tgt, want_pred=False,
        rows=rows)
    assert none is None
    assert torch.equal(part2, r["part"])
    pred3, none3 = hip.eval_chain_bf16(
        x, data["stage"], data["bs"], rows=rows)
    assert none3 is None and torch.equal(pred3, r["pred"])


# 3. eval chain against the eager fp32 reference
@pytest.mark.parametrize("rows", ROWS)
def test_eval_chain_matches_eager_fp32(run, data, rows):
    M = M_MAX
    r = data["x"][:M].float()
    for i, (W, b) in enumerate(zip(data["Wb"], data["bs"])):
        r = r @ W.float().t() + b
        if i < 3:
            r = torch.relu(r)
    ref_b = r.flatten().bfloat16().float()
    err = (run(M, rows)["pred"] - ref_b).abs()
    scale = ref_b.abs().mean().clamp(min=1.0)
    print(f"rows={rows}: max err {err.max().item():.3e} "
          f"bound {(0.12 * scale + 0.05).item():.3e}")
    assert err.max() <= 0.12 * scale + 0.05, (err.max().item(), scale.item())


# 4. eval_accumulate
@pytest.mark.parametrize("n", [1, 7, 256, 257, 1000])
def test_eval_accumulate_fixed_order_fp64(hip, dev, n):
    """Hand-made partials (one row, fewer and more rows than the
    workgroup's 256 threads) onto a nonzero accumulator, against the
    exact sum of the same numbers (math.fsum), within 4 ulp of fp64, and
    bit-identical on a second run."""
    g = torch.Generator(device="cpu").manual_seed(n)
    part = torch.rand(n, 4, generator=g) * 100.0
    part[:, 2] -= 25.0  # a signed column (sum t)
    acc0 = torch.tensor([12345.0, 3.25, 1e3 + 1e-9, 0.5, 7.0],
                        dtype=torch.float64)
    M = 64 * n - 3
    accs = []
    for _ in range(2):
        acc = acc0.to(dev)
        hip.eval_accumulate(part.to(dev), acc, M)
        accs.append(acc.cpu())
    assert torch.equal(accs[0], accs[1])
    got = accs[0].tolist()
    assert got[0] == 12345.0 + M
    for c in range(4):
        ref = math.fsum([acc0[1 + c].item()] + part[:, c].double().tolist())
        ulps = abs(got[1 + c] - ref) / np.spacing(abs(ref))
        print(f"n={n} col {c}: {ulps:.2f} ulp")
        assert ulps <= 4, (n, c, got[1 + c], ref)


def _model(dev, seed=7):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    return TabularMLP(100).to(dev)


def _batches(dev, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = sum(BATCHES)
    x = torch.randn(n, 100, generator=g).bfloat16().to(dev)
    t = torch.randn(n, 1, generator=g).to(dev)
    return x, t


# 5. FusedEvaluator over unequal batches
@pytest.mark.parametrize("rows", (0,) + ROWS)
def test_evaluator_over_batches(dev, rows):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    model = _model(dev)
    x, t = _batches(dev)
    ev = fe.FusedEvaluator(model, rows=rows)
    states = []
    for _ in range(2):
        ev.reset()
        off = 0
        for b in BATCHES:
            ev.update(x[off:off + b], t[off:off + b])
            off += b
        before = ev.state()
        ev.update(x[:0], t[:0])  # empty batch: no-op
        assert torch.equal(ev.state(), before)
        states.append(ev.state())
    assert torch.equal(states[0], states[1])
    got = ev.compute()
    pred = fe.fused_predict(model, x)
    assert pred.shape == (x.shape[0], 1) and pred.dtype == torch.float32
    _check_metrics(got, _metrics(pred, t))
    assert got["rows"] == sum(BATCHES)
    ev.reset()
    assert torch.equal(ev.state().cpu(),
                       torch.zeros(5, dtype=torch.float64))
    assert math.isnan(ev.compute()["mse"])
    # fp64 targets are cast to fp32 ahead of the kernel: same bits
    ev.update(x[:97], t[:97].double())
    a = ev.state()
    ev.reset()
    ev.update(x[:97], t[:97])
    assert torch.equal(a, ev.state())


# 6. consistency with training
def test_evaluator_agrees_with_fused_step_loss(dev):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step

    model = _model(dev)
    x, t = _batches(dev)
    x, t = x[:161].contiguous(), t[:161].contiguous()
    loss = fused_step(model, x, t).item()
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.train()
    ev = fe.FusedEvaluator(model)
    ev.update(x, t)
    mse = ev.compute()["mse"]
    print(f"fused_step loss {loss!r}  evaluator mse {mse!r}")
    # the same fp32 terms, summed in another order
    assert abs(loss - mse) <= 1e-5 * abs(loss)
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), params[n]), n
        assert torch.equal(p.grad, grads[n]), n


# 7. the weight stage follows the parameters
def test_evaluator_restages_after_weight_update(dev, hip, monkeypatch):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    model = _model(dev)
    x, _ = _batches(dev)
    x = x[:97].contiguous()
    ev = fe.FusedEvaluator(model)
    calls = []
    real = hip.step_prep

    class Counting:
        def __getattr__(self, name):
            return getattr(hip, name)

        @staticmethod
        def step_prep(*a, **k):
            calls.append(1)
            return real(*a, **k)

    monkeypatch.setattr(ev, "_hip", lambda: Counting())
    first = ev.predict(x).clone()
    assert torch.equal(ev.predict(x), first)
    assert len(calls) == 1  # staged once, reused
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)
    second = ev.predict(x)
    assert len(calls) == 2  # one re-stage, unprompted
    assert torch.equal(second, fe.FusedEvaluator(model).predict(x))
    assert not torch.equal(first, second)
    # an optimizer step is seen too
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    third = ev.predict(x)
    assert len(calls) == 3
    assert torch.equal(third, fe.FusedEvaluator(model).predict(x))
    assert not torch.equal(second, third)


def test_eval_bindings_validate_arguments(hip, data, dev):
    x = data["x"][:8].contiguous()
    st, bs = data["stage"], data["bs"]
    with pytest.raises(RuntimeError, match="32 or 64"):
        hip.eval_chain_bf16(x, st, bs, rows=48)
    with pytest.raises(RuntimeError, match="x must be contiguous bf16"):
        hip.eval_chain_bf16(x.float(), st, bs)
    with pytest.raises(RuntimeError, match="staged weight 0"):
        hip.eval_chain_bf16(x, [st[1], st[1], st[2], st[3]], bs)
    with pytest.raises(RuntimeError, match="target size mismatch"):
        hip.eval_chain_bf16(x, st, bs, target=data["tgt"][:7].contiguous())
    with pytest.raises(RuntimeError, match="pred_out"):
        hip.eval_chain_bf16(
            x, st, bs, pred_out=torch.empty(9, device=dev))
    with pytest.raises(RuntimeError, match="nothing to compute"):
        hip.eval_chain_bf16(x, st, bs, want_pred=False)
    pred, part = hip.eval_chain_bf16(
        x[:0], st, bs, target=data["tgt"][:0].contiguous())
    assert pred.numel() == 0
    assert torch.equal(part.cpu(), torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match=r"acc must be contiguous fp64"):
        hip.eval_accumulate(part, torch.zeros(5, device=dev), 0)


# 8. end to end with the loader
def test_evaluator_over_loader_batches(dev, tmp_path):
    import pyarrow.parquet as pq

    from ray_shuffling_data_loader_amd.data_generation import (
        float_data_spec,
        generate_data,
    )
    from ray_shuffling_data_loader_amd.models import fused_eval as fe
    from ray_shuffling_data_loader_amd.torch_dataset import (
        TorchShufflingDataset,
    )

    names = [f"f{i}" for i in range(100)]
    filenames, _ = generate_data(
        300, 4, 1, 0.0, str(tmp_path), spec=float_data_spec(100),
        include_key=False,
    )
    tables = [pq.read_table(f) for f in filenames]
    feats = np.concatenate([
        np.stack([t.column(n).to_numpy() for n in names], 1) for t in tables
    ])
    labels = np.concatenate([t.column("labels").to_numpy() for t in tables])
    n = feats.shape[0]
    assert n == 300

    ds = TorchShufflingDataset(
        list(filenames), num_epochs=1, num_trainers=1, batch_size=64,
        rank=0, num_reducers=2, feature_columns=names,
        feature_types=[torch.bfloat16] * 100, label_column="labels",
        feature_matrix=True, device=dev,
    )
    model = _model(dev)
    ev = fe.FusedEvaluator(model)
    ds.set_epoch(0)
    for d, lab in ds:
        assert d[0].dtype == torch.bfloat16 and d[0].is_cuda
        ev.update(d[0], lab)
    got = ev.compute()
    assert got["rows"] == n
    # all rows in file order; the shuffle must not matter
    x = torch.from_numpy(feats).to(dev).bfloat16()
    t = torch.from_numpy(labels).to(dev).float()
    _check_metrics(got, _metrics(fe.fused_predict(model, x), t))
