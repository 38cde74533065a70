"""Host logic of sample weights and pos_weight on CPU:
``fused_step(sample_weight=, pos_weight=)`` and
``FusedEvaluator(weighted=True)`` with the torch FakeHip mirror of the chain
kernels standing in for the extension (as tests/test_fused_bce_cpu.py does).

FakeHip has no weighted head (no HEAD_WEIGHTS), so fused_step takes its
documented fallback: the forward binding with ``target=None`` and the head
formed in torch (``fused_step.loss_head``) from the bf16 ``out``. The
evaluator's composed path does the same in fp64.

Bounds. Step: those of test_fused_bce_cpu.py::test_bce_step_matches_autograd
(loss within 5 %, every gradient within 0.25 * mean|g| + 5e-4 of autograd).
Evaluator: those of test_binary_evaluator_over_uneven_batches — fp64 sums of
fp64 terms of its own bf16 logits against numpy fp64 on the same logits at
1e-12 relative; ``rows`` exact, and ``accuracy`` and ``weight_sum`` exact
too, because the weights are multiples of 1/16 and their sums are exact in
fp64. The weights are also multiples of 2^-20, so the fixed-point histogram
represents them exactly and the weighted AUC is held to the same 1e-12
against a direct pairwise Mann-Whitney statistic.
"""

import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BATCHES = [97, 64, 1]


@pytest.fixture()
def mods(monkeypatch):
    from _fake_hip import FakeHip
    import ray_shuffling_data_loader_amd.ops.shuffle_ops as so
    from ray_shuffling_data_loader_amd.models import fused_eval, fused_step

    monkeypatch.setattr(so, "_load_hip", lambda: FakeHip)
    return fused_step, fused_eval


def _model(seed=3):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    return TabularMLP(100)


def _data(n, seed=5, soft=False, regression=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 100, generator=g).bfloat16()
    if regression:
        return x, torch.randn(n, 1, generator=g)
    t = torch.rand(n, 1, generator=g)
    if not soft:
        t = (t >= 0.5).float()
    return x, t


def _weights(n, seed=9):
    """Multiples of 1/16 in [0, 4], every fifth one (from row 3) exactly 0."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(1, 65, (n,), generator=g).float() / 16.0
    w[3::5] = 0.0
    return w


# ---------------------------------------------------------------------
# fused_step(sample_weight=, pos_weight=)
# ---------------------------------------------------------------------


def _mirror_autograd(model, x, t, loss, w, pos_weight):
    """Autograd through the mirror's arithmetic (fp32 matmuls on the
    bf16-cast weights) and torch's weighted losses, mean over the batch."""
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    ws = [m.weight.detach().bfloat16().float().requires_grad_() for m in lin]
    bs = [m.bias.detach().clone().requires_grad_() for m in lin]
    h = x.float()
    for i, (wt, b) in enumerate(zip(ws, bs)):
        h = h @ wt.t() + b
        if i < 3:
            h = torch.relu(h)
    if loss == "bce":
        pw = None if pos_weight is None else torch.tensor([pos_weight])
        val = torch.nn.functional.binary_cross_entropy_with_logits(
            h, t, weight=w.reshape(-1, 1), pos_weight=pw)
    else:
        val = (w.reshape(-1, 1) * (h - t) ** 2).mean()
    val.backward()
    grads = []
    for wt, b in zip(ws, bs):
        grads += [wt.grad, b.grad]
    return val.detach(), grads


CASES = [("mse", False, None), ("bce", False, None), ("bce", True, None),
         ("bce", False, 3.0), ("bce", True, 3.0)]


@pytest.mark.parametrize("loss,soft,pos_weight", CASES)
@pytest.mark.parametrize("M", [1, 33, 97])
def test_weighted_step_matches_autograd(mods, M, loss, soft, pos_weight):
    fs, _ = mods
    model = _model(4)
    x, t = _data(M, seed=10 + M, soft=soft, regression=loss == "mse")
    w = _weights(M)
    got = fs.fused_step(model, x, t, loss=loss, sample_weight=w,
                        pos_weight=pos_weight)
    ref_loss, ref_grads = _mirror_autograd(model, x, t, loss, w, pos_weight)
    print(f"M={M} loss {got.item()!r} ref {ref_loss.item()!r}")
    assert got.dtype == torch.float32 and got.dim() == 0
    assert abs(got.item() - ref_loss.item()) <= 0.05 * ref_loss.item()
    for (n, p), q in zip(model.named_parameters(), ref_grads):
        assert p.grad is not None and p.grad.shape == q.shape, n
        scale = q.abs().mean().clamp(min=1e-6)
        err = (p.grad - q).abs().max()
        print(f"  {n}: err {err.item():.3e} scale {scale.item():.3e}")
        assert err <= 0.25 * scale + 5e-4, (n, err.item(), scale.item())


@pytest.mark.parametrize("loss", ["mse", "bce"])
@pytest.mark.parametrize("shape", ["flat", "column", "fp64"])
def test_unit_weights_are_the_unweighted_call(mods, loss, shape):
    fs, _ = mods
    m0 = _model(6)
    m1 = copy.deepcopy(m0)
    x, t = _data(97, regression=loss == "mse")
    ones = torch.ones(97, 1) if shape == "column" else torch.ones(97)
    if shape == "fp64":
        ones = ones.double()
    l0 = fs.fused_step(m0, x, t, loss=loss)
    l1 = fs.fused_step(m1, x, t, loss=loss, sample_weight=ones,
                       pos_weight=None)
    assert torch.equal(l0, l1)
    for p, q in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_bce_head_keeps_its_signature_and_results(mods):
    fs, _ = mods
    g = torch.Generator().manual_seed(2)
    out = (4 * torch.randn(65, 1, generator=g)).bfloat16()
    t = torch.rand(65, 1, generator=g)
    dyb, part = fs.bce_head(out, t, 65)
    dyw, partw = fs.loss_head(out, t, 65, "bce", torch.ones(65), None)
    assert torch.equal(dyb, dyw) and torch.equal(part, partw)
    dyz, partz = fs.loss_head(out, t, 65, "bce", torch.zeros(65), 3.0)
    assert not dyz.float().any() and partz.item() == 0.0


def test_weighted_step_flat_grads_and_hook(mods):
    """The grad_hook staging and flat-grad mode only carry the arguments:
    same bits as the plain weighted step."""
    fs, _ = mods
    m0 = _model(8)
    m1 = copy.deepcopy(m0)
    x, t = _data(65)
    w = _weights(65)
    l0 = fs.fused_step(m0, x, t, loss="bce", sample_weight=w,
                       pos_weight=3.0)
    params = list(m1.parameters())
    flat = torch.zeros(sum(p.numel() for p in params))
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    m1._rsdl_flat_grads = True
    stages = []
    l1 = fs.fused_step(m1, x, t, grad_hook=stages.append, loss="bce",
                       sample_weight=w, pos_weight=3.0)
    assert stages == ["bias", "w1", "w2", "w3"]
    assert torch.equal(l0, l1)
    for p, q in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(p.grad, q.grad)
    # and the weights did something
    m2 = copy.deepcopy(m0)
    l2 = fs.fused_step(m2, x, t, loss="bce")
    assert not torch.equal(l0, l2)


def test_argument_validation(mods):
    fs, _ = mods
    model = _model()
    x, t = _data(8)
    with pytest.raises(ValueError, match="sample_weight has 7 values"):
        fs.fused_step(model, x, t, loss="bce", sample_weight=torch.ones(7))
    with pytest.raises(ValueError, match="pos_weight needs loss='bce'"):
        fs.fused_step(model, x, t, pos_weight=2.0)
    with pytest.raises(ValueError, match="pos_weight needs loss='bce'"):
        fs.fused_step(model, x, t, loss="mse", pos_weight=1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and > 0"):
            fs.fused_step(model, x, t, loss="bce", pos_weight=bad)
    for p in model.parameters():
        assert p.grad is None


# ---------------------------------------------------------------------
# FusedEvaluator(weighted=True)
# ---------------------------------------------------------------------


def _np_keys(o32):
    bits = o32.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)
    return (u >> 16).astype(np.int64)


def _np_weighted_auc(keys, cls, w):
    """Pairwise weighted Mann-Whitney on the truncated logits (the keys
    order as they do), fp64: ties count one half."""
    kp, wp = keys[cls], w[cls]
    kn, wn = keys[~cls], w[~cls]
    if wp.sum() == 0 or wn.sum() == 0:
        return float("nan")
    gt = (kp[:, None] > kn[None, :]).astype(np.float64)
    eq = (kp[:, None] == kn[None, :]).astype(np.float64)
    pair = wp[:, None] * wn[None, :]
    return float((pair * (gt + 0.5 * eq)).sum() / (wp.sum() * wn.sum()))


def _np_reference(pred, tgt, w, task):
    o32 = pred.reshape(-1).float().numpy()
    o = o32.astype(np.float64)
    t = tgt.reshape(-1).float().numpy().astype(np.float64)
    w = w.reshape(-1).float().numpy().astype(np.float64)
    sw = w.sum()
    res = {"rows": t.size, "weight_sum": sw}
    if task == "regression":
        d = o - t
        mse = (w * d * d).sum() / sw
        den = (w * t * t).sum() - (w * t).sum() ** 2 / sw
        res.update({"mse": mse, "rmse": math.sqrt(mse),
                    "mae": (w * np.abs(d)).sum() / sw,
                    "r2": 1.0 - (w * d * d).sum() / den})
        return res
    e = np.exp(-np.abs(o))
    sg = np.where(o >= 0, 1 / (1 + e), e / (1 + e))
    ll = np.maximum(o, 0) - o * t + np.log1p(e)
    cls = t >= 0.5
    res.update({
        "logloss": (w * ll).sum() / sw,
        "accuracy": (w * ((o >= 0) == cls)).sum() / sw,
        "brier": (w * (sg - t) ** 2).sum() / sw,
        "base_rate": (w * t).sum() / sw,
        "auc": _np_weighted_auc(_np_keys(o32), cls, w),
    })
    return res


def _close(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in ("rows", "weight_sum", "accuracy"):
        if k in want:
            assert got[k] == want[k], (k, got[k], want[k])
    for k in want:
        print(f"{k}: got {got[k]!r} want {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (
            k, got[k], want[k])


def _run(ev, x, t, w):
    off, preds = 0, []
    for b in BATCHES:
        ev.update(x[off:off + b], t[off:off + b], w[off:off + b])
        # same slices: a CPU matmul may round differently at another M
        preds.append(ev.predict(x[off:off + b]))
        off += b
    return torch.cat(preds)


@pytest.mark.parametrize("soft", [False, True])
def test_weighted_binary_evaluator_over_uneven_batches(mods, soft):
    _, fe = mods
    model = _model()
    n = sum(BATCHES)
    x, t = _data(n, soft=soft)
    w = _weights(n)
    ev = fe.FusedEvaluator(model, task="binary", weighted=True)
    pred = _run(ev, x, t, w)
    got = ev.compute()
    _close(got, _np_reference(pred, t, w, "binary"))
    assert 0.0 <= got["auc"] <= 1.0
    h = ev.hist_state()
    assert h.shape == (2, 65536) and h.dtype == torch.int64
    units = torch.round(w * 2.0 ** 20).long()
    assert int(h.sum()) == int(units.sum())
    cls = (t.reshape(-1) >= 0.5)
    idx = cls.long() * 65536 + torch.from_numpy(
        _np_keys(pred.reshape(-1).numpy()))
    want = torch.zeros(2 * 65536, dtype=torch.int64).index_add_(
        0, idx, units).view(2, 65536)
    assert torch.equal(h, want)
    st = ev.state()
    assert st.shape == (6,) and st.dtype == torch.float64
    assert st[0].item() == n and st[5].item() == w.double().sum().item()
    ev.reset()
    assert not ev.hist_state().any() and not ev.state().any()
    m = ev.compute()
    assert m["rows"] == 0 and m["weight_sum"] == 0.0
    assert math.isnan(m["logloss"]) and math.isnan(m["auc"])


def test_weighted_regression_evaluator_over_uneven_batches(mods):
    _, fe = mods
    model = _model()
    n = sum(BATCHES)
    x, t = _data(n, regression=True)
    w = _weights(n)
    ev = fe.FusedEvaluator(model, weighted=True)
    pred = _run(ev, x, t, w)
    got = ev.compute()
    _close(got, _np_reference(pred, t, w, "regression"))
    assert ev.hist_state() is None and ev.state().shape == (6,)


def test_unit_weights_give_the_unweighted_metrics(mods):
    _, fe = mods
    model = _model()
    x, t = _data(97)
    a = fe.FusedEvaluator(model, task="binary")
    b = fe.FusedEvaluator(model, task="binary", weighted=True)
    a.update(x, t)
    b.update(x, t, torch.ones(97, 1, dtype=torch.float64))
    ma, mb = a.compute(), b.compute()
    assert mb.pop("weight_sum") == 97.0
    assert ma == mb
    assert a.state().shape == (5,)
    assert torch.equal(a.hist_state() * (1 << 20), b.hist_state())


def test_weight_arguments_are_checked(mods):
    _, fe = mods
    model = _model()
    x, t = _data(8)
    plain = fe.FusedEvaluator(model, task="binary")
    with pytest.raises(ValueError, match="weighted=True"):
        plain.update(x, t, torch.ones(8))
    assert not plain.state().any()
    ev = fe.FusedEvaluator(model, task="binary", weighted=True)
    with pytest.raises(ValueError, match="needs update"):
        ev.update(x, t)
    with pytest.raises(ValueError, match="7 values for 8 rows"):
        ev.update(x, t, torch.ones(7))
    assert not ev.state().any()


@pytest.mark.parametrize("task", ["regression", "binary"])
def test_zero_weight_sum_gives_nan(mods, task):
    _, fe = mods
    model = _model()
    x, t = _data(33)
    ev = fe.FusedEvaluator(model, task=task, weighted=True)
    ev.update(x, t, torch.zeros(33))
    got = ev.compute()
    assert got["rows"] == 33 and got["weight_sum"] == 0.0
    for k, v in got.items():
        if k not in ("rows", "weight_sum"):
            assert math.isnan(v), (k, v)


def test_single_class_gives_nan_weighted_auc(mods):
    _, fe = mods
    model = _model()
    x, _ = _data(64)
    w = _weights(64)
    for label in (0.0, 1.0):
        ev = fe.FusedEvaluator(model, task="binary", weighted=True)
        ev.update(x, torch.full((64, 1), label), w)
        got = ev.compute()
        assert math.isnan(got["auc"])
        assert got["base_rate"] == label and not math.isnan(got["logloss"])
    # the other class present, but only at weight 0: absent all the same
    t = torch.ones(64, 1)
    t[3] = 0.0
    assert w[3] == 0.0
    ev = fe.FusedEvaluator(model, task="binary", weighted=True)
    ev.update(x, t, w)
    assert math.isnan(ev.compute()["auc"])


def _gloo_worker(rank, world, port, result_q):
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, os.path.dirname(here))
        sys.path.insert(0, here)
        import torch.distributed as dist

        from _fake_hip import FakeHip
        import ray_shuffling_data_loader_amd.ops.shuffle_ops as so
        from ray_shuffling_data_loader_amd.models import fused_eval

        so._load_hip = lambda: FakeHip
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)

        model = _model()
        x, t = _data(200)
        w = _weights(200)
        lo, hi = (0, 77) if rank == 0 else (77, 200)  # unequal halves
        ev = fused_eval.FusedEvaluator(model, task="binary", weighted=True)
        ev.update(x[lo:hi], t[lo:hi], w[lo:hi])
        local = ev.state().tolist()
        local_hist = int(ev.hist_state().sum())
        result_q.put((rank, ev.compute(), (local, local_hist)))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        import traceback

        result_q.put((rank, "ERR", f"{e}\n{traceback.format_exc()}"))


def test_weighted_compute_all_reduces_under_gloo(mods, mp_spawn_context):
    import socket

    _, fe = mods
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    rq = mp_spawn_context.Queue()
    procs = [
        mp_spawn_context.Process(target=_gloo_worker, args=(r, 2, port, rq))
        for r in range(2)
    ]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, metrics, local = rq.get(timeout=300)
        assert metrics != "ERR", local
        results[rank] = (metrics, local)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # both ranks report the metrics of the whole, bit-equal; their own
    # states (six sums, histogram) stay local
    assert results[0][0] == results[1][0]
    w = _weights(200)
    units = torch.round(w * 2.0 ** 20).long()
    for rank, (lo, hi) in enumerate([(0, 77), (77, 200)]):
        local, local_hist = results[rank][1]
        assert len(local) == 6 and local[0] == hi - lo
        assert local[5] == w[lo:hi].double().sum().item()
        assert local_hist == int(units[lo:hi].sum())
    model = _model()
    x, t = _data(200)
    ev = fe.FusedEvaluator(model, task="binary")
    pred = torch.cat([ev.predict(x[:77]), ev.predict(x[77:])])
    _close(results[0][0], _np_reference(pred, t, w, "binary"))
