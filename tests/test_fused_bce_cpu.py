"""Host logic of the binary-classification objective on CPU:
``fused_step(loss="bce")`` and ``FusedEvaluator(task="binary")`` with the
torch FakeHip mirror of the chain kernels standing in for the extension
(as tests/test_chain_sim.py and tests/test_fused_eval_cpu.py do).

FakeHip has no BCE head, so fused_step takes its documented fallback: the
forward binding with ``target=None`` and the head formed in torch from the
bf16 ``out``. The evaluator's composed path does the same in fp64.

Bounds. Step: those of test_chain_sim.py::test_fused_step_glue_cpu (loss
within 5 %, every gradient within 0.25 * mean|g| + 5e-4 of autograd).
Evaluator: its sums are fp64 sums of fp64 terms of its own bf16 logits, so
they are compared at 1e-12 relative against numpy fp64 on the same logits;
``rows`` and ``accuracy`` (an integer count over rows) are exact.
"""

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


def _data(n, seed=5, soft=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 100, generator=g).bfloat16()
    t = torch.rand(n, 1, generator=g)
    if not soft:
        t = (t >= 0.5).float()
    return x, t


# ---------------------------------------------------------------------
# fused_step(loss="bce")
# ---------------------------------------------------------------------


def _mirror_autograd(model, x, t):
    """Autograd through the mirror's arithmetic (fp32 matmuls on the
    bf16-cast weights) and binary_cross_entropy_with_logits. Returns the
    loss and the gradients w.r.t. the bf16-cast weights and the biases,
    in named_parameters order."""
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    ws = [m.weight.detach().bfloat16().float().requires_grad_() for m in lin]
    bs = [m.bias.detach().clone().requires_grad_() for m in lin]
    h = x.float()
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.t() + b
        if i < 3:
            h = torch.relu(h)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(h, t)
    loss.backward()
    grads = []
    for w, b in zip(ws, bs):
        grads += [w.grad, b.grad]
    return loss.detach(), grads


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("M", [1, 33, 97])
def test_bce_step_matches_autograd(mods, M, soft):
    fs, _ = mods
    model = _model(4)
    x, t = _data(M, seed=10 + M, soft=soft)
    loss = fs.fused_step(model, x, t, loss="bce")
    ref_loss, ref_grads = _mirror_autograd(model, x, t)
    print(f"M={M} loss {loss.item()!r} ref {ref_loss.item()!r}")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(loss.item() - ref_loss.item()) <= 0.05 * ref_loss.item()
    for (n, p), q in zip(model.named_parameters(), ref_grads):
        assert p.grad is not None and p.grad.shape == q.shape, n
        scale = q.abs().mean().clamp(min=1e-6)
        err = (p.grad - q).abs().max()
        print(f"  {n}: err {err.item():.3e} scale {scale.item():.3e}")
        assert err <= 0.25 * scale + 5e-4, (n, err.item(), scale.item())


def test_unknown_loss_raises(mods):
    fs, _ = mods
    model = _model()
    x, t = _data(8)
    with pytest.raises(ValueError, match="'mse' or 'bce'"):
        fs.fused_step(model, x, t, loss="huber")
    for p in model.parameters():
        assert p.grad is None


def test_mse_keyword_is_the_default_call(mods):
    import copy

    fs, _ = mods
    m0 = _model(6)
    m1 = copy.deepcopy(m0)
    x, _ = _data(97)
    t = torch.randn(97, 1, generator=torch.Generator().manual_seed(1))
    l0 = fs.fused_step(m0, x, t)
    l1 = fs.fused_step(m1, x, t, loss="mse")
    assert torch.equal(l0, l1)
    for p, q in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_bce_step_flat_grads_and_hook(mods):
    """The grad_hook staging and flat-grad mode only carry the argument:
    same bits as the plain BCE step."""
    import copy

    fs, _ = mods
    m0 = _model(8)
    m1 = copy.deepcopy(m0)
    x, t = _data(65)
    l0 = fs.fused_step(m0, x, t, loss="bce")
    params = list(m1.parameters())
    flat = torch.zeros(sum(p.numel() for p in params))
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    m1._rsdl_flat_grads = True
    stages = []
    l1 = fs.fused_step(m1, x, t, grad_hook=stages.append, loss="bce")
    assert stages == ["bias", "w1", "w2", "w3"]
    assert torch.equal(l0, l1)
    for p, q in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(p.grad, q.grad)


# ---------------------------------------------------------------------
# FusedEvaluator(task="binary")
# ---------------------------------------------------------------------


def _np_keys(o32):
    bits = o32.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)
    return (u >> 16).astype(np.int64)


def _np_auc(keys, cls):
    pos = np.bincount(keys[cls], minlength=65536).astype(np.float64)
    neg = np.bincount(keys[~cls], minlength=65536).astype(np.float64)
    if pos.sum() == 0 or neg.sum() == 0:
        return float("nan")
    below = np.cumsum(neg) - neg
    return float((pos * (below + neg / 2)).sum() / (pos.sum() * neg.sum()))


def _np_reference(pred, tgt):
    """numpy fp64 metrics of fp32 logits ``pred`` and targets ``tgt``."""
    o32 = pred.reshape(-1).float().numpy()
    o = o32.astype(np.float64)
    t = tgt.reshape(-1).float().numpy().astype(np.float64)
    e = np.exp(-np.abs(o))
    sg = np.where(o >= 0, 1 / (1 + e), e / (1 + e))
    ll = np.maximum(o, 0) - o * t + np.log1p(e)
    cls = t >= 0.5
    n = t.size
    return {
        "rows": n,
        "logloss": ll.sum() / n,
        "accuracy": int(((o >= 0) == cls).sum()) / n,
        "brier": ((sg - t) ** 2).sum() / n,
        "base_rate": t.sum() / n,
        "auc": _np_auc(_np_keys(o32), cls),
    }


def _close(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    assert got["rows"] == want["rows"]
    assert got["accuracy"] == want["accuracy"]
    for k in ("logloss", "brier", "base_rate", "auc"):
        print(f"{k}: got {got[k]!r} want {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (
            k, got[k], want[k])


@pytest.mark.parametrize("soft", [False, True])
def test_binary_evaluator_over_uneven_batches(mods, soft):
    _, fe = mods
    model = _model()
    x, t = _data(sum(BATCHES), soft=soft)
    ev = fe.FusedEvaluator(model, task="binary")
    off, preds = 0, []
    for b in BATCHES:
        ev.update(x[off:off + b], t[off:off + b])
        # same slices: a CPU matmul may round differently at another M
        preds.append(ev.predict(x[off:off + b]))
        off += b
    pred = torch.cat(preds)
    got = ev.compute()
    _close(got, _np_reference(pred, t))
    assert 0.0 <= got["auc"] <= 1.0
    h = ev.hist_state()
    assert h.shape == (2, 65536) and h.dtype == torch.int64
    assert int(h.sum()) == sum(BATCHES)
    cls = (t.reshape(-1) >= 0.5).numpy()
    keys = _np_keys(pred.reshape(-1).numpy())
    want = np.stack([np.bincount(keys[~cls], minlength=65536),
                     np.bincount(keys[cls], minlength=65536)])
    assert np.array_equal(h.numpy(), want)
    st = ev.state()
    assert st.shape == (5,) and st[0].item() == sum(BATCHES)
    ev.reset()
    assert not ev.hist_state().any() and not ev.state().any()
    m = ev.compute()
    assert m["rows"] == 0 and math.isnan(m["logloss"]) and math.isnan(
        m["auc"])


def test_auc_false_omits_key_and_histogram(mods):
    _, fe = mods
    model = _model()
    x, t = _data(97)
    ev = fe.FusedEvaluator(model, task="binary", auc=False)
    ev.update(x, t)
    got = ev.compute()
    assert "auc" not in got
    assert set(got) == {"rows", "logloss", "accuracy", "brier", "base_rate"}
    assert ev.hist_state() is None and ev._hist is None
    full = fe.FusedEvaluator(model, task="binary")
    full.update(x, t)
    want = full.compute()
    want.pop("auc")
    assert got == want


def test_single_class_gives_nan_auc(mods):
    _, fe = mods
    model = _model()
    x, _ = _data(64)
    for label in (0.0, 1.0):
        ev = fe.FusedEvaluator(model, task="binary")
        ev.update(x, torch.full((64, 1), label))
        got = ev.compute()
        assert math.isnan(got["auc"])
        assert got["base_rate"] == label and not math.isnan(got["logloss"])


def test_auc_is_one_half_for_a_constant_logit(mods):
    """All rows tie in one key: the tie-aware statistic is exactly 1/2."""
    _, fe = mods
    model = _model()
    with torch.no_grad():
        for p in model.parameters():
            p.zero_()
    x, t = _data(97)
    ev = fe.FusedEvaluator(model, task="binary")
    ev.update(x, t)
    got = ev.compute()
    assert got["auc"] == 0.5
    assert abs(got["logloss"] - math.log(2.0)) <= 1e-12
    assert got["brier"] == 0.25


def test_regression_task_is_unchanged_and_task_is_validated(mods):
    _, fe = mods
    model = _model()
    x, t = _data(33)
    a = fe.FusedEvaluator(model)
    b = fe.FusedEvaluator(model, task="regression", auc=True)
    a.update(x, t)
    b.update(x, t)
    assert a.compute() == b.compute()
    assert set(a.compute()) == {"rows", "mse", "rmse", "mae", "r2"}
    assert b.hist_state() is None
    with pytest.raises(ValueError, match="'regression' or 'binary'"):
        fe.FusedEvaluator(model, task="multiclass")


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
        lo, hi = (0, 77) if rank == 0 else (77, 200)  # unequal halves
        ev = fused_eval.FusedEvaluator(model, task="binary")
        ev.update(x[lo:hi], t[lo:hi])
        local = ev.state().tolist()
        local_hist = int(ev.hist_state().sum())
        result_q.put((rank, ev.compute(), (local, local_hist)))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        import traceback

        result_q.put((rank, "ERR", f"{e}\n{traceback.format_exc()}"))


def test_binary_compute_all_reduces_under_gloo(mods, mp_spawn_context):
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
    # states stay local
    assert results[0][0] == results[1][0]
    assert results[0][1][0][0] == 77 and results[1][1][0][0] == 123
    assert results[0][1][1] == 77 and results[1][1][1] == 123
    model = _model()
    x, t = _data(200)
    ev = fe.FusedEvaluator(model, task="binary")
    pred = torch.cat([ev.predict(x[:77]), ev.predict(x[77:])])
    _close(results[0][0], _np_reference(pred, t))
