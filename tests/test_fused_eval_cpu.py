"""Host logic of models/fused_eval.py on CPU: the composed path (the
training forward binding's ``out`` + fp64 torch accumulation) with the
torch FakeHip mirror of the chain kernels standing in for the extension,
as tests/test_chain_sim.py does for fused_step.

Reference: the same MLP written out with torch ops on the bf16-cast
weights in fp32. FakeHip's ``out`` is bf16, so the composed path's
predictions may differ from that fp32 reference by the bf16 rounding of
the head value, half an ulp = 2^-9 relative; the bound used is one full
ulp, 2^-8 |ref|, plus 1e-6 for values near zero. The accumulated metrics
are fp64 sums of the evaluator's own predictions, so they are compared
against fp64 metrics of ``fused_predict``'s outputs at 1e-12 relative
(a handful of fp64 roundings over a few hundred terms).
"""

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BATCHES = [64, 33, 1, 161]


@pytest.fixture()
def fe(monkeypatch):
    from _fake_hip import FakeHip
    import ray_shuffling_data_loader_amd.ops.shuffle_ops as so
    from ray_shuffling_data_loader_amd.models import fused_eval

    monkeypatch.setattr(so, "_load_hip", lambda: FakeHip)
    return fused_eval


def _model(seed=3):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    return TabularMLP(100)


def _data(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 100, generator=g).bfloat16(),
            torch.randn(n, 1, generator=g))


def _ref_pred(model, x):
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    h = x.float()
    for i, m in enumerate(lin):
        h = h @ m.weight.detach().bfloat16().float().t() + m.bias.detach()
        if i < 3:
            h = torch.relu(h)
    return h


def _metrics(pred, tgt):
    p = pred.reshape(-1).double()
    t = tgt.reshape(-1).float().double()
    n = t.numel()
    sse = ((p - t) ** 2).sum().item()
    return {
        "rows": n,
        "mse": sse / n,
        "rmse": math.sqrt(sse / n),
        "mae": (p - t).abs().sum().item() / n,
        "r2": 1.0 - sse / ((t * t).sum().item() - t.sum().item() ** 2 / n),
    }


def _close(got, want, rel=1e-12):
    assert got["rows"] == want["rows"]
    for k in ("mse", "rmse", "mae", "r2"):
        assert abs(got[k] - want[k]) <= rel * max(abs(want[k]), 1.0), (
            k, got[k], want[k])


def test_fused_predict_matches_torch_reference(fe):
    model = _model()
    x, _ = _data(161)
    pred = fe.fused_predict(model, x)
    assert pred.shape == (161, 1) and pred.dtype == torch.float32
    ref = _ref_pred(model, x)
    err = (pred - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-6
    assert bool((err <= bound).all()), (err - bound).max().item()
    # the composed path's predictions are bf16 values
    assert torch.equal(pred, pred.bfloat16().float())


def test_accumulates_across_unequal_batches(fe):
    model = _model()
    x, t = _data(sum(BATCHES))
    ev = fe.FusedEvaluator(model)
    off, preds = 0, []
    for b in BATCHES:
        ev.update(x[off:off + b], t[off:off + b])
        # same slices: a CPU matmul may round differently at another M
        preds.append(fe.fused_predict(model, x[off:off + b]))
        off += b
    got = ev.compute()
    _close(got, _metrics(torch.cat(preds), t))
    # The fp32 reference's metrics are within what bf16 predictions allow:
    # |d mse| <= (2 * mean|o - t| + max|dpred|) * max|dpred|, with
    # |dpred| <= 2^-8 max|ref|. One pass over everything (fp64 targets,
    # read as fp32) regroups the same sums and lies within it too.
    ref = _ref_pred(model, x)
    want = _metrics(ref, t)
    dp = 2.0 ** -8 * ref.abs().max().item() + 1e-6
    slack = (2 * want["mae"] + dp) * dp
    assert abs(got["mse"] - want["mse"]) <= slack
    whole = fe.FusedEvaluator(model)
    whole.update(x, t.double())
    assert whole.compute()["rows"] == sum(BATCHES)
    assert abs(whole.compute()["mse"] - want["mse"]) <= slack


def test_reset_and_empty_batch(fe):
    model = _model()
    x, t = _data(97)
    ev = fe.FusedEvaluator(model)
    ev.update(x, t)
    before = ev.state()
    ev.update(x[:0], t[:0])  # no-op
    assert torch.equal(ev.state(), before)
    assert fe.fused_predict(model, x[:0]).shape == (0, 1)
    ev.reset()
    assert torch.equal(ev.state(), torch.zeros(5, dtype=torch.float64))
    ev.update(x[:33], t[:33])
    _close(ev.compute(), _metrics(fe.fused_predict(model, x[:33]), t[:33]))


def test_zero_rows_give_nan_metrics(fe):
    ev = fe.FusedEvaluator(_model())
    for m in (ev.compute(),):
        assert m["rows"] == 0
        for k in ("mse", "rmse", "mae", "r2"):
            assert math.isnan(m[k]), k
    ev.update(*_data(8))
    ev.reset()
    assert math.isnan(ev.compute()["mse"])


def test_input_rejection(fe):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    model = _model()
    x, t = _data(16)
    ev = fe.FusedEvaluator(model)
    strided = torch.cat([x, x], 1)[:, :100]  # right shape, not contiguous
    for bad in (x.float(), x[:, :64].contiguous(), strided):
        with pytest.raises(RuntimeError,
                           match=r"x must be contiguous bf16 \[M,100\]"):
            ev.update(bad, t)
        with pytest.raises(RuntimeError,
                           match=r"x must be contiguous bf16 \[M,100\]"):
            fe.fused_predict(model, bad)
    with pytest.raises(RuntimeError, match="target size mismatch"):
        ev.update(x, t[:8])
    with pytest.raises(AssertionError,
                       match="requires the stock TabularMLP"):
        fe.FusedEvaluator(TabularMLP(100, depth=2))
    with pytest.raises(AssertionError):
        fe.FusedEvaluator(TabularMLP(100, hidden=256))
    assert torch.equal(ev.state(), torch.zeros(5, dtype=torch.float64))


def test_evaluation_has_no_side_effects(fe):
    model = _model()
    x, t = _data(65)
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    model.train()
    ev = fe.FusedEvaluator(model)
    ev.update(x, t)
    a = ev.compute()
    model.eval()
    ev.reset()
    ev.update(x, t)
    assert ev.compute() == a  # model.training does not matter
    for n, p in model.named_parameters():
        assert p.grad is None, n
        assert torch.equal(p.detach(), params[n]), n


def test_weights_are_followed(fe):
    model = _model()
    x, _ = _data(40)
    ev = fe.FusedEvaluator(model)
    first = ev.predict(x)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)
    second = ev.predict(x)
    assert torch.equal(second, fe.FusedEvaluator(model).predict(x))
    assert not torch.equal(first, second)


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
        ev = fused_eval.FusedEvaluator(model)
        ev.update(x[lo:hi], t[lo:hi])
        local = ev.state().tolist()
        result_q.put((rank, ev.compute(), local))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        import traceback

        result_q.put((rank, "ERR", f"{e}\n{traceback.format_exc()}"))


def test_compute_all_reduces_under_gloo(fe, mp_spawn_context):
    import socket

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
    # both ranks report the metrics of the whole, bit-equal
    assert results[0][0] == results[1][0]
    assert results[0][1][0] == 77 and results[1][1][0] == 123
    model = _model()
    x, t = _data(200)
    pred = torch.cat([fe.fused_predict(model, x[:77]),
                      fe.fused_predict(model, x[77:])])
    _close(results[0][0], _metrics(pred, t))
