"""GPU tests of the fused optimizer (csrc/step_glue.hip step_update and
step_finalize_update, models/fused_optim.py): the kernels against the
numpy oracle of tests/_optim_cases.py bit for bit, the staged bf16 buffers
against hip.step_prep (the already pinned kernel), ``fused_step(optimizer=)``
against ``fused_step`` followed by ``step()``, the staging validity rule,
the evaluator's cache and the launch count.

fp32 values are compared as bits, except that any NaN equals any NaN where
the salted gradients overflow (inf - inf): the payload of a generated NaN
is the processor's own. bf16 images are compared as bits throughout (a NaN
images as 0x7FC0 on both sides)."""

import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _optim_cases as oc  # noqa: E402
from test_step_glue_gpu import (  # noqa: E402
    _fin_oracle,
    _int_parts,
    _nan_outs,
    _salt,
)

pytestmark = pytest.mark.gpu

STAGE_NUMEL = [512 * 112, 256 * 512, 128 * 256, 256 * 512, 128 * 256, 128]
STAGE_NAMES = ["W1s", "W2s", "W3s", "W2Ts", "W3Ts", "w4b"]
NAMES = ["W1", "W2", "W3", "w4", "b1", "b2", "b3", "b4"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    h = shuffle_ops._load_hip()
    assert h.STEP_OPTIM == 1
    return h


def _hyper(kind, t, grad_scale, lr, momentum=0.0, nesterov=False,
           weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
    """hyper= of the bindings, in fp64, from the specification."""
    if kind == "sgd":
        return [grad_scale, lr, momentum, weight_decay,
                1.0 if nesterov else 0.0]
    b1, b2 = betas
    return [grad_scale, 1.0 - lr * weight_decay, 1.0 - b1, b2, 1.0 - b2,
            lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), eps]


def _masters(dev, seed, salted):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for s in oc.SHAPES:
        w = torch.randn(s, device=dev, generator=g) / 8
        out.append(_salt(w, dev) if salted and w.numel() >= 128 else w)
    return out


def _nan_staged(dev):
    """Staged buffers as their owner creates them, except that everything
    the update must write is NaN: only W1s columns 100..111 are zero."""
    nan = torch.tensor([0x7FC1], dtype=torch.int16, device=dev)
    bufs = [nan.expand(n).contiguous().view(torch.bfloat16)
            for n in STAGE_NUMEL]
    w1 = bufs[0].view(16, 7, 2, 32, 8)
    w1[:, 6, 1] = 0
    w1[:, 6, 0, :, 4:] = 0
    return bufs


def _n_state(kind, kw):
    if kind == "adamw":
        return 2
    return 1 if kw.get("momentum") else 0


def _zero_state(dev, kind, kw):
    return [torch.zeros(s, device=dev)
            for _ in range(_n_state(kind, kw)) for s in oc.SHAPES]


def _np(t):
    return t.detach().cpu().numpy()


def _bits16(t):
    return _np(t.view(torch.int16)).view(np.uint16)


def _check_against_oracle(ora, params, state, bufs, tag):
    for i, n in enumerate(NAMES):
        assert oc.same_f32(_np(params[i]), ora.p[i]), (tag, n)
    for s, want in enumerate([ora.s1, ora.s2][:len(state) // 8]):
        for i, n in enumerate(NAMES):
            assert oc.same_f32(_np(state[s * 8 + i]), want[i]), (tag, s, n)
    for n, b, w in zip(STAGE_NAMES, bufs, oc.staged(ora.p)):
        assert np.array_equal(_bits16(b), w), (tag, n)
    assert not oc.w1s_pad(_bits16(bufs[0])).any(), tag


UPDATE_CASES = [
    ("sgd", {}, 1.0),
    ("sgd", {"momentum": 0.9, "weight_decay": 1e-2}, 1.0),
    ("sgd", {"momentum": 0.9, "nesterov": True}, 0.5),
    ("adamw", {}, 1.0),
    ("adamw", {"weight_decay": 1e-2, "betas": (0.8, 0.99), "eps": 1e-6},
     0.5),
]


@pytest.mark.parametrize("kind,kw,grad_scale", UPDATE_CASES)
def test_step_update_matches_oracle(dev, hip, kind, kw, grad_scale):
    P = _masters(dev, 1, salted=True)
    state = _zero_state(dev, kind, kw)
    bufs = _nan_staged(dev)
    ora = oc.Oracle(kind, [_np(p) for p in P], **kw)
    code = hip.OPT_SGD if kind == "sgd" else hip.OPT_ADAMW
    versions = [p._version for p in P]
    for t in range(3):
        lr = [1e-2, 5e-3, 1e-3][t]
        grads = _masters(dev, 10 + t, salted=True)
        kept = [g.clone() for g in grads]
        hip.step_update(grads, P[:4], P[4:], state, bufs, code,
                        _hyper(kind, t + 1, grad_scale, lr, **kw))
        ora.step([_np(g) for g in grads], lr, grad_scale)
        for g, k in zip(grads, kept):
            assert torch.equal(g.view(torch.int32), k.view(torch.int32))
        _check_against_oracle(ora, P, state, bufs, (kind, t))
    # every written tensor's version counter moved once per step
    assert [p._version for p in P] == [v + 3 for v in versions]


def test_update_refusals_name_the_tensor(dev, hip):
    P = _masters(dev, 2, salted=False)
    grads = _masters(dev, 3, salted=False)
    bufs = _nan_staged(dev)
    before = [p.clone() for p in P]
    h = _hyper("sgd", 1, 1.0, 1e-2, momentum=0.9)
    state = _zero_state(dev, "sgd", {"momentum": 0.9})
    bad = list(state)
    bad[3] = torch.zeros(127, device=dev)
    with pytest.raises(RuntimeError, match="state 3"):
        hip.step_update(grads, P[:4], P[4:], bad, bufs, hip.OPT_SGD, h)
    with pytest.raises(RuntimeError, match="state must hold 0"):
        hip.step_update(grads, P[:4], P[4:], state, bufs, hip.OPT_SGD,
                        _hyper("sgd", 1, 1.0, 1e-2))
    with pytest.raises(RuntimeError, match="state must hold 16"):
        hip.step_update(grads, P[:4], P[4:], state, bufs, hip.OPT_ADAMW,
                        _hyper("adamw", 1, 1.0, 1e-2))
    badg = list(grads)
    badg[1] = torch.zeros(256 * 512 + 1, device=dev)[1:]  # misaligned
    with pytest.raises(RuntimeError, match="grad 1 must be 16-byte"):
        hip.step_update(badg, P[:4], P[4:], state, bufs, hip.OPT_SGD, h)
    badb = list(bufs)
    badb[4] = torch.zeros(128 * 256, device=dev)  # fp32, not bf16
    with pytest.raises(RuntimeError, match="staged buffer 4"):
        hip.step_update(grads, P[:4], P[4:], state, badb, hip.OPT_SGD, h)
    with pytest.raises(RuntimeError, match="kind"):
        hip.step_update(grads, P[:4], P[4:], state, bufs, 7, h)
    with pytest.raises(RuntimeError, match="weight 2"):
        hip.step_update(grads, [P[0], P[1], P[2].double(), P[3]], P[4:],
                        state, bufs, hip.OPT_SGD, h)
    for p, b in zip(P, before):
        assert torch.equal(p, b)
    assert all(not s.any() for s in state)


@pytest.mark.parametrize("kind,kw", [
    ("sgd", {"momentum": 0.9, "nesterov": True, "weight_decay": 1e-2}),
    ("adamw", {"weight_decay": 1e-2}),
])
@pytest.mark.parametrize("db_rows", [1, 65])
@pytest.mark.parametrize("ns", [(1, 1, 1), (3, 5, 8)])
def test_finalize_update_integer_partials(dev, hip, ns, db_rows, kind, kw):
    """The partials of test_finalize_integer_partials: the gradients must
    equal part.sum(0) bit for bit, parameters and state the oracle applied
    to those gradients, and the staged buffers hip.step_prep of the
    updated masters. NaN sits in every pad column of part1, in
    db_part[:, 1153:], in the pre-filled gradient outputs and in the
    staged buffers: none of it may survive."""
    p1, p2, p3, dbp, lp = _int_parts(dev, ns, db_rows, db_rows, sum(ns))
    p1.view(-1, 512, 128)[:, :, 100:] = float("nan")
    dbp[:, 1153:] = float("nan")
    M = 4096
    want = _fin_oracle(torch.nan_to_num(p1, nan=0.0), p2, p3,
                       torch.nan_to_num(dbp, nan=0.0), lp, M)
    P = _masters(dev, 4, salted=False)
    state = _zero_state(dev, kind, kw)
    bufs = _nan_staged(dev)
    ora = oc.Oracle(kind, [_np(p) for p in P], **kw)
    code = hip.OPT_SGD if kind == "sgd" else hip.OPT_ADAMW
    for t in range(2):
        outs = _nan_outs(dev)
        got = hip.step_finalize_update(
            p1, p2, p3, dbp, lp, M, outs, P[:4], P[4:], state, bufs, code,
            _hyper(kind, t + 1, 1.0, 1e-2, **kw))
        for g, o in zip(got[1:], outs):
            assert g.data_ptr() == o.data_ptr()
        for n, g, w in zip(["loss"] + NAMES, got, want):
            assert g.shape == w.shape, n
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), n
        # and exactly what step_finalize gives
        for g, w in zip(got, hip.step_finalize(p1, p2, p3, dbp, lp, M)):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
        ora.step([_np(g) for g in got[1:]], 1e-2)
        _check_against_oracle(ora, P, state, bufs, (kind, t))
        for n, b, w in zip(STAGE_NAMES, bufs, hip.step_prep(P[:4])):
            assert torch.equal(b.view(torch.int16), w.view(torch.int16)), n
        for t_ in list(got) + P + state:
            assert torch.isfinite(t_).all()
        for b in bufs:
            assert torch.isfinite(b.float()).all()


# ---------------------------------------------------------------------
# whole step
# ---------------------------------------------------------------------

KINDS = {
    "sgd": {"lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-4},
    "adamw": {"lr": 1e-3, "weight_decay": 1e-2},
}


def _model_and_opt(dev, kind, seed):
    from ray_shuffling_data_loader_amd.models.fused_optim import (
        FusedOptimizer,
    )
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    model = TabularMLP(100).to(dev)
    return model, FusedOptimizer(model, kind, **KINDS[kind])


def _twin(model, opt):
    from ray_shuffling_data_loader_amd.models.fused_optim import (
        FusedOptimizer,
    )

    m2 = copy.deepcopy(model)
    for p in m2.parameters():
        p.grad = None
    o2 = FusedOptimizer(m2, opt.kind, lr=1.0)
    o2.load_state_dict(opt.state_dict())
    return m2, o2


def _batch(dev, M, loss, tdtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, 100, device=dev, generator=g)
    y = x[:, :4].sum(1, keepdim=True) + 3.0  # learnable
    if loss == "bce":
        # ~84 % positives: the head bias, read in fp32, has a gradient
        # that lowers the loss at once, whatever the bf16 images do
        y = (y > 1.0).float()
    return x.bfloat16(), y.to(tdtype)


def _assert_same_run(tag, m_a, o_a, m_b, o_b):
    for (n, p), q in zip(m_a.named_parameters(), m_b.parameters()):
        assert torch.equal(p.grad.view(torch.int32),
                           q.grad.view(torch.int32)), (tag, n, "grad")
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (
            tag, n)
        assert o_a.state[n].keys() == o_b.state[n].keys()
        for s in o_a.state[n]:
            assert torch.equal(o_a.state[n][s].view(torch.int32),
                               o_b.state[n][s].view(torch.int32)), (tag, n, s)
    for n, a, b in zip(STAGE_NAMES, o_a._staged, o_b._staged):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (
            tag, n)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("loss", ["mse", "bce"])
@pytest.mark.parametrize("m_rows", [1, 33, 4097])
def test_fused_step_with_optimizer_is_step_then_update(
        dev, hip, m_rows, loss, tdtype, kind):
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step

    m_a, o_a = _model_and_opt(dev, kind, 100 + m_rows)
    m_b, o_b = _twin(m_a, o_a)
    x, y = _batch(dev, m_rows, loss, tdtype, m_rows)
    start = [p.detach().clone() for p in m_a.parameters()]
    losses = []
    for t in range(3):
        l_a = fused_step(m_a, x, y, loss=loss, optimizer=o_a)
        l_b = fused_step(m_b, x, y, loss=loss)
        o_b.step()
        assert torch.equal(l_a, l_b), (t, l_a.item(), l_b.item())
        assert o_a.step_count == o_b.step_count == t + 1
        _assert_same_run(t, m_a, o_a, m_b, o_b)
        # the fused step keeps its staging valid; step_prep agrees with it
        assert o_a._stage_key == o_a._key(o_a._params())
        for n, a, w in zip(STAGE_NAMES, o_a._staged,
                           hip.step_prep(
                               [p.detach() for p in o_a._params()[:4]])):
            assert torch.equal(a.view(torch.int16), w.view(torch.int16)), (
                t, n)
        losses.append(l_a.item())
    print(f"M={m_rows} {loss} {kind} losses {losses}")
    assert all(not torch.equal(p, s)
               for p, s in zip(m_a.parameters(), start))
    assert losses[2] < losses[0], losses


def test_fused_step_with_optimizer_flat_grads(dev, hip):
    """Flat-grad mode in a world of one takes the fused path and writes
    the gradients into the pre-created views."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from test_step_glue_gpu import _flat_grad_views

    m_a, o_a = _model_and_opt(dev, "sgd", 7)
    m_b, o_b = _twin(m_a, o_a)
    flat = _flat_grad_views(m_a, dev)
    flat.fill_(float("nan"))
    ptrs = [p.grad.data_ptr() for p in m_a.parameters()]
    x, y = _batch(dev, 33, "mse", torch.float32, 3)
    for t in range(2):
        l_a = fused_step(m_a, x, y, optimizer=o_a)
        l_b = fused_step(m_b, x, y)
        o_b.step()
        assert torch.equal(l_a, l_b)
        _assert_same_run(t, m_a, o_a, m_b, o_b)
    assert [p.grad.data_ptr() for p in m_a.parameters()] == ptrs
    assert torch.isfinite(flat).all()


def test_stale_staging_is_not_used(dev, hip):
    """A weight changed behind the optimizer's back: the key mismatches
    and the next step restages through step_prep."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step

    m_a, o_a = _model_and_opt(dev, "sgd", 21)
    x, y = _batch(dev, 33, "mse", torch.float32, 5)
    for _ in range(2):
        fused_step(m_a, x, y, optimizer=o_a)
    m_old, o_old = _twin(m_a, o_a)  # what a stale staging would compute
    with torch.no_grad():
        o_a._params()[1].mul_(0.5)
    assert o_a._stage_key != o_a._key(o_a._params())
    m_ref, o_ref = _twin(m_a, o_a)  # fresh optimizer, state copied
    assert o_ref._stage_key is None
    l_a = fused_step(m_a, x, y, optimizer=o_a)
    l_ref = fused_step(m_ref, x, y, optimizer=o_ref)
    l_old = fused_step(m_old, x, y, optimizer=o_old)
    assert torch.equal(l_a, l_ref)
    assert not torch.equal(l_a, l_old)
    _assert_same_run("restaged", m_a, o_a, m_ref, o_ref)
    assert o_a._stage_key == o_a._key(o_a._params())
    # a replaced tensor is seen too
    lin = o_a._lin[2]
    lin.weight = torch.nn.Parameter(lin.weight.detach() * 2.0)
    assert o_a._stage_key != o_a._key(o_a._params())
    m_ref, o_ref = _twin(m_a, o_a)
    assert torch.equal(fused_step(m_a, x, y, optimizer=o_a),
                       fused_step(m_ref, x, y, optimizer=o_ref))
    _assert_same_run("replaced", m_a, o_a, m_ref, o_ref)


def test_evaluator_sees_the_fused_update(dev, hip):
    from ray_shuffling_data_loader_amd.models.fused_eval import (
        FusedEvaluator,
    )
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step

    model, opt = _model_and_opt(dev, "adamw", 31)
    x, y = _batch(dev, 4097, "mse", torch.float32, 9)
    ev = FusedEvaluator(model)
    ev.update(x, y)
    before = ev.state()
    fused_step(model, x, y, optimizer=opt)
    ev.reset()
    ev.update(x, y)
    after = ev.state()
    fresh = FusedEvaluator(model)
    fresh.update(x, y)
    assert not torch.equal(after, before)
    assert torch.equal(after.view(torch.int64),
                       fresh.state().view(torch.int64))


def _device_kernels(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(
        activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]
    ) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()
             if e.device_type == DeviceType.CUDA]
    copies = [n for n in names
              if "memcpy" in n.lower() or "memset" in n.lower()]
    return [n for n in names if n not in copies], copies


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fused_optimizer_launch_count(dev, hip, kind):
    """Warmed, fp32 target: a step with optimizer= launches no step_prep,
    exactly one step_finalize* kernel, no memcpy or memset, and at least
    one kernel fewer than a plain step (which has no optimizer at all)."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step

    M = 8215
    model, opt = _model_and_opt(dev, kind, 8)
    plain = copy.deepcopy(model)
    x, y = _batch(dev, M, "mse", torch.float32, 8)
    for _ in range(3):
        fused_step(plain, x, y)
        fused_step(model, x, y, optimizer=opt)
    k0, c0 = _device_kernels(lambda: fused_step(plain, x, y))
    k1, c1 = _device_kernels(lambda: fused_step(model, x, y, optimizer=opt))
    print("plain:", k0)
    print("optimizer=:", k1)
    assert c0 == [] and c1 == [], (c0, c1)
    assert any("step_prep" in n for n in k0), k0
    assert not any("step_prep" in n for n in k1), k1
    assert sum("step_finalize" in n for n in k1) == 1, k1
    assert any("step_finalize_update" in n for n in k1), k1
    assert 1 <= len(k1) <= len(k0) - 1, (k0, k1)
