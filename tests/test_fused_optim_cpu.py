"""FusedOptimizer (models/fused_optim.py) on CPU: the unfused torch-op form
of the update against the numpy oracle of tests/_optim_cases.py, bit for
bit; ``fused_step(optimizer=)`` through the FakeHip stand-in; checkpoint
round trip; refusals; and the distance to torch.optim on fp64.

Bound against torch.optim. ``torch.optim.SGD`` / ``AdamW`` on fp64 copies,
fed the same fp32 gradients for 5 steps, is the reference. torch's own fp32
CPU optimizer (``foreach=False``) on the same inputs shows what fp32
rounding costs: its maximum parameter error e_t. Ours is a second fp32
formulation of the same mathematics that orders its operations differently
(``m + a1*(g - m)`` for ``lerp``, a divide for ``addcdiv``), so its
maximum error must stay within 4 * e_t. Both are printed.
"""

import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _optim_cases as oc  # noqa: E402

STEPS = 5
LRS = [1e-2, 1e-2, 5e-3, 2.5e-3, 1e-3]  # changed between steps


def _model(seed=3):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    return TabularMLP(100)


@pytest.fixture()
def fake(monkeypatch):
    """fused_step / FusedOptimizer with FakeHip as the extension."""
    from _fake_hip import FakeHip
    import ray_shuffling_data_loader_amd.ops.shuffle_ops as so

    monkeypatch.setattr(so, "_load_hip", lambda: FakeHip)
    from ray_shuffling_data_loader_amd.models import fused_optim, fused_step

    return fused_step, fused_optim


def _grads(seed):
    g = torch.Generator().manual_seed(seed)
    return [
        [torch.randn(s, generator=g) for s in oc.SHAPES]
        for _ in range(STEPS)
    ]


def _assert_bits(got, want, tag):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (
        tag, float(np.abs(got - want).max()))


CONFIGS = [
    ("sgd", {}),
    ("sgd", {"momentum": 0.9}),
    ("sgd", {"momentum": 0.9, "nesterov": True}),
    ("sgd", {"weight_decay": 1e-2}),
    ("sgd", {"momentum": 0.9, "nesterov": True, "weight_decay": 1e-2}),
    ("adamw", {}),
    ("adamw", {"weight_decay": 1e-2, "betas": (0.8, 0.99), "eps": 1e-6}),
]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("kind,kw", CONFIGS)
def test_torch_fallback_equals_oracle(fake, kind, kw, grad_scale):
    _, fo = fake
    model = _model()
    opt = fo.FusedOptimizer(model, kind, lr=LRS[0], **kw)
    params = opt._params()
    ora = oc.Oracle(kind, [p.detach().numpy() for p in params], **kw)
    slots = {"sgd": ["momentum_buffer"], "adamw": ["exp_avg", "exp_avg_sq"]}
    for t, grads in enumerate(_grads(11)):
        opt.lr = LRS[t]
        for p, g in zip(params, grads):
            p.grad = g
        opt.zero_grad()
        assert all(p.grad is g for p, g in zip(params, grads))
        opt.step(grad_scale=grad_scale)
        ora.step([g.numpy() for g in grads], LRS[t], grad_scale)
        assert opt.step_count == ora.t == t + 1
        for i, (n, p) in enumerate(zip(opt._names, params)):
            _assert_bits(p, ora.p[i], (t, n))
            st = opt.state[n]
            if kind == "sgd" and not kw.get("momentum"):
                assert st == {}
                continue
            assert list(st) == slots[kind]
            for s, want in zip(slots[kind], (ora.s1[i], ora.s2[i])):
                _assert_bits(st[s], want, (t, n, s))


def _data(M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, 100, generator=g).bfloat16(),
            torch.randn(M, 1, generator=g))


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fused_step_with_optimizer_is_step_then_update(fake, kind):
    fs, fo = fake
    kw = {"momentum": 0.9} if kind == "sgd" else {"weight_decay": 1e-2}
    m_a = _model(5)
    m_b = copy.deepcopy(m_a)
    o_a = fo.FusedOptimizer(m_a, kind, lr=1e-2, **kw)
    o_b = fo.FusedOptimizer(m_b, kind, lr=1e-2, **kw)
    for t in range(2):
        x, y = _data(33, 20 + t)
        l_a = fs.fused_step(m_a, x, y, optimizer=o_a)
        l_b = fs.fused_step(m_b, x, y)
        grads_b = [p.grad.clone() for p in m_b.parameters()]
        before = [p.detach().clone() for p in m_b.parameters()]
        o_b.step()
        assert torch.equal(l_a, l_b)
        assert o_a.step_count == o_b.step_count == t + 1
        for (n, p), q, g, b in zip(m_a.named_parameters(),
                                   m_b.parameters(), grads_b, before):
            assert torch.equal(p.grad, g), (t, n)
            assert torch.equal(p, q), (t, n)
            assert not torch.equal(q, b), (t, n)
            for s in o_a.state[n]:
                assert torch.equal(o_a.state[n][s], o_b.state[n][s]), (t, n)


def test_optimizer_none_changes_nothing(fake):
    fs, _ = fake
    m_a = _model(6)
    m_b = copy.deepcopy(m_a)
    x, y = _data(33, 30)
    assert torch.equal(fs.fused_step(m_a, x, y, optimizer=None),
                       fs.fused_step(m_b, x, y))
    for p, q in zip(m_a.parameters(), m_b.parameters()):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_round_trip_resumes_exactly(fake, kind):
    _, fo = fake
    kw = ({"momentum": 0.9, "weight_decay": 1e-3} if kind == "sgd"
          else {"weight_decay": 1e-2})
    grads = _grads(13)
    model = _model(7)
    opt = fo.FusedOptimizer(model, kind, lr=1e-2, **kw)

    def run(o, t):
        for p, g in zip(o._params(), grads[t]):
            p.grad = g
        o.step()

    for t in range(3):
        run(opt, t)
    sd = copy.deepcopy(opt.state_dict())
    weights = copy.deepcopy(model.state_dict())
    assert sd["kind"] == kind and sd["step"] == 3
    assert sorted(sd["state"]) == sorted(n for n, _ in
                                         model.named_parameters())
    run(opt, 3)
    # the saved copy is not the live state
    n0 = opt._names[0]
    s0 = next(iter(sd["state"][n0]))
    assert not torch.equal(sd["state"][n0][s0], opt.state[n0][s0])
    # resume in a differently initialised model with other hyper-parameters
    m2 = _model(99)
    m2.load_state_dict(weights)
    o2 = fo.FusedOptimizer(m2, "sgd", lr=0.5)
    o2._stage_key = "stale"
    o2.load_state_dict(sd)
    assert o2._stage_key is None
    assert (o2.kind, o2.step_count, o2.lr) == (kind, 3, 1e-2)
    for n in sd["state"]:
        for s, t in sd["state"][n].items():
            assert torch.equal(o2.state[n][s], t)
            assert o2.state[n][s].data_ptr() != t.data_ptr()
    run(o2, 3)
    for (n, p), q in zip(model.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), n
        for s in opt.state[n]:
            assert torch.equal(opt.state[n][s], o2.state[n][s]), (n, s)


def test_refusals_come_before_any_change(fake):
    _, fo = fake
    model = _model(8)
    before = copy.deepcopy(model.state_dict())
    with pytest.raises(ValueError, match="kind"):
        fo.FusedOptimizer(model, "adam", lr=1e-2)
    with pytest.raises(ValueError, match="lr"):
        fo.FusedOptimizer(model, "sgd", lr=-1e-2)
    with pytest.raises(ValueError, match="nesterov"):
        fo.FusedOptimizer(model, "sgd", lr=1e-2, nesterov=True)
    with pytest.raises(ValueError, match="betas"):
        fo.FusedOptimizer(model, "adamw", lr=1e-2, betas=(0.9, 1.0))
    other = torch.nn.Sequential(torch.nn.Linear(100, 64), torch.nn.ReLU(),
                                torch.nn.Linear(64, 1))
    with pytest.raises(ValueError, match="stock TabularMLP"):
        fo.FusedOptimizer(other, "sgd", lr=1e-2)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k])
    assert not hasattr(model, "_fused_buf")
    # a state_dict that does not fit is refused whole
    opt = fo.FusedOptimizer(model, "adamw", lr=1e-2)
    sd = opt.state_dict()
    sd["hyper"]["lr"] = -1.0
    with pytest.raises(ValueError, match="lr"):
        opt.load_state_dict(sd)
    sd = opt.state_dict()
    sd["state"].pop(opt._names[0])
    sd["step"] = 17
    with pytest.raises(ValueError, match="names"):
        opt.load_state_dict(sd)
    assert opt.step_count == 0 and opt.lr == 1e-2
    # a step without gradients says so
    with pytest.raises(RuntimeError, match="no .grad"):
        opt.step()
    # an optimizer of another model
    fs = fake[0]
    x, y = _data(4, 1)
    with pytest.raises(ValueError, match="another model"):
        fs.fused_step(_model(9), x, y, optimizer=opt)


@pytest.mark.parametrize(
    "kind,kw",
    [
        ("sgd", {"momentum": 0.9, "weight_decay": 1e-2}),
        ("sgd", {"momentum": 0.9, "nesterov": True}),
        ("adamw", {"weight_decay": 1e-2}),
        ("adamw", {"weight_decay": 0.0}),
    ],
)
def test_error_against_fp64_torch_optim(fake, kind, kw):
    _, fo = fake
    model = _model(10)
    opt = fo.FusedOptimizer(model, kind, lr=1e-2, **kw)
    params = list(model.parameters())
    p64 = [p.detach().double().clone() for p in params]
    p32 = [p.detach().clone() for p in params]
    cls = torch.optim.SGD if kind == "sgd" else torch.optim.AdamW
    t64 = cls(p64, lr=1e-2, foreach=False, **kw)
    t32 = cls(p32, lr=1e-2, foreach=False, **kw)
    g = torch.Generator().manual_seed(17)
    for _ in range(STEPS):
        for p, a, b in zip(params, p64, p32):
            p.grad = torch.randn(p.shape, generator=g)
            a.grad = p.grad.double()
            b.grad = p.grad.clone()
        opt.step()
        t64.step()
        t32.step()
    e_ours = max((p.detach().double() - a).abs().max().item()
                 for p, a in zip(params, p64))
    e_torch = max((b.double() - a).abs().max().item()
                  for b, a in zip(p32, p64))
    print(f"{kind} {kw}: max |p - p64| ours {e_ours:.3e} "
          f"torch fp32 {e_torch:.3e}")
    assert e_torch > 0.0
    assert e_ours <= 4.0 * e_torch, (e_ours, e_torch)
