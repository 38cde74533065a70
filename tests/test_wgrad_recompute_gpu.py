"""GPU tests of the dW2 wgrad that recomputes a1 (csrc/wgrad_frag.hip,
wgrad_rc_body) and of the forward chain that then emits no a1^T
(csrc/fwd_chain.hip, fwd_chain_kernel<.., EMIT_A1 = false>).

Everything here is an identity of bits: the recompute runs the forward's
own MFMAs and epilogue on the forward's own inputs, and the wgrad's
accumulators see the same products in the same chunk order, so partials,
gradients, parameters and optimizer state are compared with torch.equal,
never within a tolerance. The integer-valued cases of tests/_exact_cases.py
are in addition compared with an fp64 oracle per slab: |dz| <= 2 and a slab
of at most 18 chunks keep every sum of magnitudes under 2^24 (asserted), so
each fp32 partial is exact in any order."""

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _exact_cases import REGIMES, int_matrix, make_case  # noqa: E402

pytestmark = pytest.mark.gpu

# M -> mchunks = 2 * ceil(M / 32). 1: one partly filled tile; 33: the second
# tile almost all padding; 65: the last 64-row workgroup of the forward has
# no second m-tile; 1, 33, 65, 97: one chunk per slab, so every slab starts
# or ends inside a pair; 2049: two chunks per slab; 8215 and 20000: 8 and 18
# chunks per slab, the steady loop (the shapes of the grouped tests).
SHAPES = [1, 33, 65, 97, 2049, 8215, 20000]


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    h = _load_hip()
    assert hasattr(h, "wgrad_recompute_partials_bf16")
    return h


def _mchunks(m):
    return 2 * ((m + 31) // 32)


def _bits(t):
    """Floating tensors as their bit patterns: -0 != +0, NaN == NaN."""
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t


def _k_frag(t):
    """[R, 112] (R a multiple of 32) -> the forward's fragment-major layout
    [R/32][7][2][32][8], flat: x blocks and the swizzled W1 alike."""
    r = t.shape[0]
    return (t.view(r // 32, 32, 7, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
            .view(-1))


def _pad(t, rows):
    out = torch.zeros(rows, 112, dtype=t.dtype, device=t.device)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def _inputs(kind, m):
    """(x [m,100] bf16, W1 [512,100] bf16, b1 [512] fp32, dz2 [m,256] bf16)
    on the CPU."""
    if kind == "normal":
        g = torch.Generator(device="cpu").manual_seed(4000 + m)
        x = torch.randn(m, 100, generator=g).bfloat16()
        w1 = (0.1 * torch.randn(512, 100, generator=g)).bfloat16()
        # positive, negative and zero biases: the padded rows then carry
        # relu(b1) != 0 against dz = 0
        b1 = torch.randn(512, generator=g)
        b1[::3] = 0.0
        assert (b1 > 0).any() and (b1 < 0).any() and (b1 == 0).any()
        dz = torch.randn(m, 256, generator=g).bfloat16()
        return x, w1, b1, dz
    # The regime's W1 and b1 (they depend on the regime alone) and x drawn
    # in the regime's range: make_case itself also pins the head, which
    # holds up to its own 161 rows only.
    case = make_case(kind, 1)
    x = int_matrix(m, 100, 9000 + m, REGIMES[kind]["x"])
    return x, case["W1"], case["b1"], int_matrix(m, 256, 9100 + m, 2)


@functools.lru_cache(maxsize=None)
def _run(kind, m):
    """(recomputed partials, the present path's partials, a1 [Mp,512] as the
    forward emitted it, dz2 [Mp,256]); Mp = 16 * mchunks. Read-only."""
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
        _load_hip,
        t_frag_swizzle,
        t_frag_unswizzle,
    )

    hip = _load_hip()
    dev = torch.device("cuda", 0)
    mchunks = _mchunks(m)
    mp = 16 * mchunks
    x, w1, b1, dz = _inputs(kind, m)
    x, w1, b1 = x.to(dev), w1.to(dev), b1.to(dev)
    dzp = torch.zeros(mp, 256, dtype=torch.bfloat16, device=dev)
    dzp[:m] = dz.to(dev)
    dz2t = t_frag_swizzle(dzp)
    bf = dict(dtype=torch.bfloat16, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    # The present path: the forward's emitted a1^T into the grouped kernel.
    # Layers 2 and 3 and the other two wgrads run on zeros.
    a1t = hip.fwd_chain_bf16(
        x, w1, b1, torch.zeros(256, 512, **bf), torch.zeros(256, **f32),
        torch.zeros(128, 256, **bf), torch.zeros(128, **f32),
        torch.zeros(128, **bf), torch.zeros(1, **f32), rows=64)[0]
    assert a1t.numel() == 16 * mchunks * 512
    old = hip.wgrad_grouped_partials_bf16(
        torch.zeros(16 * mchunks * 512, **bf),
        torch.zeros(4 * mchunks * 512, **bf), dz2t, a1t,
        torch.zeros(4 * mchunks * 512, **bf),
        torch.zeros(8 * mchunks * 512, **bf), mchunks)[1]
    new = hip.wgrad_recompute_partials_bf16(
        _k_frag(_pad(x, mp)), _k_frag(_pad(w1, 512)), b1, dz2t, mchunks)
    torch.cuda.synchronize()
    return new, old, t_frag_unswizzle(a1t, mp, 512), dzp


@pytest.mark.parametrize("m", SHAPES)
@pytest.mark.parametrize("kind", ["small", "wide", "normal"])
def test_partials_bit_for_bit(hip, kind, m):
    new, old, a1, dz = _run(kind, m)
    mchunks = _mchunks(m)
    assert new.dtype == torch.float32 and new.shape == old.shape
    ns = new.shape[0]
    cps = -(-mchunks // ns)
    assert ns == -(-mchunks // cps) and new.shape[1] == 256 * 512
    bad = (new != old).sum().item()
    print(f"{kind} M={m}: {ns} slabs of {cps} chunks, {bad} differing")
    assert torch.equal(new, old), (kind, m, ns, cps, bad)
    if kind == "normal":
        return
    # The integer cases: both must also be the exact per-slab products.
    rows = ns * cps * 16
    a = torch.zeros(rows, 256, dtype=torch.float64, device=dz.device)
    b = torch.zeros(rows, 512, dtype=torch.float64, device=dz.device)
    a[:dz.shape[0]] = dz.double()
    b[:a1.shape[0]] = a1.double()
    a = a.view(ns, cps * 16, 256)
    b = b.view(ns, cps * 16, 512)
    bound = torch.bmm(a.abs().transpose(1, 2), b.abs()).max().item()
    assert bound < 2 ** 24, (kind, m, bound)
    ref = torch.bmm(a.transpose(1, 2), b).reshape(ns, 256 * 512)
    assert ref.abs().max().item() > 0
    assert torch.equal(new.double(), ref), (
        kind, m, (new.double() != ref).sum().item())


def test_recompute_inputs_checked(hip):
    new, _, _, _ = _run("small", 97)
    dev = new.device
    bf = dict(dtype=torch.bfloat16, device=dev)
    good = [torch.zeros(4 * 7 * 512, **bf), torch.zeros(512 * 112, **bf),
            torch.zeros(512, device=dev), torch.zeros(8 * 8 * 512, **bf)]
    assert hip.wgrad_recompute_partials_bf16(*good, 8).shape == new.shape
    with pytest.raises(RuntimeError, match="mchunks"):
        hip.wgrad_recompute_partials_bf16(*good, 0)
    with pytest.raises(RuntimeError, match="mchunks"):
        hip.wgrad_recompute_partials_bf16(*good, 7)
    with pytest.raises(RuntimeError, match="xs"):
        hip.wgrad_recompute_partials_bf16(good[0][:-512], *good[1:], 8)
    with pytest.raises(RuntimeError, match="dz2t"):
        hip.wgrad_recompute_partials_bf16(*good, 10)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("m", [1, 65, 4097])
def test_forward_without_emission(hip, m, loss, weighted):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(500 + m)
    model = [(0.1 * torch.randn(n, k, generator=g)).bfloat16().to(dev)
             for n, k in ((512, 100), (256, 512), (128, 256))]
    biases = [(0.1 * torch.randn(n, generator=g)).to(dev)
              for n in (512, 256, 128, 1)]
    w4 = (0.1 * torch.randn(128, generator=g)).bfloat16().to(dev)
    x = torch.randn(m, 100, generator=g).bfloat16().to(dev)
    t = torch.rand(m, generator=g).to(dev)
    kw = dict(target=t, rows=64, loss=loss)
    if weighted:
        kw["weight"] = (2.0 * torch.rand(m, generator=g)).to(dev)
        if loss == 1:
            kw["pos_weight"] = 1.5
    args = (x, model[0], biases[0], model[1], biases[1], model[2], biases[2],
            w4, biases[3])
    emit = hip.fwd_chain_bf16(*args, **kw)
    quiet = hip.fwd_chain_bf16(*args, emit_a1=False, **kw)
    assert len(emit) == len(quiet) == 8
    assert emit[0].numel() == 16 * _mchunks(m) * 512
    assert quiet[0].numel() == 0
    names = ["a1t", "mask1", "a2t", "mask2", "a3", "out", "dyb", "loss_part"]
    for n, a, b in zip(names[1:], emit[1:], quiet[1:]):
        assert a.shape == b.shape and a.dtype == b.dtype, n
        assert torch.equal(_bits(a), _bits(b)), (m, loss, weighted, n)
    with pytest.raises(RuntimeError, match="emit_a1"):
        hip.fwd_chain_bf16(*args, emit_a1=False, target=t, rows=32)
    with pytest.raises(RuntimeError, match="emit_a1"):
        hip.fwd_chain_bf16(*args, emit_a1=False, target=t, rows=64,
                           pi16=True)




@pytest.mark.parametrize("m", [33, 4097])
def test_whole_step_recompute_on_off(hip, monkeypatch, m):
    """fused_step with the recompute pair on, off and on again: the loss and
    all eight gradients bit for bit; then the fallbacks, on which the knob
    has no effect."""
    from ray_shuffling_data_loader_amd.models import fused_step as fs
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    dev = torch.device("cuda", 0)
    torch.manual_seed(23)
    model = TabularMLP(100).to(dev)
    x = torch.randn(m, 100, device=dev).bfloat16()
    t = torch.randn(m, 1, device=dev)
    monkeypatch.setattr(fs, "_NATIVE_GLUE", True)
    monkeypatch.setattr(fs, "_WGRAD_VARIANT", 0)
    monkeypatch.setattr(fs, "_WGRAD_GROUPED", None)
    monkeypatch.setattr(fs, "_PI16", False)
    monkeypatch.setattr(fs, "_CHAIN_ROWS", 64)
    lin = fs._layers(model)
    assert fs._native_ok(hip, lin, x, t, None)

    def run(recompute):
        monkeypatch.setattr(fs, "_WGRAD_RECOMPUTE", recompute)
        for p in model.parameters():
            p.grad = None
        loss = fs.fused_step(model, x, t)
        return ([loss.clone()] + [q.weight.grad.clone() for q in lin]
                + [q.bias.grad.clone() for q in lin])

    on, off, on2 = run(True), run(False), run(True)
    assert len(on) == 9
    for i, (a, b, c) in enumerate(zip(on, off, on2)):
        assert torch.equal(_bits(a), _bits(b)), (m, i, "on/off")
        assert torch.equal(_bits(a), _bits(c)), (m, i, "on/on")
    assert all(torch.isfinite(a).all() for a in on)
    assert on[2].abs().max().item() > 0

    # Fallbacks: each runs, and the knob changes nothing there.
    for name, value in (("_WGRAD_GROUPED", False), ("_WGRAD_VARIANT", 2),
                        ("_PI16", True), ("_CHAIN_ROWS", 32)):
        with monkeypatch.context() as mp:
            mp.setattr(fs, name, value)
            a, b = run(True), run(False)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(_bits(u), _bits(v)), (m, name, i)
            assert torch.isfinite(u).all(), (m, name, i)
        # everything the partition of the wgrad sums cannot touch is the
        # default path's (the slab size regroups the loss and db partials)
        if name in ("_WGRAD_GROUPED", "_WGRAD_VARIANT"):
            for i in (0, 4, 5, 6, 7, 8):  # loss, dW4, db1-db4
                assert torch.equal(_bits(a[i]), _bits(on[i])), (m, name, i)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("m", [33, 4097])
def test_whole_step_with_optimizer(hip, monkeypatch, m, kind):
    """With optimizer=: loss, gradients, parameters and optimizer state of
    two steps, bit for bit across on / off / on."""
    from ray_shuffling_data_loader_amd.models import fused_step as fs
    from ray_shuffling_data_loader_amd.models.fused_optim import (
        FusedOptimizer,
    )
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    dev = torch.device("cuda", 0)
    hyper = {"sgd": {"lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-4},
             "adamw": {"lr": 1e-3, "weight_decay": 1e-2}}[kind]
    g = torch.Generator(device=dev).manual_seed(m)
    x = torch.randn(m, 100, device=dev, generator=g).bfloat16()
    t = torch.randn(m, 1, device=dev, generator=g)
    monkeypatch.setattr(fs, "_NATIVE_GLUE", True)
    monkeypatch.setattr(fs, "_WGRAD_VARIANT", 0)
    monkeypatch.setattr(fs, "_WGRAD_GROUPED", None)
    monkeypatch.setattr(fs, "_PI16", False)
    monkeypatch.setattr(fs, "_CHAIN_ROWS", 64)

    def run(recompute):
        monkeypatch.setattr(fs, "_WGRAD_RECOMPUTE", recompute)
        torch.manual_seed(31)
        model = TabularMLP(100).to(dev)
        opt = FusedOptimizer(model, kind, **hyper)
        got = []
        for _ in range(2):
            got.append(fs.fused_step(model, x, t, optimizer=opt).clone())
        for n, p in model.named_parameters():
            got += [p.grad.clone(), p.detach().clone()]
            got += [opt.state[n][s].clone() for s in sorted(opt.state[n])]
        return got

    on, off, on2 = run(True), run(False), run(True)
    assert len(on) == len(off) == len(on2) > 2 + 16
    for i, (a, b, c) in enumerate(zip(on, off, on2)):
        assert torch.equal(_bits(a), _bits(b)), (m, kind, i, "on/off")
        assert torch.equal(_bits(a), _bits(c)), (m, kind, i, "on/on")
