"""GPU tests of sample weights and pos_weight: the WEIGHTED heads of
fwd_chain_kernel and eval_chain_kernel (csrc/fwd_chain.hip), the wider
eval_accumulate (csrc/step_glue.hip), their bindings,
``fused_step(sample_weight=, pos_weight=)`` and
``FusedEvaluator(weighted=True)``.

Shapes, data and every bound are those of tests/test_fused_bce_gpu.py (a
single row, a partial and a full first m-tile, a partial and a full second
m-tile, an odd tile count whose last 64-row workgroup has no second
m-tile; both slab sizes), plus per-row weights: multiples of 1/16 in
[0, 4] with exact zeros.

Bounds.
  loss_part / the evaluator's weighted logloss and brier sums: rel 2e-5
    against fp64 on the kernel's own fp32 logits (the weight adds one
    rounding per term to that file's budget).
  dyb: one bf16 ulp (2^-8 relative) around bf16 of the fp64 value; rows
    with w = 0 exactly 0.
  sums of w, w t and w correct for 0/1 targets, and the fixed-point
    histogram: exact (multiples of 1/16, at most 64 per slab).
  weighted regression metrics: 1e-5 |ref| + 1e-5
    (tests/test_fused_eval_gpu.py::_check_metrics).
  whole step against eager autocast, native against composed: the
    expressions of test_bce_step_edge_batch_sizes,
    test_bce_step_matches_eager_4097 and
    test_bce_native_step_matches_composed.
"""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [1, 31, 32, 33, 64, 65, 97]
ROWS = (32, 64)
M_MAX = max(SHAPES)
BATCHES = [97, 64, 1]
REL = 2e-5
BF16_ULP = 2.0 ** -8
FP32_TINY = float(torch.finfo(torch.float32).tiny)
POS_WEIGHT = 3.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    return shuffle_ops._load_hip()


def _model_from(Wb, bs, dev):
    """The stock TabularMLP holding the given (bf16-exact) weights."""
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    model = TabularMLP(100).to(dev)
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, W, b in zip(lin, Wb, bs):
            m.weight.copy_(W.float().view_as(m.weight))
            m.bias.copy_(b.view_as(m.bias))
    return model


def _weights(n, g):
    """Multiples of 1/16 in [0, 4]; every fifth row from row 3 exactly 0."""
    w = torch.randint(1, 65, (n,), generator=g).float() / 16.0
    w[3::5] = 0.0
    return w


@pytest.fixture(scope="module")
def data(dev):
    """The fixture of tests/test_fused_bce_gpu.py (same seed, same draws
    in the same order), then regression targets and the weights."""
    g = torch.Generator(device="cpu").manual_seed(65)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    Wb = [
        (rn(512, 100) / 10).bfloat16(),
        (rn(256, 512) / 22).bfloat16(),
        (rn(128, 256) / 16).bfloat16(),
        (rn(1, 128) / 11).bfloat16(),
    ]
    bs = [(rn(n) / 4).bfloat16().float() for n in (512, 256, 128, 1)]
    soft = torch.rand(M_MAX, generator=g).to(dev)
    hard = (soft >= 0.5).float()
    even = (torch.arange(M_MAX, device=dev) % 2) == 0
    x = rn(M_MAX, 100).bfloat16()
    return {
        "Wb": Wb,
        "bs": bs,
        "x": x,
        "tgt": torch.where(even, hard, soft),
        "hard": hard,
        "reg": rn(M_MAX),
        "w": _weights(M_MAX, g).to(dev),
    }


def _fwd(hip, data, bs, M, rows, tgt, loss, **kw):
    Wb = data["Wb"]
    return hip.fwd_chain_bf16(
        data["x"][:M].contiguous(), Wb[0], bs[0], Wb[1], bs[1], Wb[2],
        bs[2], Wb[3].flatten(), bs[3], target=tgt, rows=rows, loss=loss,
        **kw,
    )


def _ref_head(o, t, w, loss, p):
    """fp64 (per-row loss term, dl/do) of fp32 logits, fp32 targets and
    fp32 weights; both already scaled by w."""
    o = o.reshape(-1).double()
    t = t.reshape(-1).float().double()
    w = w.reshape(-1).float().double()
    if loss == 0:
        d = o - t
        return w * d * d, 2.0 * w * d
    e = torch.exp(-o.abs())
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sg = torch.where(o >= 0, big, small)
    cs = torch.where(o >= 0, small, big)
    lp = torch.log1p(e)
    ll = (p * t * (torch.clamp(-o, min=0.0) + lp)
          + (1.0 - t) * (torch.clamp(o, min=0.0) + lp))
    return w * ll, w * ((1.0 - t) * sg - p * t * cs)


def _slab_sums(v, rows):
    n = v.numel()
    nwg = (n + rows - 1) // rows
    return torch.nn.functional.pad(v, (0, nwg * rows - n)).view(
        nwg, rows).sum(1)


def _bits(a):
    return a.view(torch.int16) if a.dtype == torch.bfloat16 else a


def _check_head(hip, data, dev, bs, M, rows, tgt, w, loss, p, tag):
    """The weighted head of fwd_chain_bf16 against fp64 on the logits of
    FusedEvaluator.predict (bit-equal to the training head's)."""
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    fw = _fwd(hip, data, bs, M, rows, tgt, loss, weight=w, pos_weight=p)
    f0 = _fwd(hip, data, bs, M, rows, tgt, loss)
    assert len(fw) == 8 and len(f0) == 8
    # the weights must not reach the layers
    for i, nm in enumerate(["a1t", "mask1", "a2t", "mask2", "a3", "out"]):
        assert torch.equal(_bits(fw[i]), _bits(f0[i])), (tag, nm)
    model = _model_from(data["Wb"], bs, dev)
    o = fe.FusedEvaluator(model, rows=rows).predict(
        data["x"][:M].contiguous()).reshape(-1)
    assert torch.equal(o.bfloat16(), fw[5].flatten()), tag
    wv = w if w is not None else torch.ones(M, device=dev)
    terms, grad = _ref_head(o, tgt, wv, loss, p)
    ref_lp = _slab_sums(terms, rows)
    lp = fw[7]
    assert lp.shape == ref_lp.shape and lp.dtype == torch.float32
    assert bool(torch.isfinite(lp).all()), (tag, lp)
    err_lp = (lp.double() - ref_lp).abs()
    rel = (err_lp / ref_lp.abs().clamp(min=FP32_TINY)).max().item()
    print(f"{tag}: loss_part max rel err {rel:.3e} (bound {REL:.0e})")
    assert bool((err_lp <= REL * ref_lp.abs() + FP32_TINY).all()), (
        tag, lp, ref_lp)
    ref_d = (grad / M).float().bfloat16().float()
    dyb = fw[6].flatten().float()
    assert bool(torch.isfinite(dyb).all()), tag
    err = (dyb - ref_d).abs()
    print(f"{tag}: dyb max err {err.max().item():.3e}")
    assert bool((err <= BF16_ULP * ref_d.abs()).all()), (tag, dyb, ref_d)
    zero = wv == 0
    assert bool((dyb[zero] == 0).all()), tag
    return fw, f0, o, dyb


# 1. the head in isolation
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("loss,p", [(0, 1.0), (1, 1.0), (1, POS_WEIGHT)])
@pytest.mark.parametrize("M", SHAPES)
def test_weighted_head_in_isolation(hip, data, dev, M, rows, loss, p):
    tgt = (data["reg"] if loss == 0 else data["tgt"])[:M].contiguous()
    w = data["w"][:M].contiguous()
    tag = f"M={M} rows={rows} loss={loss} p={p}"
    fw, f0, _, _ = _check_head(hip, data, dev, data["bs"], M, rows, tgt, w,
                               loss, p, tag)
    if M > 1:
        assert not torch.equal(fw[7], f0[7])
    # unit weights and pos_weight 1 through the WEIGHTED kernel: the
    # unweighted bits
    ones = torch.ones(M, device=dev)
    f1 = _fwd(hip, data, data["bs"], M, rows, tgt, loss, weight=ones,
              pos_weight=1.0)
    assert torch.equal(_bits(f1[6]), _bits(f0[6])), tag
    assert torch.equal(f1[7], f0[7]), tag
    if loss == 1 and p != 1.0:
        # pos_weight alone (no weight tensor: every w = 1)
        _check_head(hip, data, dev, data["bs"], M, rows, tgt, None, loss, p,
                    tag + " no weight")


# 2. saturated logits
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("b4", [200.0, -200.0])
@pytest.mark.parametrize("M", [1, 33, 97])
def test_weighted_head_saturation(hip, data, dev, M, rows, b4):
    bs = list(data["bs"][:3]) + [torch.tensor([b4], device=dev)]
    tgt = data["hard"][:M].contiguous()
    w = data["w"][:M].contiguous()
    if M > 1:
        assert 0 < tgt.sum().item() < M  # 0 and 1 mixed
    fw, _, o, dyb = _check_head(
        hip, data, dev, bs, M, rows, tgt, w, 1, POS_WEIGHT,
        f"M={M} rows={rows} b4={b4}")
    assert bool((o.abs() > 150).all())
    assert bool(torch.isfinite(fw[7]).all())
    # dyb is +w/M (negatives, o >> 0), -p w/M (positives, o << 0) or 0
    if b4 > 0:
        want = torch.where(tgt == 0, w / M, torch.zeros_like(w))
    else:
        want = torch.where(tgt == 1, -POS_WEIGHT * w / M,
                           torch.zeros_like(w))
    want = want.bfloat16().float()
    assert bool(((dyb - want).abs() <= BF16_ULP * want.abs()).all()), (
        dyb, want)


# 3. the whole step against eager autocast
def _eager(ref, x, t, w, loss, p):
    with torch.autocast("cuda", torch.bfloat16):
        out = ref(x)
    if loss == "bce":
        pw = None if p is None else torch.tensor([p], device=x.device)
        val = torch.nn.functional.binary_cross_entropy_with_logits(
            out.float(), t, weight=w.reshape(-1, 1), pos_weight=pw)
    else:
        val = (w.reshape(-1, 1) * (out.float() - t) ** 2).mean()
    val.backward()
    return val


def _step_data(m_rows, dev, loss):
    x = torch.randn(m_rows, 100, device=dev).bfloat16()
    if loss == "bce":
        t = torch.bernoulli(torch.full((m_rows, 1), 0.4, device=dev))
    else:
        t = torch.randn(m_rows, 1, device=dev)
    w = torch.randint(1, 65, (m_rows,), device=dev).float() / 16.0
    if m_rows > 4:
        w[3::5] = 0.0
    return x, t, w


@pytest.mark.parametrize("loss,p", [("bce", POS_WEIGHT), ("mse", None)])
def test_weighted_step_edge_batch_sizes(dev, loss, p):
    """Bounds and batch sizes of test_bce_step_edge_batch_sizes."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(33)
    for m_rows in [1, 17, 31, 32, 33, 255, 4097]:
        model = TabularMLP(100).to(dev)
        ref = TabularMLP(100).to(dev)
        ref.load_state_dict(model.state_dict())
        x, t, w = _step_data(m_rows, dev, loss)
        got = fused_step(model, x, t, loss=loss, sample_weight=w,
                         pos_weight=p)
        ref_loss = _eager(ref, x, t, w, loss, p)
        print(f"M={m_rows}: loss {got.item()!r} eager {ref_loss.item()!r}")
        assert torch.isfinite(got), m_rows
        assert (
            abs(got.item() - ref_loss.item())
            <= 0.05 * abs(ref_loss.item()) + 1e-3
        ), (m_rows, got.item(), ref_loss.item())
        if m_rows < 16:
            for _, q in model.named_parameters():
                assert torch.isfinite(q.grad).all(), m_rows
            continue
        for (n, q), (_, r) in zip(
            model.named_parameters(), ref.named_parameters()
        ):
            err = (q.grad - r.grad).abs().max()
            tol = 0.3 * r.grad.abs().max().clamp(min=1e-5) + 2e-2
            assert err <= tol, (m_rows, n, err.item())


@pytest.mark.parametrize("loss,p", [("bce", POS_WEIGHT), ("mse", None)])
def test_weighted_step_matches_eager_4097(dev, loss, p):
    """Bound of test_bce_step_matches_eager_4097."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(9)
    M = 4097
    model = TabularMLP(100).to(dev)
    ref = TabularMLP(100).to(dev)
    ref.load_state_dict(model.state_dict())
    x, t, w = _step_data(M, dev, loss)
    got = fused_step(model, x, t, loss=loss, sample_weight=w, pos_weight=p)
    ref_loss = _eager(ref, x, t, w, loss, p)
    print(f"loss {got.item()!r} eager {ref_loss.item()!r}")
    assert abs(got.item() - ref_loss.item()) <= 0.02 * ref_loss.item() + 1e-3
    for (n, q), (_, r) in zip(
        model.named_parameters(), ref.named_parameters()
    ):
        err = (q.grad - r.grad).abs().max().item()
        tol = (0.08 * r.grad.abs().mean().clamp(min=1e-5) + 1e-3).item()
        print(f"  {n}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (n, err, tol)


def _step(model, x, t, native, **kw):
    from ray_shuffling_data_loader_amd.models import fused_step as fs

    orig = fs._NATIVE_GLUE
    try:
        fs._NATIVE_GLUE = native
        return fs.fused_step(model, x, t, **kw)
    finally:
        fs._NATIVE_GLUE = orig


@pytest.mark.parametrize("loss,p", [("bce", POS_WEIGHT), ("mse", None)])
@pytest.mark.parametrize("m_rows", [1, 31, 33, 4097])
def test_weighted_native_step_matches_composed(dev, hip, m_rows, loss, p):
    """Bounds of test_bce_native_step_matches_composed: the two paths feed
    the kernels bit-identical inputs and differ only in the order of the
    fp32 partial sums; a second native call gives the same bits."""
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    assert hasattr(hip, "fused_step_bf16") and hip.HEAD_WEIGHTS == 1
    torch.manual_seed(100 + m_rows)
    m_nat = TabularMLP(100).to(dev)
    m_cmp = copy.deepcopy(m_nat)
    x, t, w = _step_data(m_rows, dev, loss)
    kw = dict(loss=loss, sample_weight=w, pos_weight=p)
    l_cmp = _step(m_cmp, x, t, native=False, **kw)
    l_nat = _step(m_nat, x, t, native=True, **kw)
    print(f"M={m_rows} loss native {l_nat.item()!r} composed "
          f"{l_cmp.item()!r}")
    assert l_nat.dtype == torch.float32 and l_nat.dim() == 0
    assert torch.allclose(l_nat, l_cmp, rtol=1e-5, atol=0.0)
    for (n, q), (_, r) in zip(
        m_nat.named_parameters(), m_cmp.named_parameters()
    ):
        assert q.grad.shape == r.grad.shape == q.shape, n
        tol = 1e-5 * r.grad.abs().max().item() + 1e-5
        err = (q.grad - r.grad).abs().max().item()
        print(f"  {n}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (n, err, tol)
    m_two = copy.deepcopy(m_cmp)
    for q in m_two.parameters():
        q.grad = None
    l_two = _step(m_two, x, t, native=True, **kw)
    assert torch.equal(l_two, l_nat)
    for q, r in zip(m_two.parameters(), m_nat.parameters()):
        assert torch.equal(q.grad, r.grad)
    # the weights did something
    m_un = copy.deepcopy(m_cmp)
    l_un = _step(m_un, x, t, native=True, loss=loss)
    assert not torch.equal(l_un, l_nat)


def test_weighted_native_step_flat_grads_same_bits(dev, hip):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(5)
    M = 4097
    m_plain = TabularMLP(100).to(dev)
    m_flat = copy.deepcopy(m_plain)
    ws = [q for n, q in m_flat.named_parameters() if n.endswith("weight")]
    bsz = [q for n, q in m_flat.named_parameters() if n.endswith("bias")]
    flat = torch.full((sum(q.numel() for q in ws + bsz),), float("nan"),
                      device=dev)
    off = 0
    for q in ws + bsz:
        q.grad = flat[off:off + q.numel()].view_as(q)
        off += q.numel()
    m_flat._rsdl_flat_grads = True
    ptrs = [q.grad.data_ptr() for q in m_flat.parameters()]
    x, t, w = _step_data(M, dev, "bce")
    # fp64 [M,1] weights: cast once by fused_step
    kw = dict(loss="bce", sample_weight=w.double().reshape(-1, 1),
              pos_weight=POS_WEIGHT)
    l_plain = _step(m_plain, x, t, native=True, **kw)
    l_flat = _step(m_flat, x, t, native=True, **kw)
    assert torch.equal(l_plain, l_flat)
    assert [q.grad.data_ptr() for q in m_flat.parameters()] == ptrs
    for q, r in zip(m_flat.parameters(), m_plain.parameters()):
        assert torch.equal(q.grad, r.grad)
    assert torch.isfinite(flat).all()
    # the staged hook route (composed) carries the arguments too
    m_hook = copy.deepcopy(m_plain)
    for q in m_hook.parameters():
        q.grad = torch.zeros_like(q)
    m_hook._rsdl_flat_grads = True
    stages = []
    l_hook = _step(m_hook, x, t, native=True, grad_hook=stages.append, **kw)
    assert stages == ["bias", "w1", "w2", "w3"]
    assert torch.allclose(l_hook, l_plain, rtol=1e-5, atol=0.0)


# 4. the evaluator
def _stage(hip, data):
    st = hip.step_prep([w.float() for w in data["Wb"]])
    return [st[0], st[1], st[2], st[5]]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("M", SHAPES)
def test_weighted_partials_column0_is_training_loss_part(hip, data, dev, M,
                                                         rows, task):
    x = data["x"][:M].contiguous()
    tgt = (data["reg"] if task == 0 else data["tgt"])[:M].contiguous()
    w = data["w"][:M].contiguous()
    _, part = hip.eval_chain_bf16(x, _stage(hip, data), data["bs"],
                                  target=tgt, rows=rows, task=task,
                                  weight=w, want_pred=False)
    f = _fwd(hip, data, data["bs"], M, rows, tgt, task, weight=w)
    nwg = (M + rows - 1) // rows
    assert part.shape == (nwg, 8) and part.dtype == torch.float32
    assert torch.equal(part[:, 0], f[7])
    assert not bool(part[:, 5:].any())
    # sum w per slab, exact
    assert torch.equal(part[:, 4], _slab_sums(w, rows))
    # unit weights: columns 0-3 are the unweighted kernel's
    ones = torch.ones(M, device=dev)
    _, p1 = hip.eval_chain_bf16(x, _stage(hip, data), data["bs"],
                                target=tgt, rows=rows, task=task,
                                weight=ones, want_pred=False)
    _, p0 = hip.eval_chain_bf16(x, _stage(hip, data), data["bs"],
                                target=tgt, rows=rows, task=task,
                                want_pred=False)
    assert p0.shape == (nwg, 4)
    assert torch.equal(p1[:, :4], p0)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_eval_accumulate_wide_partials(hip, dev, n):
    g = torch.Generator(device="cpu").manual_seed(n)
    part = torch.rand(n, 8, generator=g).to(dev)
    acc0 = torch.tensor([12345.0, 3.25, 1e3 + 1e-9, 0.5, 7.0, 2.5],
                        dtype=torch.float64, device=dev)
    acc = acc0.clone()
    hip.eval_accumulate(part, acc, 77)
    ref = acc0.clone()
    ref[0] += 77
    # thread i sums rows i, i + 256, ...; then a halving tree over the 256
    sh = torch.zeros(256, 5, dtype=torch.float64, device=dev)
    pd = part[:, :5].double()
    for r0 in range(0, n, 256):
        blk = pd[r0:r0 + 256]
        sh[:blk.shape[0]] += blk
    d = 128
    while d > 0:
        sh[:d] += sh[d:2 * d]
        d //= 2
    ref[1:] += sh[0]
    assert torch.equal(acc, ref)
    acc2 = acc0.clone()
    hip.eval_accumulate(part, acc2, 77)
    assert torch.equal(acc2, acc)


def _model(dev, seed=7):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    return TabularMLP(100).to(dev)


def _batches(dev, seed=11, regression=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = sum(BATCHES)
    x = torch.randn(n, 100, generator=g).bfloat16().to(dev)
    t = (torch.rand(n, 1, generator=g) >= 0.5).float().to(dev)
    if regression:
        t = torch.randn(n, 1, generator=g).to(dev)
    return x, t, _weights(n, g).to(dev)


def _ref_state(o, t, w):
    """fp64 {rows, sum w logloss, sum w brier, sum w t, sum w correct,
    sum w}."""
    o = o.reshape(-1)
    td = t.reshape(-1).double()
    wd = w.reshape(-1).double()
    terms, _ = _ref_head(o, t, w, 1, 1.0)
    od = o.double()
    e = torch.exp(-od.abs())
    sg = torch.where(od >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    correct = ((o >= 0) == (t.reshape(-1) >= 0.5)).double()
    return [float(td.numel()), terms.sum().item(),
            (wd * (sg - td) ** 2).sum().item(), (wd * td).sum().item(),
            (wd * correct).sum().item(), wd.sum().item()]


def _ref_hist(o, t, w):
    from ray_shuffling_data_loader_amd.models.fused_eval import logit_keys

    keys = logit_keys(o.reshape(-1))
    cls = (t.reshape(-1) >= 0.5).to(torch.int64)
    units = torch.round(w.reshape(-1).float() * 2.0 ** 20).double()
    return torch.bincount(cls * 65536 + keys, weights=units,
                          minlength=2 * 65536).to(torch.int64).view(2, 65536)


def _check_state(got, want, tag):
    print(f"{tag}: state {got} ref {want}")
    assert len(got) == 6
    for c in (0, 3, 4, 5):
        assert got[c] == want[c], (tag, c, got, want)
    for c in (1, 2):
        assert abs(got[c] - want[c]) <= REL * abs(want[c]), (
            tag, c, got[c], want[c])


@pytest.mark.parametrize("rows", ROWS)
def test_weighted_binary_evaluator_over_batches(dev, rows):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    model = _model(dev)
    x, t, w = _batches(dev)
    ev = fe.FusedEvaluator(model, rows=rows, task="binary", weighted=True)
    o = ev.predict(x)
    off = 0
    for b in BATCHES:
        ev.reset()
        ev.update(x[off:off + b], t[off:off + b], w[off:off + b])
        _check_state(ev.state().tolist(),
                     _ref_state(o[off:off + b], t[off:off + b],
                                w[off:off + b]),
                     f"rows={rows} batch {b}")
        off += b
    ev.reset()
    off = 0
    for b in BATCHES:
        ev.update(x[off:off + b], t[off:off + b], w[off:off + b])
        off += b
    want = _ref_state(o, t, w)
    _check_state(ev.state().tolist(), want, f"rows={rows} all")
    h = ev.hist_state()
    ref_h = _ref_hist(o, t, w)
    assert h.dtype == torch.int64 and h.shape == (2, 65536)
    assert torch.equal(h, ref_h)
    assert int(h.sum()) == int(torch.round(w * 2.0 ** 20).long().sum())
    got = ev.compute()
    assert set(got) == {"rows", "weight_sum", "logloss", "accuracy",
                        "brier", "base_rate", "auc"}
    assert got["rows"] == 162 and got["weight_sum"] == want[5]
    assert got["accuracy"] == want[4] / want[5]
    assert got["base_rate"] == want[3] / want[5]
    assert abs(got["logloss"] - want[1] / want[5]) <= REL * want[1] / want[5]
    # the statistic pair by pair, in fp64, from the keys and the weights
    keys = fe.logit_keys(o.reshape(-1)).cpu()
    cls = (t.reshape(-1) >= 0.5).cpu()
    wc = w.double().cpu()
    kp, kn, wp, wn = keys[cls], keys[~cls], wc[cls], wc[~cls]
    pair = wp[:, None] * wn[None, :]
    pairs_auc = ((pair * ((kp[:, None] > kn[None, :]).double()
                          + 0.5 * (kp[:, None] == kn[None, :]).double())
                  ).sum() / (wp.sum() * wn.sum())).item()
    print(f"auc {got['auc']!r} pairs {pairs_auc!r}")
    assert abs(got["auc"] - pairs_auc) <= 1e-12
    assert abs(got["auc"] - fe.auc_from_hist(ref_h.cpu())) <= 1e-12
    # the same rows in one batch: the identical histogram
    one = fe.FusedEvaluator(model, rows=rows, task="binary", weighted=True)
    one.update(x, t, w)
    assert torch.equal(one.hist_state(), h)
    # weighted=False on the same inputs: what it always gave, and unit
    # weights give its sums and its histogram in fixed point
    plain = fe.FusedEvaluator(model, rows=rows, task="binary")
    plain.update(x, t)
    unit = fe.FusedEvaluator(model, rows=rows, task="binary", weighted=True)
    unit.update(x, t, torch.ones_like(t))
    assert plain.state().shape == (5,)
    assert torch.equal(unit.state()[:5], plain.state())
    assert torch.equal(unit.hist_state(), plain.hist_state() * (1 << 20))
    with pytest.raises(ValueError, match="weighted=True"):
        plain.update(x, t, w)


@pytest.mark.parametrize("rows", ROWS)
def test_weighted_regression_evaluator_over_batches(dev, rows):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    model = _model(dev)
    x, t, w = _batches(dev, regression=True)
    ev = fe.FusedEvaluator(model, rows=rows, weighted=True)
    o = ev.predict(x).reshape(-1).double()
    off = 0
    for b in BATCHES:
        ev.update(x[off:off + b], t[off:off + b], w[off:off + b])
        off += b
    got = ev.compute()
    td, wd = t.reshape(-1).double(), w.double()
    sw = wd.sum().item()
    d = o - td
    sse = (wd * d * d).sum().item()
    den = (wd * td * td).sum().item() - (wd * td).sum().item() ** 2 / sw
    want = {"mse": sse / sw, "rmse": math.sqrt(sse / sw),
            "mae": (wd * d.abs()).sum().item() / sw, "r2": 1.0 - sse / den}
    assert got["rows"] == 162 and got["weight_sum"] == sw
    for k in want:
        bound = 1e-5 * abs(want[k]) + 1e-5
        print(f"{k}: got {got[k]!r} want {want[k]!r} bound {bound:.3e}")
        assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", [1, 33, 97])
def test_weighted_eval_without_hist_writes_nothing_else(hip, data, dev, M,
                                                        rows):
    """The pattern of test_binary_eval_without_hist_writes_nothing_else:
    given no histogram, the weighted kernel writes its predictions and
    partials only."""
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    stage = _stage(hip, data)
    x = data["x"][:M].contiguous()
    tgt = data["hard"][:M].contiguous()
    w = data["w"][:M].contiguous()
    canary = -12345.5
    big = torch.full((8 + M + 8,), canary, dtype=torch.float32, device=dev)
    pred, part = hip.eval_chain_bf16(
        x, stage, data["bs"], target=tgt, pred_out=big[8:8 + M], rows=rows,
        task=1, weight=w)
    hist = torch.zeros(2, 65536, dtype=torch.int64, device=dev)
    pred2, part2 = hip.eval_chain_bf16(
        x, stage, data["bs"], target=tgt, rows=rows, task=1, hist=hist,
        weight=w)
    torch.cuda.synchronize()
    assert bool((big[:8] == canary).all()) and bool(
        (big[8 + M:] == canary).all())
    assert torch.equal(big[8:8 + M], pred2) and torch.equal(part, part2)
    # rows >= M added nothing
    assert int(hist.sum()) == int(torch.round(w * 2.0 ** 20).long().sum())
    assert torch.equal(hist, _ref_hist(pred2, tgt, w))
    ev = fe.FusedEvaluator(_model_from(data["Wb"], data["bs"], dev),
                           rows=rows, task="binary", auc=False,
                           weighted=True)
    ev.update(x, tgt, w)
    got = ev.compute()
    assert "auc" not in got and ev.hist_state() is None
    assert ev._hist is None and got["weight_sum"] == w.double().sum().item()


# 5. bindings
def test_weight_bindings_validate_arguments(hip, data, dev):
    Wb, bs = data["Wb"], data["bs"]
    x = data["x"][:8].contiguous()
    tgt = data["hard"][:8].contiguous()
    w = data["w"][:8].contiguous()
    assert hip.HEAD_WEIGHTS == 1
    fp32w = [m.float() for m in Wb]

    def fwd(**kw):
        return hip.fwd_chain_bf16(x, Wb[0], bs[0], Wb[1], bs[1], Wb[2],
                                  bs[2], Wb[3].flatten(), bs[3], target=tgt,
                                  **kw)

    stage = _stage(hip, data)
    bad_weights = (
        w.double(),                         # dtype
        data["w"][:9].contiguous(),         # numel
        data["w"][:16:2],                   # not contiguous
        w.cpu(),                            # device
    )
    for bad in bad_weights:
        with pytest.raises(RuntimeError, match="weight must be contiguous"):
            fwd(loss=1, weight=bad)
        with pytest.raises(RuntimeError, match="weight must be contiguous"):
            hip.fused_step_bf16(x, tgt, fp32w, bs, loss=1, weight=bad)
        with pytest.raises(RuntimeError, match="weight must be contiguous"):
            hip.eval_chain_bf16(x, stage, bs, target=tgt, task=1, weight=bad)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="finite and > 0"):
            fwd(loss=1, pos_weight=bad)
        with pytest.raises(RuntimeError, match="finite and > 0"):
            hip.fused_step_bf16(x, tgt, fp32w, bs, loss=1, pos_weight=bad)
    with pytest.raises(RuntimeError, match="pos_weight needs loss=1"):
        fwd(loss=0, pos_weight=2.0)
    with pytest.raises(RuntimeError, match="pos_weight needs loss=1"):
        hip.fused_step_bf16(x, tgt, fp32w, bs, pos_weight=2.0)
    with pytest.raises(RuntimeError, match="weight needs a target"):
        hip.eval_chain_bf16(x, stage, bs, weight=w)
    with pytest.raises(RuntimeError, match="need a target"):
        hip.fwd_chain_bf16(x, Wb[0], bs[0], Wb[1], bs[1], Wb[2], bs[2],
                           Wb[3].flatten(), bs[3], weight=w)
    acc6 = torch.zeros(6, dtype=torch.float64, device=dev)
    acc5 = torch.zeros(5, dtype=torch.float64, device=dev)
    p8 = torch.zeros(3, 8, device=dev)
    p4 = torch.zeros(3, 4, device=dev)
    with pytest.raises(RuntimeError, match=r"fp64 \[6\]"):
        hip.eval_accumulate(p8, acc5, 1)
    with pytest.raises(RuntimeError, match=r"fp64 \[5\]"):
        hip.eval_accumulate(p4, acc6, 1)
    with pytest.raises(RuntimeError, match="part must be contiguous"):
        hip.eval_accumulate(torch.zeros(3, 5, device=dev), acc6, 1)
    assert not bool(acc5.any()) and not bool(acc6.any())
    # an empty batch: zero partials of the weighted width
    _, part = hip.eval_chain_bf16(
        x[:0], stage, bs, target=tgt[:0].contiguous(), task=1,
        weight=w[:0].contiguous())
    assert torch.equal(part.cpu(), torch.zeros(1, 8))
