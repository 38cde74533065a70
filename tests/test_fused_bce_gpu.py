"""GPU tests of the binary-classification objective: the BCE head of
fwd_chain_kernel, the binary task and AUC histogram of eval_chain_kernel
(csrc/fwd_chain.hip), their bindings, ``fused_step(loss="bce")`` and
``FusedEvaluator(task="binary")``.

Shapes: the smallest that reach every tail — a single row, a partial and
a full first m-tile, a partial and a full second m-tile, an odd tile
count whose last 64-row workgroup has no second m-tile — at both slab
sizes.

Bounds.
  loss_part / the evaluator's logloss and brier sums: rel 2e-5 against
    fp64 on the kernel's own fp32 logits. A slab sums at most 64
    non-negative fp32 terms, each a few ulp off from expf and log1pf;
    serial fp32 summation adds at most 64 * 2^-24 ~ 4e-6.
  dyb: one bf16 ulp (2^-8 relative) around bf16 of the fp64 value.
  counts (rows, sum t for 0/1 targets, n_correct, the histogram): exact.
  whole step against eager autocast: the project's own bounds for the
    same pipeline (tests/test_gpu_kernels.py::
    test_fused_step_edge_batch_sizes and ::test_fused_step_matches_eager).
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


@pytest.fixture(scope="module")
def data(dev):
    """Seeded bf16-exact weights, fp32 biases, the largest batch (smaller
    shapes take its leading rows) and targets in [0, 1]: hard 0/1 labels
    in the even rows, soft ones in the odd rows."""
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
    return {
        "Wb": Wb,
        "bs": bs,
        "x": rn(M_MAX, 100).bfloat16(),
        "tgt": torch.where(even, hard, soft),
        "hard": hard,
    }


def _fwd(hip, data, bs, M, rows, tgt, loss):
    Wb = data["Wb"]
    return hip.fwd_chain_bf16(
        data["x"][:M].contiguous(), Wb[0], bs[0], Wb[1], bs[1], Wb[2],
        bs[2], Wb[3].flatten(), bs[3], target=tgt, rows=rows, loss=loss,
    )


def _ref_terms(o, t):
    """fp64 (sigmoid, logloss) of fp32 logits and fp32 targets."""
    o = o.reshape(-1).double()
    t = t.reshape(-1).float().double()
    e = torch.exp(-o.abs())
    sg = torch.where(o >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    ll = torch.clamp(o, min=0.0) - o * t + torch.log1p(e)
    return sg, ll


def _slab_sums(v, rows):
    n = v.numel()
    nwg = (n + rows - 1) // rows
    return torch.nn.functional.pad(v, (0, nwg * rows - n)).view(
        nwg, rows).sum(1)


def _check_head(hip, data, dev, bs, M, rows, tgt, tag):
    """The BCE head of fwd_chain_bf16 against fp64 on the logits of
    FusedEvaluator.predict (bit-equal to the training head's)."""
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    f1 = _fwd(hip, data, bs, M, rows, tgt, 1)
    f0 = _fwd(hip, data, bs, M, rows, tgt, 0)
    assert len(f1) == 8 and len(f0) == 8
    # the loss must not reach the layers (bit patterns, through integer
    # views; every element of these six is written by the kernel)
    for i, nm in enumerate(["a1t", "mask1", "a2t", "mask2", "a3", "out"]):
        a, b = f1[i], f0[i]
        if a.dtype == torch.bfloat16:
            a, b = a.view(torch.int16), b.view(torch.int16)
        assert torch.equal(a, b), (tag, nm)
    model = _model_from(data["Wb"], bs, dev)
    o = fe.FusedEvaluator(model, rows=rows).predict(
        data["x"][:M].contiguous()).reshape(-1)
    assert torch.equal(o.bfloat16(), f1[5].flatten()), tag
    sg, ll = _ref_terms(o, tgt)
    ref_lp = _slab_sums(ll, rows)
    lp = f1[7]
    assert lp.shape == ref_lp.shape and lp.dtype == torch.float32
    assert bool(torch.isfinite(lp).all()), (tag, lp)
    # FP32_TINY: a slab whose rows are all saturated on the right side
    # sums to ~1e-87 in fp64, below anything fp32 holds (the kernel's 0)
    err_lp = (lp.double() - ref_lp).abs()
    rel = (err_lp / ref_lp.abs().clamp(min=FP32_TINY)).max().item()
    print(f"{tag}: loss_part max rel err {rel:.3e} (bound {REL:.0e})")
    assert bool((err_lp <= REL * ref_lp.abs() + FP32_TINY).all()), (
        tag, lp, ref_lp)
    ref_d = ((sg - tgt.reshape(-1).double()) / M).float().bfloat16().float()
    dyb = f1[6].flatten().float()
    err = (dyb - ref_d).abs()
    print(f"{tag}: dyb max err {err.max().item():.3e}")
    assert bool((err <= BF16_ULP * ref_d.abs()).all()), (
        tag, dyb, ref_d)
    return f1, f0, o, dyb


# 1. the head in isolation
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", SHAPES)
def test_bce_head_in_isolation(hip, data, dev, M, rows):
    tgt = data["tgt"][:M].contiguous()
    f1, f0, _, _ = _check_head(
        hip, data, dev, data["bs"], M, rows, tgt, f"M={M} rows={rows}")
    # the two heads differ where they should
    assert not torch.equal(f1[7], f0[7])


# 2. saturated logits
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("b4", [200.0, -200.0])
@pytest.mark.parametrize("M", [1, 33, 97])
def test_bce_head_saturation(hip, data, dev, M, rows, b4):
    bs = list(data["bs"][:3]) + [torch.tensor([b4], device=dev)]
    tgt = data["hard"][:M].contiguous()
    if M > 1:
        assert 0 < tgt.sum().item() < M  # 0 and 1 mixed
    _, _, o, dyb = _check_head(
        hip, data, dev, bs, M, rows, tgt, f"M={M} rows={rows} b4={b4}")
    assert bool((o.abs() > 150).all())
    if b4 > 0:
        # what the softplus form is for
        assert bool(torch.isinf(torch.log(1 + torch.exp(o))).all())
    # dyb is +-1/M or 0 to one ulp
    wrong = (tgt == 0) if b4 > 0 else (tgt == 1)
    want = torch.where(wrong, math.copysign(1.0 / M, b4), 0.0)
    want = want.to(dev).bfloat16().float()
    assert bool(((dyb - want).abs() <= BF16_ULP * want.abs()).all()), (
        dyb, want)


# 3. the whole step against eager autocast
def _eager_bce(ref, x, t):
    with torch.autocast("cuda", torch.bfloat16):
        out = ref(x)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            out.float(), t)
    loss.backward()
    return loss


def test_bce_step_edge_batch_sizes(dev):
    """Bounds and batch sizes of test_fused_step_edge_batch_sizes."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(33)
    for m_rows in [1, 17, 31, 32, 33, 255, 4097]:
        model = TabularMLP(100).to(dev)
        ref = TabularMLP(100).to(dev)
        ref.load_state_dict(model.state_dict())
        x = torch.randn(m_rows, 100, device=dev).bfloat16()
        t = torch.bernoulli(torch.full((m_rows, 1), 0.4, device=dev))
        loss = fused_step(model, x, t, loss="bce")
        ref_loss = _eager_bce(ref, x, t)
        print(f"M={m_rows}: loss {loss.item()!r} eager {ref_loss.item()!r}")
        assert torch.isfinite(loss), m_rows
        assert (
            abs(loss.item() - ref_loss.item())
            <= 0.05 * abs(ref_loss.item()) + 1e-3
        ), (m_rows, loss.item(), ref_loss.item())
        if m_rows < 16:
            # ill-posed at single-digit M (relu-mask flips), as in the
            # MSE test: finiteness + loss parity is the check
            for _, p in model.named_parameters():
                assert torch.isfinite(p.grad).all(), m_rows
            continue
        for (n, p), (_, q) in zip(
            model.named_parameters(), ref.named_parameters()
        ):
            err = (p.grad - q.grad).abs().max()
            tol = 0.3 * q.grad.abs().max().clamp(min=1e-5) + 2e-2
            assert err <= tol, (m_rows, n, err.item())


def test_bce_step_matches_eager_4097(dev):
    """Bound of test_fused_step_matches_eager at M = 4097."""
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(9)
    M = 4097
    model = TabularMLP(100).to(dev)
    ref = TabularMLP(100).to(dev)
    ref.load_state_dict(model.state_dict())
    x = torch.randn(M, 100, device=dev).bfloat16()
    t = torch.bernoulli(torch.full((M, 1), 0.4, device=dev))
    loss = fused_step(model, x, t, loss="bce")
    ref_loss = _eager_bce(ref, x, t)
    print(f"loss {loss.item()!r} eager {ref_loss.item()!r}")
    assert abs(loss.item() - ref_loss.item()) <= 0.02 * ref_loss.item() + 1e-3
    for (n, p), (_, q) in zip(
        model.named_parameters(), ref.named_parameters()
    ):
        err = (p.grad - q.grad).abs().max().item()
        tol = (0.08 * q.grad.abs().mean().clamp(min=1e-5) + 1e-3).item()
        print(f"  {n}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (n, err, tol)


# 4. native against composed, flat-grad mode
def _step(model, x, t, native, **kw):
    from ray_shuffling_data_loader_amd.models import fused_step as fs

    orig = fs._NATIVE_GLUE
    try:
        fs._NATIVE_GLUE = native
        return fs.fused_step(model, x, t, loss="bce", **kw)
    finally:
        fs._NATIVE_GLUE = orig


@pytest.mark.parametrize("m_rows", [1, 31, 33, 4097])
def test_bce_native_step_matches_composed(dev, hip, m_rows):
    """What test_step_glue_gpu.py::test_native_step_matches_composed
    requires for MSE, with loss="bce": both paths feed the chain and wgrad
    kernels bit-identical inputs (the composed path passes loss=1 to the
    same forward kernel) and differ only in the order of the fp32 partial
    sums — loss at rtol 1e-5, gradients at 1e-5 * max|g| + 1e-5 — and a
    second native call gives the same bits.

    Native and composed are NOT bit-equal to each other, for either loss:
    the composed path sums loss_part and the wgrad slabs with torch ops,
    the native one in step_finalize. Measured on an MI355X
    (profiles/r06/native_vs_composed_bits.txt): MSE is bit-equal at
    M = 1 and 31, differs in the last bit of the loss and of dW1-dW3 at
    M = 33 and in every gradient at M = 4097; BCE is bit-equal at M = 1,
    differs by one ulp of the loss at M = 31 and like MSE at 33 and 4097
    (largest gradient difference 7.5e-9). Hence the MSE test's bounds, and
    bit-equality only where that test has it: between two native calls."""
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    assert hasattr(hip, "fused_step_bf16") and hip.LOSS_BCE == 1
    torch.manual_seed(100 + m_rows)
    m_nat = TabularMLP(100).to(dev)
    m_cmp = copy.deepcopy(m_nat)
    x = torch.randn(m_rows, 100, device=dev).bfloat16()
    t = torch.bernoulli(torch.full((m_rows, 1), 0.4, device=dev))
    l_cmp = _step(m_cmp, x, t, native=False)
    l_nat = _step(m_nat, x, t, native=True)
    bit_equal = torch.equal(l_nat, l_cmp) and all(
        torch.equal(p.grad, q.grad)
        for p, q in zip(m_nat.parameters(), m_cmp.parameters()))
    print(f"M={m_rows} loss native {l_nat.item()!r} composed "
          f"{l_cmp.item()!r} bit-equal {bit_equal}")
    assert l_nat.dtype == torch.float32 and l_nat.dim() == 0
    assert torch.allclose(l_nat, l_cmp, rtol=1e-5, atol=0.0)
    for (n, p), (_, q) in zip(
        m_nat.named_parameters(), m_cmp.named_parameters()
    ):
        assert p.grad.shape == q.grad.shape == p.shape, n
        tol = 1e-5 * q.grad.abs().max().item() + 1e-5
        err = (p.grad - q.grad).abs().max().item()
        print(f"  {n}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (n, err, tol)
    m_two = copy.deepcopy(m_cmp)
    for p in m_two.parameters():
        p.grad = None
    l_two = _step(m_two, x, t, native=True)
    assert torch.equal(l_two, l_nat)
    for p, q in zip(m_two.parameters(), m_nat.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_bce_native_step_flat_grads_same_bits(dev, hip):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(5)
    M = 4097
    m_plain = TabularMLP(100).to(dev)
    m_flat = copy.deepcopy(m_plain)
    ws = [p for n, p in m_flat.named_parameters() if n.endswith("weight")]
    bsz = [p for n, p in m_flat.named_parameters() if n.endswith("bias")]
    flat = torch.full((sum(p.numel() for p in ws + bsz),), float("nan"),
                      device=dev)
    off = 0
    for p in ws + bsz:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    m_flat._rsdl_flat_grads = True
    ptrs = [p.grad.data_ptr() for p in m_flat.parameters()]
    x = torch.randn(M, 100, device=dev).bfloat16()
    t = torch.bernoulli(torch.full((M, 1), 0.4, device=dev))
    l_plain = _step(m_plain, x, t, native=True)
    l_flat = _step(m_flat, x, t, native=True)
    assert torch.equal(l_plain, l_flat)
    assert [p.grad.data_ptr() for p in m_flat.parameters()] == ptrs
    for p, q in zip(m_flat.parameters(), m_plain.parameters()):
        assert torch.equal(p.grad, q.grad)
    assert torch.isfinite(flat).all()


# 5. it learns
def test_bce_step_actually_learns(dev):
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(21)
    M = 8192
    model = TabularMLP(100).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=5e-2, momentum=0.9)
    w_true = torch.randn(100, 1, device=dev) * 0.3
    losses = []
    for _ in range(60):
        x = torch.randn(M, 100, device=dev).bfloat16()
        t = torch.bernoulli(torch.sigmoid(x.float() @ w_true))
        loss = fused_step(model, x, t, loss="bce")
        opt.step()
        losses.append(float(loss))
    start = sum(losses[:5]) / 5
    end = sum(losses[-5:]) / 5
    print(f"start {start:.4f} end {end:.4f}")
    assert end < start and end < math.log(2.0), (start, end, losses[::10])


# 6. the evaluator
def _model(dev, seed=7):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(seed)
    return TabularMLP(100).to(dev)


def _batches(dev, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = sum(BATCHES)
    x = torch.randn(n, 100, generator=g).bfloat16().to(dev)
    t = (torch.rand(n, 1, generator=g) >= 0.5).float().to(dev)
    return x, t


def _ref_state(o, t):
    """fp64 {rows, sum logloss, sum brier, sum t, n_correct}."""
    sg, ll = _ref_terms(o, t)
    td = t.reshape(-1).double()
    correct = ((o.reshape(-1) >= 0) == (t.reshape(-1) >= 0.5)).sum().item()
    return [float(td.numel()), ll.sum().item(),
            ((sg - td) ** 2).sum().item(), td.sum().item(), float(correct)]


def _ref_hist(o, t):
    from ray_shuffling_data_loader_amd.models.fused_eval import logit_keys

    keys = logit_keys(o.reshape(-1))
    cls = (t.reshape(-1) >= 0.5).to(torch.int64)
    return torch.bincount(cls * 65536 + keys, minlength=2 * 65536).view(
        2, 65536)


def _check_state(got, want, tag):
    print(f"{tag}: state {got} ref {want}")
    assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4], (
        tag, got, want)
    for c in (1, 2):
        assert abs(got[c] - want[c]) <= REL * abs(want[c]), (
            tag, c, got[c], want[c])


@pytest.mark.parametrize("rows", ROWS)
def test_binary_evaluator_over_batches(dev, rows):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    model = _model(dev)
    x, t = _batches(dev)
    ev = fe.FusedEvaluator(model, rows=rows, task="binary")
    o = torch.cat([ev.predict(x[a:b]) for a, b in ((0, 97), (97, 161),
                                                    (161, 162))])
    assert torch.equal(o, ev.predict(x))
    # per batch
    off = 0
    for b in BATCHES:
        ev.reset()
        ev.update(x[off:off + b], t[off:off + b])
        _check_state(ev.state().tolist(),
                     _ref_state(o[off:off + b], t[off:off + b]),
                     f"rows={rows} batch {b}")
        off += b
    # accumulated
    ev.reset()
    off = 0
    for b in BATCHES:
        ev.update(x[off:off + b], t[off:off + b])
        off += b
    _check_state(ev.state().tolist(), _ref_state(o, t), f"rows={rows} all")
    h = ev.hist_state()
    ref_h = _ref_hist(o, t)
    assert h.dtype == torch.int64 and h.shape == (2, 65536)
    assert torch.equal(h, ref_h)
    assert int(h.sum()) == sum(BATCHES)
    got = ev.compute()
    assert set(got) == {"rows", "logloss", "accuracy", "brier",
                        "base_rate", "auc"}
    ref_auc = fe.auc_from_hist(ref_h.cpu())
    # an independent evaluation of the same statistic from the keys:
    # pairs counted one by one in integers
    keys = fe.logit_keys(o.reshape(-1)).cpu()
    cls = (t.reshape(-1) >= 0.5).cpu()
    kp, kn = keys[cls], keys[~cls]
    twice = (2 * (kp[:, None] > kn[None, :]).sum()
             + (kp[:, None] == kn[None, :]).sum()).item()
    pairs_auc = twice / (2.0 * kp.numel() * kn.numel())
    print(f"auc {got['auc']!r} ref {ref_auc!r} pairs {pairs_auc!r}")
    assert abs(got["auc"] - pairs_auc) <= 1e-12
    assert abs(got["auc"] - ref_auc) <= 1e-12
    st = _ref_state(o, t)
    assert got["rows"] == 162 and got["accuracy"] == st[4] / 162
    assert got["base_rate"] == st[3] / 162
    # the same rows in one batch of 162: the identical histogram
    one = fe.FusedEvaluator(model, rows=rows, task="binary")
    one.update(x, t)
    assert torch.equal(one.hist_state(), h)
    ev.reset()
    assert not bool(ev.hist_state().any()) and not bool(ev.state().any())
    assert math.isnan(ev.compute()["auc"])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", [1, 33, 97])
def test_binary_eval_without_hist_writes_nothing_else(hip, data, dev, M,
                                                      rows):
    """auc=False: no histogram exists, and the kernel given no histogram
    writes its predictions and partials only — canaries around a
    caller-owned prediction buffer stay, and the partials are those of
    the run with a histogram."""
    from ray_shuffling_data_loader_amd.models import fused_eval as fe

    st = hip.step_prep([w.float() for w in data["Wb"]])
    stage = [st[0], st[1], st[2], st[5]]
    x = data["x"][:M].contiguous()
    tgt = data["hard"][:M].contiguous()
    canary = -12345.5
    big = torch.full((8 + M + 8,), canary, dtype=torch.float32, device=dev)
    pred, part = hip.eval_chain_bf16(
        x, stage, data["bs"], target=tgt, pred_out=big[8:8 + M], rows=rows,
        task=1)
    hist = torch.zeros(2, 65536, dtype=torch.int64, device=dev)
    pred2, part2 = hip.eval_chain_bf16(
        x, stage, data["bs"], target=tgt, rows=rows, task=1, hist=hist)
    torch.cuda.synchronize()
    assert bool((big[:8] == canary).all()) and bool(
        (big[8 + M:] == canary).all())
    assert torch.equal(big[8:8 + M], pred2) and torch.equal(part, part2)
    assert int(hist.sum()) == M  # rows >= M added nothing
    assert torch.equal(hist, _ref_hist(pred2, tgt))
    # regression partials of the same call are the parent's columns
    _, part0 = hip.eval_chain_bf16(x, stage, data["bs"], target=tgt,
                                   rows=rows, want_pred=False)
    assert torch.equal(part0[:, 2], part[:, 2])  # sum t either way
    ev = fe.FusedEvaluator(_model_from(data["Wb"], data["bs"], dev),
                           rows=rows, task="binary", auc=False)
    ev.update(x, tgt)
    got = ev.compute()
    assert "auc" not in got and ev.hist_state() is None
    assert ev._hist is None


def test_binary_evaluator_agrees_with_bce_step_loss(dev):
    from ray_shuffling_data_loader_amd.models import fused_eval as fe
    from ray_shuffling_data_loader_amd.models.fused_step import fused_step

    model = _model(dev)
    x, t = _batches(dev)
    x, t = x[:161].contiguous(), t[:161].contiguous()
    loss = fused_step(model, x, t, loss="bce").item()
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    ev = fe.FusedEvaluator(model, task="binary")
    ev.update(x, t)
    ll = ev.compute()["logloss"]
    print(f"fused_step bce loss {loss!r}  evaluator logloss {ll!r}")
    # the same fp32 slab sums, added in fp32 and divided there vs in fp64
    assert abs(loss - ll) <= 1e-6 * abs(loss)
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), params[n]), n
        assert torch.equal(p.grad, grads[n]), n


# 7. bindings
def test_bce_bindings_validate_arguments(hip, data, dev):
    Wb, bs = data["Wb"], data["bs"]
    x = data["x"][:8].contiguous()
    tgt = data["hard"][:8].contiguous()
    assert hip.LOSS_MSE == 0 and hip.LOSS_BCE == 1
    with pytest.raises(RuntimeError, match="loss must be 0"):
        hip.fwd_chain_bf16(x, Wb[0], bs[0], Wb[1], bs[1], Wb[2], bs[2],
                           Wb[3].flatten(), bs[3], target=tgt, loss=2)
    with pytest.raises(RuntimeError, match="loss must be 0"):
        hip.fused_step_bf16(x, tgt, [w.float() for w in Wb], bs, loss=-1)
    st = hip.step_prep([w.float() for w in Wb])
    stage = [st[0], st[1], st[2], st[5]]
    with pytest.raises(RuntimeError, match="task must be 0"):
        hip.eval_chain_bf16(x, stage, bs, target=tgt, task=2)
    good = torch.zeros(2, 65536, dtype=torch.int64, device=dev)
    for bad in (
        good.to(torch.int32),                     # dtype
        torch.zeros(2, 65535, dtype=torch.int64, device=dev),  # shape
        torch.zeros(65536, 2, dtype=torch.int64, device=dev),
        torch.zeros(2 * 65536, dtype=torch.int64, device=dev),
        torch.zeros(2, 2 * 65536, dtype=torch.int64,
                    device=dev)[:, ::2],          # not contiguous
        good.cpu(),                               # device
    ):
        with pytest.raises(RuntimeError, match="hist must be contiguous"):
            hip.eval_chain_bf16(x, stage, bs, target=tgt, task=1, hist=bad)
    with pytest.raises(RuntimeError, match="hist needs task=1"):
        hip.eval_chain_bf16(x, stage, bs, target=tgt, task=0, hist=good)
    with pytest.raises(RuntimeError, match="hist needs task=1"):
        hip.eval_chain_bf16(x, stage, bs, task=1, hist=good)
    assert not bool(good.any())
    # an empty batch leaves the histogram alone
    _, part = hip.eval_chain_bf16(
        x[:0], stage, bs, target=tgt[:0].contiguous(), task=1, hist=good)
    assert torch.equal(part.cpu(), torch.zeros(1, 4))
    assert not bool(good.any())
