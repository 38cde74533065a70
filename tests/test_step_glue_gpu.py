"""GPU tests of the fused step's native glue (csrc/step_glue.hip):
step_prep, step_finalize, and hip.fused_step_bf16 against the composed
path of models/fused_step.py. Oracles are torch constructions."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    return shuffle_ops._load_hip()


def _swz(W):
    """shuffle_ops.cpp swizzle_frag: [N,K] -> [N/32][K/16][2][32][8]."""
    N, K = W.shape
    return (
        W.view(N // 32, 32, K // 16, 2, 8)
        .permute(0, 2, 3, 1, 4)
        .contiguous()
        .view(-1)
    )


def _swz_t(W):
    """shuffle_ops.cpp swizzle_frag_T: model-layout W [K,N] -> the
    fragment-major swizzle of W^T."""
    K, N = W.shape
    return (
        W.view(K // 16, 2, 8, N // 32, 32)
        .permute(3, 0, 1, 4, 2)
        .contiguous()
        .view(-1)
    )


def _bits(vals, dev):
    return torch.tensor(vals, dtype=torch.int32, device=dev).view(
        torch.float32
    )


def _salt(W, dev):
    """Overwrite the head of W with the rounding corner cases."""
    special = torch.cat([
        _bits([
            0x3F808000,  # tie, kept mantissa even -> rounds DOWN to 0x3F80
            0x3F818000,  # tie, kept mantissa odd  -> rounds UP to 0x3F82
            0x3F808001,  # just above a tie -> up
            0x3F807FFF,  # just below a tie -> down
            0x3F7F8000,  # tie that carries into the exponent
            0x00000001,  # smallest denormal
            0x00008000,  # denormal tie (even) -> 0
            0x00018000,  # denormal tie (odd) -> up
            0x007FFFFF,  # largest denormal
            0x7F7F0000,  # large, exactly representable
            0x7F7FFFFF,  # FLT_MAX -> +inf in bf16
        ], dev),
        -_bits([0x3F808000, 0x3F818000, 0x00018000, 0x7F7F0000,
                0x7F7FFFFF], dev),
        torch.tensor([-0.0, 0.0, 3.0e38, -3.0e38, 1e-40, -1e-40],
                     device=dev),
    ])
    flat = W.view(-1)
    n = special.numel()
    # head of the first row and a strided spread through the rest
    flat[:n] = special
    idx = torch.arange(n, device=dev) * 97 + 131
    flat[idx % flat.numel()] = special
    return W


def _master(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    shapes = [(512, 100), (256, 512), (128, 256), (1, 128)]
    return [
        _salt(torch.randn(s, device=dev, generator=g) / 8, dev)
        for s in shapes
    ]


def test_prep_matches_torch_construction(dev, hip):
    W = _master(dev, 1)
    nan_bf16 = torch.tensor([0x7FC1], dtype=torch.int16, device=dev)
    numel = [512 * 112, 256 * 512, 128 * 256, 256 * 512, 128 * 256, 128]
    bufs = [
        nan_bf16.expand(n).contiguous().view(torch.bfloat16) for n in numel
    ]
    assert all(torch.isnan(b).all() for b in bufs)
    got = hip.step_prep(W, None, bufs)
    assert len(got) == 6
    for g, b in zip(got, bufs):
        assert g.data_ptr() == b.data_ptr()
    Wb = [w.bfloat16() for w in W]
    W1p = torch.nn.functional.pad(Wb[0], (0, 12))
    want = [
        _swz(W1p), _swz(Wb[1]), _swz(Wb[2]), _swz_t(Wb[1]), _swz_t(Wb[2]),
        Wb[3].view(-1),
    ]
    names = ["W1s", "W2s", "W3s", "W2Ts", "W3Ts", "w4"]
    for n, g, w in zip(names, got, want):
        # bit compare: torch.equal on the int16 views (0.0 == -0.0 and
        # inf == inf would hide a sign or rounding slip in a float compare)
        assert torch.equal(g.view(torch.int16), w.view(torch.int16)), n
    # the W1 pad (k 100..111) was written as zeros over the NaN fill
    w1 = got[0].view(16, 7, 2, 32, 8)
    assert (w1[:, 6, 1].view(torch.int16) == 0).all()
    assert (w1[:, 6, 0, :, 4:].view(torch.int16) == 0).all()
    # freshly allocated outputs give the same bits
    fresh = hip.step_prep(W)
    for n, g, w in zip(names, fresh, want):
        assert torch.equal(g.view(torch.int16), w.view(torch.int16)), n


@pytest.mark.parametrize("m_rows", [1, 3, 1023, 1024, 4101])
def test_prep_target_cast(dev, hip, m_rows):
    W = _master(dev, 2)
    g = torch.Generator(device=dev).manual_seed(m_rows)
    t64 = torch.randn(m_rows, 1, device=dev, dtype=torch.float64,
                      generator=g) * 1e3
    t64[0] = -0.0
    out = hip.step_prep(W, t64)[6]
    assert out.dtype == torch.float32 and out.shape == (m_rows,)
    assert torch.equal(out, t64.float().view(-1))
    flat64 = t64.view(-1)
    assert torch.equal(hip.step_prep(W, flat64)[6], flat64.float())
    t32 = t64.float()
    assert torch.equal(hip.step_prep(W, t32)[6], t32.float().view(-1))
    assert torch.equal(hip.step_prep(W, t32.view(-1))[6], t32.view(-1))


# ---------------------------------------------------------------------
# finalize
# ---------------------------------------------------------------------

_OUT_SHAPES = [(512, 100), (256, 512), (128, 256), (1, 128), (512,),
               (256,), (128,), (1,)]


def _int_parts(dev, ns, db_rows, loss_n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)

    def ri(*shape):
        return torch.randint(
            -8, 9, shape, device=dev, generator=g
        ).float()

    return (ri(ns[0], 512 * 128), ri(ns[1], 256 * 512),
            ri(ns[2], 128 * 256), ri(db_rows, 1156), ri(loss_n))


def _fin_oracle(p1, p2, p3, dbp, lp, M):
    s = dbp.sum(0)
    return [
        lp.sum() / M,
        p1.sum(0).view(512, 128)[:, :100].contiguous(),
        p2.sum(0).view(256, 512),
        p3.sum(0).view(128, 256),
        (s[897:1025] + s[1025:1153]).view(1, 128),
        s[:512], s[512:768], s[768:896], s[896:897],
    ]


def _nan_outs(dev):
    return [torch.full(s, float("nan"), device=dev) for s in _OUT_SHAPES]


def _check_fin(got, want):
    names = ["loss", "dW1", "dW2", "dW3", "dW4", "db1", "db2", "db3",
             "db4"]
    for n, g, w in zip(names, got, want):
        assert g.shape == w.shape, (n, g.shape, w.shape)
        assert torch.isfinite(g).all(), n
        assert torch.equal(g, w), (n, (g - w).abs().max().item())


@pytest.mark.parametrize(
    "ns,db_rows,loss_n",
    [
        ((1, 1, 1), 1, 1),
        ((3, 5, 8), 3, 5),
        ((5, 8, 3), 65, 257),
        ((8, 3, 1), 8, 8),
        ((128, 128, 256), 7813, 7813),  # flagship M=250k
    ],
)
def test_finalize_integer_partials(dev, hip, ns, db_rows, loss_n):
    """Small-integer partials sum exactly in any order, so the outputs
    must equal part.sum(0) bit for bit. NaN sits in every pad column and
    in the pre-filled outputs: none of it may survive."""
    p1, p2, p3, dbp, lp = _int_parts(dev, ns, db_rows, loss_n, sum(ns))
    p1.view(-1, 512, 128)[:, :, 100:] = float("nan")
    dbp[:, 1153:] = float("nan")
    # A power-of-two M keeps sum / M exact, so the oracle does not depend
    # on whether torch divides or multiplies by the reciprocal.
    M = 4096
    clean1 = torch.nan_to_num(p1, nan=0.0)
    cleandb = torch.nan_to_num(dbp, nan=0.0)
    want = _fin_oracle(clean1, p2, p3, cleandb, lp, M)
    outs = _nan_outs(dev)
    got = hip.step_finalize(p1, p2, p3, dbp, lp, M, outs)
    for g, o in zip(got[1:], outs):
        assert g.data_ptr() == o.data_ptr()
    _check_fin(got, want)
    # dW4 is the two-halves sum, loss is sum / M
    s = cleandb.sum(0)
    assert torch.equal(got[4].view(-1), s[897:1025] + s[1025:1153])
    assert torch.equal(got[0], lp.sum() / M)
    # freshly allocated outputs
    _check_fin(hip.step_finalize(p1, p2, p3, dbp, lp, M), want)


@pytest.mark.parametrize("ns,db_rows", [((5, 8, 3), 129), ((16, 16, 32), 513)])
def test_finalize_is_deterministic(dev, hip, ns, db_rows):
    """Fixed summation order: two calls on the same random (non-integer)
    partials agree bit for bit, and track the fp64 column sums."""
    g = torch.Generator(device=dev).manual_seed(7)
    shapes = [(ns[0], 512 * 128), (ns[1], 256 * 512), (ns[2], 128 * 256),
              (db_rows, 1156), (db_rows,)]
    parts = [torch.randn(s, device=dev, generator=g) for s in shapes]
    M = 32 * db_rows
    a = hip.step_finalize(*parts, M)
    b = hip.step_finalize(*parts, M, _nan_outs(dev))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    want = _fin_oracle(*[p.double() for p in parts], M)
    for x, w in zip(a, want):
        # fp32 sum of n terms vs fp64: n * eps * max|term sum| is ample
        tol = 1e-5 * w.abs().max().item() + 1e-5
        assert (x.double() - w).abs().max().item() <= tol


# ---------------------------------------------------------------------
# whole step
# ---------------------------------------------------------------------


def _flat_grad_views(model, dev):
    """One flat buffer, [W1, W2, W3, W4, b1..b4], .grad = views of it."""
    ws = [p for n, p in model.named_parameters() if n.endswith("weight")]
    bs = [p for n, p in model.named_parameters() if n.endswith("bias")]
    ordered = ws + bs
    flat = torch.zeros(sum(p.numel() for p in ordered), device=dev)
    off = 0
    for p in ordered:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    model._rsdl_flat_grads = True
    return flat


def _step(model, x, t, native, grad_hook=None):
    from ray_shuffling_data_loader_amd.models import fused_step as fs

    orig = fs._NATIVE_GLUE
    try:
        fs._NATIVE_GLUE = native
        return fs.fused_step(model, x, t, grad_hook=grad_hook)
    finally:
        fs._NATIVE_GLUE = orig


def _assert_grads_close(model, ref, tag):
    for (n, p), (_, q) in zip(
        model.named_parameters(), ref.named_parameters()
    ):
        assert p.grad.shape == q.grad.shape == p.shape, (tag, n)
        tol = 1e-5 * q.grad.abs().max().item() + 1e-5
        err = (p.grad - q.grad).abs().max().item()
        print(f"{tag} {n}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (tag, n, err, tol)


@pytest.mark.parametrize("m_rows", [1, 31, 33, 4097, 8215])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64])
def test_native_step_matches_composed(dev, hip, m_rows, tdtype):
    """Both paths feed the chain and wgrad kernels bit-identical inputs;
    only the order of the fp32 partial sums differs."""
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    assert hasattr(hip, "fused_step_bf16")
    torch.manual_seed(100 + m_rows)
    m_nat = TabularMLP(100).to(dev)
    m_cmp = copy.deepcopy(m_nat)
    x = torch.randn(m_rows, 100, device=dev).bfloat16()
    t = torch.randn(m_rows, 1, device=dev).to(tdtype)
    l_cmp = _step(m_cmp, x, t, native=False)
    l_nat = _step(m_nat, x, t, native=True)
    print(f"M={m_rows} loss native {l_nat.item()} composed {l_cmp.item()}")
    assert l_nat.dtype == torch.float32 and l_nat.dim() == 0
    assert torch.allclose(l_nat, l_cmp, rtol=1e-5, atol=0.0)
    _assert_grads_close(m_nat, m_cmp, f"M={m_rows}")
    # a second native call gives the same bits (fixed summation order)
    m_two = copy.deepcopy(m_cmp)
    for p in m_two.parameters():
        p.grad = None
    l_two = _step(m_two, x, t, native=True)
    assert torch.equal(l_two, l_nat)
    for p, q in zip(m_two.parameters(), m_nat.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_native_step_flat_grads_in_place(dev, hip):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(5)
    M = 4097
    m_plain = TabularMLP(100).to(dev)
    m_flat = copy.deepcopy(m_plain)
    flat = _flat_grad_views(m_flat, dev)
    flat.fill_(float("nan"))
    ptrs = [p.grad.data_ptr() for p in m_flat.parameters()]
    x = torch.randn(M, 100, device=dev).bfloat16()
    t = torch.randn(M, 1, device=dev)
    l_plain = _step(m_plain, x, t, native=True)
    l_flat = _step(m_flat, x, t, native=True)
    assert torch.equal(l_plain, l_flat)
    assert [p.grad.data_ptr() for p in m_flat.parameters()] == ptrs
    for p, q in zip(m_flat.parameters(), m_plain.parameters()):
        assert torch.equal(p.grad, q.grad)
    assert torch.isfinite(flat).all()


def test_grad_hook_stages_take_composed_path(dev, hip):
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(6)
    M = 4097
    m_ref = TabularMLP(100).to(dev)
    m_hook = copy.deepcopy(m_ref)
    _flat_grad_views(m_hook, dev)
    x = torch.randn(M, 100, device=dev).bfloat16()
    t = torch.randn(M, 1, device=dev)
    stages = []
    l_ref = _step(m_ref, x, t, native=False)
    l_hook = _step(m_hook, x, t, native=True, grad_hook=stages.append)
    assert stages == ["bias", "w1", "w2", "w3"]
    assert torch.allclose(l_hook, l_ref, rtol=1e-5, atol=0.0)
    _assert_grads_close(m_hook, m_ref, "grad_hook")


def test_native_step_launch_count(dev, hip):
    """One warmed native step: at most 8 device kernels (prep, x swizzle,
    fwd, bwd, three wgrads, finalize), no memcpy, no memset."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    torch.manual_seed(8)
    M = 8215
    model = TabularMLP(100).to(dev)
    x = torch.randn(M, 100, device=dev).bfloat16()
    t = torch.randn(M, 1, device=dev)
    for _ in range(3):
        _step(model, x, t, native=True)
    torch.cuda.synchronize()
    with profile(
        activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]
    ) as prof:
        _step(model, x, t, native=True)
        torch.cuda.synchronize()
    devs = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    names = [e.name for e in devs]
    print("device events:", names)
    copies = [n for n in names
              if "memcpy" in n.lower() or "memset" in n.lower()]
    kernels = [n for n in names if n not in copies]
    assert copies == [], copies
    assert 1 <= len(kernels) <= 8, kernels
    assert any("step_prep" in n for n in kernels), kernels
    assert any("step_finalize" in n for n in kernels), kernels
