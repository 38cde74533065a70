"""GPU tests that pin the fused chain, wgrad and finalize kernels
(csrc/fwd_chain.hip, csrc/bwd_chain.hip, csrc/wgrad_frag.hip,
csrc/step_glue.hip) and the older GEMM kernels (csrc/wgrad_kernel.hip,
csrc/wgrad_wide.hip, csrc/relu_bwd.hip) to an exact fp64 oracle.

The inputs are the integer-valued cases of tests/_exact_cases.py, for which
every fp32 accumulator holds the mathematically exact value in any
summation order (tests/test_exact_cases.py proves the precondition on the
CPU). The only inexact operation left is the round-to-nearest-even bf16
conversion of an exactly known number, so every comparison below is
``torch.equal`` against the oracle: no tolerance, and nothing compared with
a sibling kernel. bf16 tensors are compared as bit patterns with -0
folded into +0 (the sign of a zero is not part of the mathematics).

Integers do not exercise fractional exponents; section 4 runs one dense
random pass under a bound derived from the number formats alone.
"""

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu

REGIMES = list(ec.REGIMES)
ROWS = (32, 64)
PI16 = (False, True)
DIRECT, LDS = 1, 2
FWD_NAMES = ["a1t", "mask1", "a2t", "mask2", "a3", "out", "dyb", "loss_part"]
BWD_NAMES = ["dz1t", "dz2t", "dz3t", "db1", "db2", "db3", "db4", "dw4"]
STEP_NAMES = ["loss", "dW1", "dW2", "dW3", "dW4", "db1", "db2", "db3", "db4"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    return shuffle_ops._load_hip()


@functools.lru_cache(maxsize=None)
def _case(name, M):
    """(case on the GPU, CPU oracle). Built once; never modified."""
    case = ec.make_case(name, M)
    on = {k: (v.cuda() if torch.is_tensor(v) else v)
          for k, v in case.items()}
    return on, ec.reference(case)


@functools.lru_cache(maxsize=None)
def _fused_ref(name, M):
    case = ec.make_case(name, M)
    return ec.reference(case, ec.fused_dy(case))


def _bits(t):
    """bf16 -> int16 bit patterns, -0 folded into +0."""
    assert t.dtype == torch.bfloat16
    return (t.float() + 0.0).bfloat16().contiguous().view(torch.int16)


def _eq_bf16(got, ref, what):
    ref = ref.to(got.device)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    g, r = _bits(got), _bits(ref)
    assert torch.equal(g, r), (
        what, int((g != r).sum()), got[g != r][:4].tolist(),
        ref[g != r][:4].tolist())


def _eq_f32(got, ref64, what):
    """fp32 kernel output against an exactly representable fp64 value."""
    assert got.dtype == torch.float32, what
    ref = ref64.to(got.device).reshape(got.shape)
    assert torch.equal(ref.float().double(), ref), what  # fp32-exact oracle
    bad = got.double() != ref
    assert not bool(bad.any()), (
        what, int(bad.sum()), got[bad][:4].tolist(), ref[bad][:4].tolist())


def _valid_words(M, dev):
    """Per m-tile word with the bits of the rows < M set (pad rows carry
    arbitrary bits; their dz is zero regardless)."""
    mt = (M + 31) // 32
    valid = torch.full((mt,), 0xFFFFFFFF, dtype=torch.int64, device=dev)
    if M % 32:
        valid[M // 32] = (1 << (M % 32)) - 1
    return valid.view(-1, 1)


def _eq_mask(got, alive, M, what):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import relu_mask_words

    ref = relu_mask_words(alive.to(got.device).float())
    valid = _valid_words(M, got.device)
    g = (got.to(torch.int64) & 0xFFFFFFFF) & valid
    r = (ref.to(torch.int64) & 0xFFFFFFFF) & valid
    assert torch.equal(g, r), (what, int((g != r).sum()))


def _unsw(flat, M, c, pi16):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
        t_frag_unswizzle,
    )

    return t_frag_unswizzle(flat, M, c, pi16)


# ---------------------------------------------------------------------
# 1. the chain kernels, run once per key
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd(hip):
    cache = {}

    def run(name, M, rows, pi16):
        key = (name, M, rows, pi16)
        if key not in cache:
            c, _ = _case(name, M)
            mchunks = 2 * ((M + 31) // 32)
            xt = torch.empty(4 * mchunks * 512, dtype=torch.bfloat16,
                             device=c["x"].device)
            res = hip.fwd_chain_bf16(
                c["x"], c["W1"], c["b1"], c["W2"], c["b2"], c["W3"],
                c["b3"], c["w4"], c["b4"], target=c["target"], xt_out=xt,
                pi16=pi16, rows=rows,
            )
            out = dict(zip(FWD_NAMES, res))
            out["xt"] = xt
            cache[key] = out
        return cache[key]

    return run


@pytest.fixture(scope="module")
def bwd_on_fwd(hip, fwd):
    """The backward on the forward kernel's own a3 and mask words and the
    case's integer dy (the staged whole step)."""
    cache = {}

    def run(name, M, rows, pi16):
        key = (name, M, rows, pi16)
        if key not in cache:
            c, _ = _case(name, M)
            f = fwd(name, M, rows, pi16)
            res = hip.bwd_chain_bf16(
                c["dy"], f["a3"], f["mask1"], f["mask2"], c["w4"], c["W3"],
                c["W2"], pi16=pi16, rows=rows,
            )
            cache[key] = dict(zip(BWD_NAMES, res))
        return cache[key]

    return run


@pytest.mark.parametrize("pi16", PI16)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", ec.SHAPES)
@pytest.mark.parametrize("name", REGIMES)
def test_forward_equals_oracle(fwd, name, M, rows, pi16):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import t_frag_swizzle

    c, ref = _case(name, M)
    f = fwd(name, M, rows, pi16)
    _eq_bf16(_unsw(f["a1t"], M, 512, pi16), ref["a1"], "a1t")
    _eq_bf16(_unsw(f["a2t"], M, 256, pi16), ref["a2"], "a2t")
    _eq_bf16(f["a3"], ref["a3"], "a3")
    _eq_bf16(f["out"], ref["out"], "out")
    _eq_mask(f["mask1"], ref["mask1"], M, "mask1")
    _eq_mask(f["mask2"], ref["mask2"], M, "mask2")
    mp = (M + 31) // 32 * 32
    xt = t_frag_swizzle(
        torch.nn.functional.pad(c["x"], (0, 28, 0, mp - M)), pi16)
    assert torch.equal(f["xt"].view(torch.int16), xt.view(torch.int16))
    assert f["loss_part"].numel() == (M + rows - 1) // rows
    if M in ec.HEAD_SHAPES:
        # 2/M, (2/M) d and every d^2 are exact
        dy = ec.fused_dy(ec.make_case(name, M))
        _eq_bf16(f["dyb"], dy, "dyb")
        _eq_f32(f["loss_part"], ec.slab_sums(ref["loss_terms"], rows),
                "loss_part")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", ec.SHAPES)
@pytest.mark.parametrize("name", REGIMES)
def test_eval_equals_oracle(hip, name, M, rows):
    """pred is the head value before its bf16 rounding, in fp32; partial
    columns 1-3 are the per-slab sums of |o - t|, t and t^2 on the small
    integer eval_target (column 0, sum (o - t)^2, passes 2^24 and is left
    to tests/test_fused_eval_gpu.py)."""
    c, ref = _case(name, M)
    st = hip.step_prep([c["W1"].float(), c["W2"].float(), c["W3"].float(),
                        c["w4"].float().reshape(1, 128)])
    pred, part = hip.eval_chain_bf16(
        c["x"], [st[0], st[1], st[2], st[5]],
        [c["b1"], c["b2"], c["b3"], c["b4"]], target=c["eval_target"],
        rows=rows)
    assert pred.dtype == torch.float32 and pred.shape == (M,)
    assert torch.equal(pred, ref["out_fp32"].to(pred.device))
    o = ref["out_fp32"].double()
    t = ec.make_case(name, M)["eval_target"].double()
    assert part.shape == ((M + rows - 1) // rows, 4)
    _eq_f32(part[:, 1].contiguous(), ec.slab_sums((o - t).abs(), rows),
            "sum |o - t|")
    _eq_f32(part[:, 2].contiguous(), ec.slab_sums(t, rows), "sum t")
    _eq_f32(part[:, 3].contiguous(), ec.slab_sums(t * t, rows), "sum t^2")


@pytest.mark.parametrize("pi16", PI16)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", ec.SHAPES)
@pytest.mark.parametrize("name", REGIMES)
def test_backward_equals_oracle(hip, dev, name, M, rows, pi16):
    """Fed the ORACLE's a3 and mask words, never the GPU forward's, so a
    forward slip cannot mask a backward one. The binding reduces the db
    partials with atomics; integer sums do not depend on the order."""
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import relu_mask_words

    c, ref = _case(name, M)
    res = hip.bwd_chain_bf16(
        c["dy"], ref["a3"].to(dev),
        relu_mask_words(ref["a1"].to(dev).float()),
        relu_mask_words(ref["a2"].to(dev).float()),
        c["w4"], c["W3"], c["W2"], pi16=pi16, rows=rows,
    )
    b = dict(zip(BWD_NAMES, res))
    _eq_bf16(_unsw(b["dz1t"], M, 512, pi16), ref["dz1"], "dz1t")
    _eq_bf16(_unsw(b["dz2t"], M, 256, pi16), ref["dz2"], "dz2t")
    _eq_bf16(_unsw(b["dz3t"], M, 128, pi16), ref["dz3"], "dz3t")
    for k in ("db1", "db2", "db3", "db4"):
        _eq_f32(b[k].contiguous(), ref[k], k)
    _eq_f32(b["dw4"].contiguous(), ref["dW4"], "dw4")


# ---------------------------------------------------------------------
# 2. fragment wgrad, both kernels, against dz^T @ src
# ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wgrad_inputs(mchunks):
    m = 16 * mchunks - 5
    return (ec.int_matrix(m, 512, seed=2000 + mchunks).cuda(),
            ec.int_matrix(m, 512, seed=3000 + mchunks).cuda())


@pytest.mark.parametrize("variant", [DIRECT, LDS])
@pytest.mark.parametrize("mchunks", ec.WGRAD_MCHUNKS)
@pytest.mark.parametrize("n,k,nt_w,kt_w", ec.WGRAD_SHAPES)
def test_wgrad_frag_equals_oracle(hip, n, k, nt_w, kt_w, mchunks, variant):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
        t_frag_swizzle,
        wgrad_frag,
    )

    dz, src = _wgrad_inputs(mchunks)
    dz, src = dz[:, :n].contiguous(), src[:, :k].contiguous()
    at_f, bt_f = t_frag_swizzle(dz), t_frag_swizzle(src)
    ref = dz.double().t() @ src.double()
    part = hip.wgrad_frag_partials_bf16(at_f, bt_f, n, k, mchunks, nt_w,
                                        kt_w, variant=variant)
    assert part.shape[1] == n * k
    assert torch.equal(part.double().sum(0).view(n, k), ref), (
        n, k, mchunks, variant)
    dw = wgrad_frag(at_f, bt_f, n, k, mchunks, variant=variant)
    _eq_f32(dw, ref, ("wgrad_frag", n, k, mchunks, variant))


# ---------------------------------------------------------------------
# 3. the whole step: staged through the bindings, then the one call
# ---------------------------------------------------------------------
def _db_part_row(b):
    """One db_part row (db1 | db2 | db3 | db4 | dW4 half 0 | half 1 | pad)
    from the backward binding's reduced outputs, the layout step_finalize
    reads (kPartWPad = 1156 floats)."""
    row = torch.zeros(1, 1156, dtype=torch.float32, device=b["db1"].device)
    row[0, 0:512] = b["db1"]
    row[0, 512:768] = b["db2"]
    row[0, 768:896] = b["db3"]
    row[0, 896] = b["db4"][0]
    row[0, 897:1025] = b["dw4"].reshape(-1)
    return row


@pytest.mark.parametrize("variant", [DIRECT, LDS])
@pytest.mark.parametrize("pi16", PI16)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", ec.SHAPES)
@pytest.mark.parametrize("name", REGIMES)
def test_staged_step_equals_oracle(hip, fwd, bwd_on_fwd, name, M, rows, pi16,
                                   variant):
    """fwd_chain -> bwd_chain -> three fragment wgrads on the kernels' own
    emitted fragments -> step_finalize, wired as fused_step_bf16 wires
    them."""
    _, ref = _case(name, M)
    f = fwd(name, M, rows, pi16)
    b = bwd_on_fwd(name, M, rows, pi16)
    mchunks = 2 * ((M + 31) // 32)
    p1 = hip.wgrad_frag_partials_bf16(b["dz1t"], f["xt"], 512, 128, mchunks,
                                      2, 4, variant=variant)
    p2 = hip.wgrad_frag_partials_bf16(b["dz2t"], f["a1t"], 256, 512, mchunks,
                                      1, 8, variant=variant)
    p3 = hip.wgrad_frag_partials_bf16(b["dz3t"], f["a2t"], 128, 256, mchunks,
                                      1, 8, variant=variant)
    got = dict(zip(STEP_NAMES, hip.step_finalize(
        p1, p2, p3, _db_part_row(b), f["loss_part"], M)))
    for k in STEP_NAMES[1:]:
        _eq_f32(got[k], ref[k], k)
    if M in ec.HEAD_SHAPES:
        _eq_f32(got["loss"], ref["loss"], "loss")


@pytest.mark.parametrize("variant", [DIRECT, LDS])
@pytest.mark.parametrize("pi16", PI16)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("M", ec.FUSED_SHAPES)
@pytest.mark.parametrize("name", REGIMES)
def test_fused_step_equals_oracle(hip, name, M, rows, pi16, variant):
    """hip.fused_step_bf16 itself: dy = (2/M) d is exact at these M."""
    c, _ = _case(name, M)
    ref = _fused_ref(name, M)
    got = dict(zip(STEP_NAMES, hip.fused_step_bf16(
        c["x"], c["target"],
        [c["W1"].float(), c["W2"].float(), c["W3"].float(),
         c["w4"].float().reshape(1, 128)],
        [c["b1"], c["b2"], c["b3"], c["b4"]],
        pi16=pi16, rows=rows, wgrad_variant=variant)))
    for k in STEP_NAMES:
        _eq_f32(got[k], ref[k], k)


# ---------------------------------------------------------------------
# 4. real-valued data under a bound derived from the formats
# ---------------------------------------------------------------------
def _dense_data(dev):
    """The seeded N(0,1)-scaled fixture of tests/test_chain_rows64_gpu.py
    (same generator, same draws) at M = 161."""
    g = torch.Generator(device="cpu").manual_seed(64)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    Ws = [
        (rn(512, 100) / 10).bfloat16(),
        (rn(256, 512) / 22).bfloat16(),
        (rn(128, 256) / 16).bfloat16(),
        (rn(1, 128) / 11).bfloat16(),
    ]
    bs = [(rn(n) / 4).bfloat16().float() for n in (512, 256, 128, 1)]
    return Ws, bs, rn(161, 100).bfloat16(), rn(161, 1)


def _mask_bits(mask, M):
    """[mtiles, N] int32 mask words -> [M, N] bool."""
    w = mask.to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, device=mask.device, dtype=torch.int64)
    bits = (w.unsqueeze(1) >> sh.view(1, 32, 1)) & 1
    return bits.reshape(-1, mask.shape[1])[:M].bool()


def _stage_check(name, got, ref64, k, absum):
    """|got - ref64| <= 2^-8 |ref64| + (K + 2) 2^-24 (sum_k |a w| + |b|):
    half a bf16 ulp (bounded above) plus the worst-case error of K fp32
    additions in any order and the bias add. Returns the fp32 term."""
    acc = (k + 2) * 2.0 ** -24 * absum
    bound = 2.0 ** -8 * ref64.abs() + acc
    err = (got.double() - ref64).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f"{name}: max err/bound {ratio:.4f}")
    assert bool((err <= bound).all()), (name, ratio)
    return acc


@pytest.mark.parametrize("rows", ROWS)
def test_dense_random_within_derived_bound(hip, dev, rows):
    """Stage by stage: each stage's fp64 reference is computed from the
    tensors the kernel itself emitted for the previous stage, so the bound
    covers one GEMM and one bf16 conversion, nothing accumulated."""
    M = 161
    Ws, bs, x, tgt = _dense_data(dev)
    W = [w.double() for w in Ws]
    f = dict(zip(FWD_NAMES, hip.fwd_chain_bf16(
        x, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], Ws[3].flatten(), bs[3],
        target=tgt, rows=rows)))
    a1 = _unsw(f["a1t"], M, 512, False)
    a2 = _unsw(f["a2t"], M, 256, False)
    src = x.double()
    for name, got, Wl, b, k, mask in [
            ("a1", a1, W[0], bs[0], 100, f["mask1"]),
            ("a2", a2, W[1], bs[1], 512, f["mask2"]),
            ("a3", f["a3"], W[2], bs[2], 256, None)]:
        z = src @ Wl.t() + b.double()
        absum = src.abs() @ Wl.abs().t() + b.double().abs()
        acc = _stage_check(name, got, torch.relu(z), k, absum)
        if mask is not None:
            bits = _mask_bits(mask, M)
            assert torch.equal(bits, got > 0), name
            sure = z.abs() > acc
            assert torch.equal(bits[sure], (z > 0)[sure]), name
        src = got.double()
    o = src @ W[3].t() + bs[3].double()
    _stage_check("out", f["out"], o, 128,
                 src.abs() @ W[3].abs().t() + bs[3].double().abs())

    b = dict(zip(BWD_NAMES, hip.bwd_chain_bf16(
        f["dyb"], f["a3"], f["mask1"], f["mask2"], Ws[3].flatten(), Ws[2],
        Ws[1], rows=rows)))
    dy = f["dyb"].double().reshape(M, 1)
    dz3 = _unsw(b["dz3t"], M, 128, False)
    dz2 = _unsw(b["dz2t"], M, 256, False)
    dz1 = _unsw(b["dz1t"], M, 512, False)
    live3 = (f["a3"] > 0).double()
    _stage_check("dz3", dz3, dy * W[3] * live3, 1, (dy * W[3]).abs() * live3)
    for name, got, up, Wl, k, mask in [
            ("dz2", dz2, dz3, W[2], 128, f["mask2"]),
            ("dz1", dz1, dz2, W[1], 256, f["mask1"])]:
        bits = _mask_bits(mask, M).double()
        _stage_check(name, got, (up.double() @ Wl) * bits, k,
                     (up.double().abs() @ Wl.abs()) * bits)


# ---------------------------------------------------------------------
# 5. the older GEMM kernels (ChunkedLinear / LinearReLU)
# ---------------------------------------------------------------------
# The dispatcher of wgrad_bf16 (csrc/shuffle_ops.cpp) sends every shape to
# csrc/wgrad_kernel.hip unless RSDL_WGRAD_WIDE is set (read per call); with
# it, M >= 4096 and N, K >= 64 go to csrc/wgrad_wide.hip, whose launcher
# picks one of three tiles by the padded shape:
#   (4099, 512, 100), (4099, 256, 512) -> 256 x 128
#   (4099, 128, 256)                   -> 128 x 256
#   (4099, 64, 64)  (padded to 128^2)  -> 128 x 128
# (255, 128, 256) with the variable set still runs wgrad_kernel.hip
# (M < 4096).
WIDE_SHAPES = [(4099, 512, 100), (4099, 256, 512), (4099, 128, 256),
               (4099, 64, 64), (255, 128, 256)]


def _wgrad_case(hip, m, n, k):
    dy = ec.int_matrix(m, n, seed=41 * m + n).cuda()
    x = ec.int_matrix(m, k, seed=43 * m + k).cuda()
    dw, db = hip.wgrad_bf16(dy, x, True)
    _eq_f32(dw, dy.double().t() @ x.double(), ("dW", m, n, k))
    _eq_f32(db, dy.double().sum(0), ("db", m, n, k))
    dw2, _ = hip.wgrad_bf16(dy, x, False)
    assert torch.equal(dw2, dw)


@pytest.mark.parametrize("m,n,k", ec.GEMM_SHAPES)
def test_wgrad_kernel_equals_oracle(hip, monkeypatch, m, n, k):
    monkeypatch.delenv("RSDL_WGRAD_WIDE", raising=False)
    _wgrad_case(hip, m, n, k)


@pytest.mark.parametrize("m,n,k", WIDE_SHAPES)
def test_wgrad_wide_equals_oracle(hip, monkeypatch, m, n, k):
    monkeypatch.setenv("RSDL_WGRAD_WIDE", "1")
    _wgrad_case(hip, m, n, k)


@pytest.mark.parametrize("m,n", ec.RELU_BWD_SHAPES)
def test_relu_bwd_bias_equals_oracle(hip, m, n):
    dy = ec.int_matrix(m, n, seed=47 * m + n).cuda()
    y = ec.int_matrix(m, n, seed=53 * m + n).cuda()
    dx, db = hip.relu_bwd_bias(dy, y)
    ref = torch.where(y > 0, dy.double(), torch.zeros_like(dy).double())
    _eq_bf16(dx, ref.float().bfloat16(), ("dx", m, n))
    _eq_f32(db, ref.sum(0), ("db", m, n))
