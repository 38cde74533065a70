"""GPU tests of the LDS-ring fragment wgrad kernel (csrc/wgrad_frag.hip,
wgrad_lds_kernel) against the direct kernel it must match bit for bit."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# Ring depth the kernel ships with (kLdsStages in csrc/wgrad_frag.hip).
S = 6
DIRECT, LDS = 1, 2

# Every (N, K, nt_w, kt_w) the launcher dispatches to the ring kernel.
SHAPES = [(256, 512, 1, 8), (128, 256, 1, 8), (512, 128, 2, 4)]

# 1, 2: one-chunk slabs (nslabs clamps to mchunks) and whole workgroups
# that return early; S-1 .. 2S+1: around the prologue/steady/drain seams
# of the ring; 1021: 8-chunk slabs with a short last slab; 4099: a slab
# count that is no multiple of 8 (XCD decode padding).
MCHUNKS = [1, 2, S - 1, S, S + 1, 2 * S + 1, 1021, 4099]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(mchunks):
    """Random bf16 dz / src [M, 512] with M = 16 * mchunks - 5 rows (the
    zero-padded tail of the last chunk is exercised); shapes take column
    slices. Built once per mchunks and never modified."""
    g = torch.Generator(device="cuda").manual_seed(1000 + mchunks)
    m = 16 * mchunks - 5
    dz = torch.randn(m, 512, device="cuda", generator=g).bfloat16()
    src = torch.randn(m, 512, device="cuda", generator=g).bfloat16()
    return dz, src


def _frags(mchunks, n, k):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import t_frag_swizzle

    dz, src = _inputs(mchunks)
    dz, src = dz[:, :n].contiguous(), src[:, :k].contiguous()
    return dz, src, t_frag_swizzle(dz), t_frag_swizzle(src)


@pytest.mark.parametrize("mchunks", MCHUNKS)
@pytest.mark.parametrize("n,k,nt_w,kt_w", SHAPES)
def test_partials_bit_equal(dev, n, k, nt_w, kt_w, mchunks):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    hip = _load_hip()
    _, _, at_f, bt_f = _frags(mchunks, n, k)
    ref = hip.wgrad_frag_partials_bf16(at_f, bt_f, n, k, mchunks, nt_w,
                                       kt_w, variant=DIRECT)
    got = hip.wgrad_frag_partials_bf16(at_f, bt_f, n, k, mchunks, nt_w,
                                       kt_w, variant=LDS)
    assert got.shape == ref.shape and ref.shape[1] == n * k
    assert torch.equal(got, ref), (
        n, k, mchunks, (got != ref).sum().item())


@pytest.mark.parametrize("n,k,nt_w,kt_w", SHAPES)
def test_lds_matches_fp64(dev, n, k, nt_w, kt_w):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import wgrad_frag

    mchunks = 1021
    dz, src, at_f, bt_f = _frags(mchunks, n, k)
    m = dz.shape[0]
    dw = wgrad_frag(at_f, bt_f, n, k, mchunks, variant=LDS)
    ref = dz.double().t() @ src.double()
    # the bound of test_wgrad_frag_matches_reference
    eps32 = 2.0 ** -24
    tol = 8 * math.log2(m) * eps32 * (2 / math.pi) * m
    err = (dw.double() - ref).abs().max().item()
    assert err <= tol, (n, k, m, err, tol)


def test_variant_checked(dev):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    hip = _load_hip()
    _, _, at_f, bt_f = _frags(2, 256, 512)
    with pytest.raises(RuntimeError, match="variant"):
        hip.wgrad_frag_partials_bf16(at_f, bt_f, 256, 512, 2, 1, 8,
                                     variant=3)
    with pytest.raises(RuntimeError, match="LDS-ring"):
        hip.wgrad_frag_partials_bf16(at_f, bt_f, 256, 512, 2, 1, 4,
                                     variant=LDS)


@pytest.mark.parametrize("m", [1000, 64 * 3 + 5])
def test_whole_step_bit_equal(dev, monkeypatch, m):
    """fused_step through hip.fused_step_bf16 with the ring kernel forced
    on for all three wgrads, and forced off: same loss, same gradients."""
    from ray_shuffling_data_loader_amd.models import fused_step as fs
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    hip = _load_hip()
    torch.manual_seed(7)
    model = TabularMLP(100).to(dev)
    x = torch.randn(m, 100, device=dev).bfloat16()
    t = torch.randn(m, 1, device=dev)
    monkeypatch.setattr(fs, "_NATIVE_GLUE", True)
    assert fs._native_ok(hip, fs._layers(model), x, t, None)

    def run(variant):
        monkeypatch.setattr(fs, "_WGRAD_VARIANT", variant)
        for p in model.parameters():
            p.grad = None
        loss = fs.fused_step(model, x, t)
        return [loss.clone()] + [
            p.grad.clone() for p in model.parameters()]

    off, on = run(DIRECT), run(LDS)
    assert len(on) == 9
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), (m, i)
