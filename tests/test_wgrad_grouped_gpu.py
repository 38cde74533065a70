"""GPU tests of the grouped wgrad launch (csrc/wgrad_frag.hip,
wgrad_grouped_kernel): dW1, dW2 and dW3 of the train step as one launch.

The inputs are integer-valued bf16 with |entries| <= 4, so the magnitudes
of the terms of any accumulator sum to at most 16 * 20000 < 2^24: every
fp32 partial and every sum of partials is exact in any order, and is
compared with torch.equal against an fp64 oracle."""

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _exact_cases import int_matrix  # noqa: E402

pytestmark = pytest.mark.gpu

# M -> mchunks = 2 * ceil(M / 32): 2 (fewer chunks than any slab target), 8
# (one chunk per slab, prologue shorter than the ring), 130 (one and two
# chunks per slab, a short last slab), 514 (chunks per slab on both sides of
# the ring depth; the drain switch), 1250 (the steady loop everywhere).
SHAPES = [1, 97, 2049, 8215, 20000]

# (N, K, nt_w, kt_w) of dW1 (x padded to 128 columns), dW2, dW3
PROBLEMS = [(512, 128, 2, 4), (256, 512, 1, 8), (128, 256, 1, 8)]


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    h = _load_hip()
    assert hasattr(h, "wgrad_grouped_partials_bf16")
    return h


def _mchunks(m):
    return 2 * ((m + 31) // 32)


@functools.lru_cache(maxsize=None)
def _case(m):
    """Per problem (dz [Mp, N], src [Mp, K]) bf16 on the GPU, Mp = 16 *
    mchunks rows of which the first m are drawn and the rest zero, and the
    six fragment tensors in the binding's order. Read-only."""
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import t_frag_swizzle

    mp = 16 * _mchunks(m)
    mats, frags = [], []
    for i, (n, k, _, _) in enumerate(PROBLEMS):
        kreal = 100 if i == 0 else k
        dz = torch.zeros(mp, n, dtype=torch.bfloat16)
        src = torch.zeros(mp, k, dtype=torch.bfloat16)
        dz[:m] = int_matrix(m, n, 7000 + 10 * i + m)
        src[:m, :kreal] = int_matrix(m, kreal, 7005 + 10 * i + m)
        dz, src = dz.cuda(), src.cuda()
        mats.append((dz, src))
        frags += [t_frag_swizzle(dz), t_frag_swizzle(src)]
    return mats, frags


@functools.lru_cache(maxsize=None)
def _grouped(m):
    """(part1, part2, part3) of one grouped launch. Read-only."""
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    _, frags = _case(m)
    parts = _load_hip().wgrad_grouped_partials_bf16(*frags, _mchunks(m))
    torch.cuda.synchronize()
    return parts


def _slab_oracle(dz, src, ns, cps):
    """[ns, N*K] fp64: dz[rows of slab s]^T @ src[rows of slab s]."""
    rows = ns * cps * 16
    n, k = dz.shape[1], src.shape[1]
    a = torch.zeros(rows, n, dtype=torch.float64, device=dz.device)
    b = torch.zeros(rows, k, dtype=torch.float64, device=dz.device)
    a[:dz.shape[0]] = dz.double()
    b[:src.shape[0]] = src.double()
    a = a.view(ns, cps * 16, n)
    b = b.view(ns, cps * 16, k)
    return torch.bmm(a.transpose(1, 2), b).reshape(ns, n * k)


@pytest.mark.parametrize("m", SHAPES)
def test_partials_per_slab_exact(hip, m):
    mchunks = _mchunks(m)
    mats, _ = _case(m)
    parts = _grouped(m)
    assert len(parts) == 3
    for i, ((n, k, _, _), (dz, src), part) in enumerate(
            zip(PROBLEMS, mats, parts)):
        assert part.dtype == torch.float32 and part.dim() == 2
        assert part.shape[1] == n * k
        ns = part.shape[0]
        assert 1 <= ns <= mchunks
        cps = -(-mchunks // ns)
        # no empty slab: the count is the one the chunks per slab imply
        assert ns == -(-mchunks // cps), (m, i, ns, cps)
        ref = _slab_oracle(dz, src, ns, cps)
        assert ref.abs().max().item() < 2 ** 24
        assert torch.equal(part.double(), ref), (
            m, i, ns, cps, (part.double() != ref).sum().item())


@pytest.mark.parametrize("m", SHAPES)
def test_summed_partials_exact(hip, m):
    mats, _ = _case(m)
    for (n, k, _, _), (dz, src), part in zip(PROBLEMS, mats, _grouped(m)):
        ref = dz.double().t() @ src.double()
        got = part.double().sum(0).view(n, k)
        assert torch.equal(got, ref), (m, n, k)


@pytest.mark.parametrize("m", SHAPES)
def test_sums_equal_separate_launches(hip, m):
    mchunks = _mchunks(m)
    _, frags = _case(m)
    for i, ((n, k, nt_w, kt_w), part) in enumerate(
            zip(PROBLEMS, _grouped(m))):
        old = hip.wgrad_frag_partials_bf16(frags[2 * i], frags[2 * i + 1],
                                           n, k, mchunks, nt_w, kt_w)
        assert torch.equal(part.double().sum(0), old.double().sum(0)), (m, i)


def test_two_launches_same_bits(hip):
    _, frags = _case(2049)
    again = hip.wgrad_grouped_partials_bf16(*frags, _mchunks(2049))
    for a, b in zip(again, _grouped(2049)):
        assert torch.equal(a, b)


def test_inputs_checked(hip):
    _, frags = _case(97)
    with pytest.raises(RuntimeError, match="numel"):
        hip.wgrad_grouped_partials_bf16(*frags, _mchunks(97) + 1)
    with pytest.raises(RuntimeError, match="mchunks"):
        hip.wgrad_grouped_partials_bf16(*frags, 0)


@pytest.mark.parametrize("m", [33, 4097])
def test_whole_step_grouped_on_off(hip, monkeypatch, m):
    """fused_step through hip.fused_step_bf16 with the grouped launch on
    and off: everything but dW1-dW3 bit for bit, those three within the
    bound the suite allows regrouped fp32 sums, and two grouped runs bit
    for bit."""
    from ray_shuffling_data_loader_amd.models import fused_step as fs
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    model = TabularMLP(100).to(dev)
    x = torch.randn(m, 100, device=dev).bfloat16()
    t = torch.randn(m, 1, device=dev)
    monkeypatch.setattr(fs, "_NATIVE_GLUE", True)
    monkeypatch.setattr(fs, "_WGRAD_VARIANT", 0)
    lin = fs._layers(model)
    assert fs._native_ok(hip, lin, x, t, None)

    def run(grouped):
        monkeypatch.setattr(fs, "_WGRAD_GROUPED", grouped)
        for p in model.parameters():
            p.grad = None
        loss = fs.fused_step(model, x, t)
        return ([loss.clone()] + [q.weight.grad.clone() for q in lin]
                + [q.bias.grad.clone() for q in lin])

    on, off, on2 = run(True), run(False), run(True)
    assert len(on) == 9
    for i, (a, b) in enumerate(zip(on, on2)):
        assert torch.equal(a, b), (m, i)
    for i in (0, 4, 5, 6, 7, 8):  # loss, dW4, db1-db4
        assert torch.equal(on[i], off[i]), (m, i)
    for i in (1, 2, 3):  # dW1-dW3
        tol = 1e-5 * off[i].abs().max().item() + 1e-5
        err = (on[i] - off[i]).abs().max().item()
        assert err <= tol, (m, i, err, tol)
