"""CPU conditions for the exact-oracle GPU tests
(tests/test_chain_exact_gpu.py): the integer cases of tests/_exact_cases.py
must be exact in fp32 in any summation order, must exercise the bf16
rounding, and the oracle must agree with the lane-level simulators of
tests/test_chain_sim.py. These are conditions on the inputs, not
measurements of any kernel."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_cases as ec  # noqa: E402

CASES = [(name, M) for name in ec.REGIMES for M in ec.SHAPES]
FUSED = [(name, M) for name in ec.REGIMES for M in ec.FUSED_SHAPES]
EMITTED = ["a1", "a2", "a3", "out", "dz3", "dz2", "dz1"]


def _report(name, M, fused=False):
    case = ec.make_case(name, M)
    if fused:
        ref = ec.reference(case, ec.fused_dy(case))
        return case, ref, ec.exactness_report(case, ref, granule=2.0 / M)
    ref = ec.reference(case)
    return case, ref, ec.exactness_report(case, ref)


@pytest.mark.parametrize("name,M", CASES)
def test_every_sum_is_exact(name, M):
    _, _, rep = _report(name, M)
    for cls, bound in rep["bounds"].items():
        assert bound < ec.LIMIT, (name, M, cls, bound)


@pytest.mark.parametrize("name,M", FUSED)
def test_every_sum_is_exact_fused_step(name, M):
    """The whole fused step feeds its backward dy = (2/M) d: every
    backward quantity is a multiple of the granule 2/M, and the bounds are
    taken in units of it."""
    case, ref, rep = _report(name, M, fused=True)
    g = 2.0 / M
    assert torch.equal(ref["dy"].reshape(-1), g * case["d"])
    for k in ("dz3", "dz2", "dz1", "dz3_pre", "dz2_pre", "dz1_pre"):
        q = ref[k].double() / g
        assert torch.equal(q, q.round()), (name, M, k)
    for cls, bound in rep["bounds"].items():
        assert bound < ec.LIMIT, (name, M, cls, bound)
    # loss = (sum of integer d^2) / M with M a power of two
    assert float(ref["loss"]) == float(torch.tensor(
        float(ref["loss"]), dtype=torch.float32))


@pytest.mark.parametrize("name,M", CASES)
def test_emitted_tensors_are_integers(name, M):
    case, ref, _ = _report(name, M)
    for k in EMITTED + ["z1", "z2", "z3", "dz3_pre", "dz2_pre", "dz1_pre",
                        "out_fp32"]:
        v = ref[k].double()
        assert torch.equal(v, v.round()), (name, M, k)
    for k in ("target", "eval_target"):
        assert torch.equal(case[k], case[k].round()), (name, M, k)
    # the fp32 target holds o - d exactly, so the kernel's diff is d
    assert torch.equal(ref["out_fp32"].double() - case["target"].double(),
                       case["d"])
    assert case["d"].abs().max() <= 8
    for k in ("b1", "b2", "b3", "b4"):
        assert bool((case[k] != 0).all()), (name, M, k)


@pytest.mark.parametrize("M", ec.HEAD_SHAPES)
@pytest.mark.parametrize("name", list(ec.REGIMES))
def test_head_gradient_is_exact(name, M):
    """At M in HEAD_SHAPES 2/M, (2/M) d and its bf16 rounding are exact."""
    case = ec.make_case(name, M)
    dy = ec.fused_dy(case).double().reshape(-1)
    assert torch.equal(dy, (2.0 / M) * case["d"])


@pytest.mark.parametrize("M", ec.SHAPES)
def test_wide_exercises_the_rounding(M):
    _, _, rep = _report("wide", M)
    for k in ("a1", "a2", "a3", "dz2", "dz1"):
        st = rep["rounding"][k]
        assert st["rounded"] >= 0.05, (M, k, st)
        assert st["ties_up"] >= 1 and st["ties_down"] >= 1, (M, k, st)


def test_tie_counter():
    """257 and 259 are ties between (256, 258) and (258, 260): to even,
    i.e. down to 256 and up to 260; 513 is nearer to 512, no tie."""
    pre = torch.tensor([257.0, 259.0, 513.0, 256.0], dtype=torch.float64)
    post = pre.float().bfloat16()
    assert post.tolist() == [256.0, 260.0, 512.0, 256.0]
    st = ec.rounding_stats(pre, post)
    assert (st["ties_down"], st["ties_up"]) == (1, 1)
    assert st["rounded"] == 0.75


@pytest.mark.parametrize("name,M", CASES)
def test_relu_layers_are_half_alive(name, M):
    _, _, rep = _report(name, M)
    for k, share in rep["alive"].items():
        assert 0.25 <= share <= 0.75, (name, M, k, share)


def test_wide_separates_the_two_readings_of_db():
    """Summing dz before or after its bf16 conversion differs in "wide"
    for every layer, so the oracle's choice (before) is a real claim."""
    _, ref, _ = _report("wide", 161)
    for i in (1, 2, 3):
        assert not torch.equal(ref[f"db{i}"], ref[f"db{i}_post"]), i


def test_integer_gemm_operands_are_exact():
    """wgrad_frag / wgrad / relu_bwd_bias cases: entries in [-4, 4], so a
    sum over m rows is bounded by 16 m (4 m for a bias gradient)."""
    m_max = max(16 * max(ec.WGRAD_MCHUNKS) - 5,
                max(s[0] for s in ec.GEMM_SHAPES),
                max(s[0] for s in ec.RELU_BWD_SHAPES))
    assert ec.INT_RANGE ** 2 * m_max < ec.LIMIT
    t = ec.int_matrix(37, 24, seed=3)
    assert torch.equal(t.double(), t.double().round())
    assert t.abs().max() == ec.INT_RANGE


def _bf16_np(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


@pytest.mark.parametrize("name", list(ec.REGIMES))
def test_oracle_matches_lane_level_simulators(name):
    """One 64-row slab through fc_layer_sim / bc_layer_sim (the kernels'
    index arithmetic and the MFMA fragment maps, fp32 accumulators), with
    the bf16 rounding applied between stages, equals the oracle exactly."""
    from test_chain_sim import (K0, K0P, MT, N1, N2, N3, S0, S1, S2, S3,
                                bc_layer_sim, fc_layer_sim)

    case = ec.make_case(name, MT)
    ref = ec.reference(case)

    def f32(t):
        return t.float().numpy()

    t0 = np.zeros((MT, S0), np.float32)
    t0[:, :K0] = f32(case["x"])
    W1p = np.zeros((N1, K0P), np.float32)
    W1p[:, :K0] = f32(case["W1"])
    tiles = [t0.reshape(-1)]
    for W, b, K, N, SS, DS, key in [
            (W1p, case["b1"], K0P, N1, S0, S1, "a1"),
            (f32(case["W2"]), case["b2"], N1, N2, S1, S2, "a2"),
            (f32(case["W3"]), case["b3"], N2, N3, S2, S3, "a3")]:
        dst = np.zeros(MT * DS, np.float32)
        fc_layer_sim(tiles[-1], W, b.numpy(), dst, K, N, SS, DS, True)
        dst = _bf16_np(dst)
        tiles.append(dst)
        assert np.array_equal(dst.reshape(MT, DS)[:, :N], f32(ref[key])), key
    a3 = tiles[3].reshape(MT, S3)[:, :N3]
    o = a3 @ f32(case["w4"]) + case["b4"].numpy()
    assert o.dtype == np.float32
    assert np.array_equal(o, ref["out_fp32"].numpy())

    # backward: tiles hold the activations (the relu masks) and are
    # overwritten in place by dz, as in the kernel
    t1, t2, t3 = (t.copy() for t in tiles[1:])
    dy = f32(case["dy"]).reshape(MT, 1)
    v3 = t3.reshape(MT, S3)
    pre3 = dy * f32(case["w4"]).reshape(1, N3) * (v3[:, :N3] > 0)
    assert np.array_equal(pre3, ref["dz3_pre"].numpy())
    v3[:, :N3] = _bf16_np(pre3.astype(np.float32))
    bc_layer_sim(t3, f32(case["W3"]).T.copy(), t2, N3, N2, S3, S2)
    pre2 = t2.reshape(MT, S2)[:, :N2].copy()
    t2 = _bf16_np(t2)
    bc_layer_sim(t2, f32(case["W2"]).T.copy(), t1, N2, N1, S2, S1)
    pre1 = t1.reshape(MT, S1)[:, :N1].copy()
    for pre, k in ((pre2, "dz2"), (pre1, "dz1")):
        assert np.array_equal(pre, ref[k + "_pre"].numpy()), k
        assert np.array_equal(_bf16_np(pre), f32(ref[k])), k
    for pre, k in ((pre1, "db1"), (pre2, "db2"), (pre3, "db3")):
        assert np.array_equal(pre.astype(np.float64).sum(0),
                              ref[k].numpy()), k
