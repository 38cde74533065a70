"""GPU tests of the 64-row workgroup slabs of the fused chain kernels
(csrc/fwd_chain.hip, csrc/bwd_chain.hip; ``rows=64``) against the 32-row
instantiations of the same build (``rows=32``).

A 64-row workgroup runs two 32-row m-tiles and issues every weight
fragment against both. The global layouts do not change and every
accumulator sees the same MFMAs in the same k order, so everything per
row must be BIT-identical between the two slab sizes; only the per-
workgroup partials (loss_part, db_part) regroup the same terms.

The shapes cover an odd and an even count of 32-row tiles, a partial
first and a partial second m-tile, a workgroup whose second m-tile does
not exist (its x block, mask rows and fragment chunks lie past the
allocations), and a single row.

Reference for the regrouped reductions: fp64 sums of the kernels' own
terms, rebuilt in fp64 from the bf16 tensors each stage reads (dy, a3,
w4, the emitted dz3/dz2 and the mask bits). The terms of db4, dW4 and
db3 are products of at most three bf16 values and exact in fp32; the
terms of db2/db1 and of the loss are fp32 dot products of 128-256 bf16
products, off from fp64 by about sqrt(K) * 2^-24 relative, an order of
magnitude inside the project's bound for reordered reductions,
1e-5 * max|ref| + 1e-5 (profiles/PERF.md, round 3).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [1, 31, 32, 33, 64, 65, 96, 97, 161]
M_MAX = max(SHAPES)
FWD_NAMES = ["a1t", "mask1", "a2t", "mask2", "a3", "out", "dyb", "loss_part"]
BWD_NAMES = ["dz1t", "dz2t", "dz3t", "db1", "db2", "db3", "db4", "dw4"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    return shuffle_ops._load_hip()


@pytest.fixture(scope="module")
def data(dev):
    """Seeded weights, biases and the largest batch; smaller shapes take
    its leading rows."""
    g = torch.Generator(device="cpu").manual_seed(64)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    Ws = [
        (rn(512, 100) / 10).bfloat16(),
        (rn(256, 512) / 22).bfloat16(),
        (rn(128, 256) / 16).bfloat16(),
        (rn(1, 128) / 11).bfloat16(),
    ]
    bs = [(rn(n) / 4).bfloat16() for n in (512, 256, 128, 1)]
    return {
        "Ws": Ws,
        "bs": bs,
        "x": rn(M_MAX, 100).bfloat16(),
        "tgt": rn(M_MAX, 1),
    }


@pytest.fixture(scope="module")
def run(hip, data):
    """chain(M, pi16, rows) -> dict of the forward and backward bindings'
    outputs, computed once per key. The backward always reads the
    rows=32 forward's outputs, so a forward slip cannot hide a backward
    one."""
    cache = {}

    def fwd(M, pi16, rows):
        Ws, bs = data["Ws"], data["bs"]
        x = data["x"][:M].contiguous()
        mchunks = 2 * ((M + 31) // 32)
        xt = torch.empty(4 * mchunks * 512, dtype=torch.bfloat16,
                         device=x.device)
        res = hip.fwd_chain_bf16(
            x, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], Ws[3].flatten(),
            bs[3], target=data["tgt"][:M].contiguous(), xt_out=xt,
            pi16=pi16, rows=rows,
        )
        return dict(zip(FWD_NAMES, res))

    def chain(M, pi16, rows):
        key = (M, pi16, rows)
        if key not in cache:
            Ws = data["Ws"]
            f = fwd(M, pi16, rows)
            src = f if rows == 32 else chain(M, pi16, 32)
            b = hip.bwd_chain_bf16(
                src["dyb"], src["a3"], src["mask1"], src["mask2"],
                Ws[3].flatten(), Ws[2], Ws[1], pi16=pi16, rows=rows,
            )
            f.update(zip(BWD_NAMES, b))
            cache[key] = f
        return cache[key]

    return chain


def _bound(ref):
    return 1e-5 * ref.abs().max().item() + 1e-5


def _mask_bits(mask, M):
    """[mtiles, N] int32 mask words -> [M, N] fp64 0/1."""
    w = mask.to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, device=mask.device, dtype=torch.int64)
    bits = (w.unsqueeze(1) >> sh.view(1, 32, 1)) & 1
    return bits.reshape(-1, mask.shape[1])[:M].double()


@pytest.mark.parametrize("pi16", [False, True])
@pytest.mark.parametrize("M", SHAPES)
def test_rows64_per_row_outputs_bit_equal(run, M, pi16):
    r32, r64 = run(M, pi16, 32), run(M, pi16, 64)
    for name in ["a1t", "a2t", "mask1", "mask2", "a3", "out", "dyb",
                 "dz1t", "dz2t", "dz3t"]:
        assert r32[name].shape == r64[name].shape, name
        assert torch.equal(r32[name], r64[name]), (name, M, pi16)
    # one partial per workgroup slab
    assert r32["loss_part"].numel() == (M + 31) // 32
    assert r64["loss_part"].numel() == (M + 63) // 64


@pytest.mark.parametrize("rows", [64, 32])
@pytest.mark.parametrize("M", SHAPES)
def test_rows64_reductions_match_fp64_terms(run, data, M, rows):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
        t_frag_unswizzle,
    )

    r = run(M, False, rows)
    Ws, bs = data["Ws"], data["bs"]
    w4 = Ws[3].flatten().double()
    a3 = r["a3"].double()
    dy = r["dyb"].double().reshape(M, 1)
    tgt = data["tgt"][:M].double()

    # loss: sum_m (a3[m] . w4 + b4 - target[m])^2 / M
    o = a3 @ w4.view(-1, 1) + bs[3].double()
    want = {"loss": ((o - tgt) ** 2).sum() / M}
    got = {"loss": r["loss_part"].double().sum() / M}

    live3 = (a3 > 0).double()
    want["db4"] = dy.sum(0)
    want["dw4"] = dy.t() @ a3
    want["db3"] = (dy * w4.view(1, -1) * live3).sum(0)
    dz3 = t_frag_unswizzle(r["dz3t"], M, 128).double()
    dz2 = t_frag_unswizzle(r["dz2t"], M, 256).double()
    want["db2"] = ((dz3 @ Ws[2].double()) * _mask_bits(r["mask2"], M)).sum(0)
    want["db1"] = ((dz2 @ Ws[1].double()) * _mask_bits(r["mask1"], M)).sum(0)
    for name in ["db1", "db2", "db3", "db4", "dw4"]:
        got[name] = r[name].double()
    for name, ref in want.items():
        err = (got[name].reshape(ref.shape) - ref).abs().max().item()
        print(f"M={M} rows={rows} {name}: err {err:.3e} "
              f"bound {_bound(ref):.3e}")
        assert err <= _bound(ref), (name, M, rows, err, _bound(ref))


def _step(hip, data, dev, M, rows, pi16=False):
    torch.manual_seed(7)
    from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

    model = TabularMLP(100).to(dev)
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    return hip.fused_step_bf16(
        data["x"][:M].contiguous(), data["tgt"][:M].contiguous(),
        [m.weight.detach() for m in lin], [m.bias.detach() for m in lin],
        pi16=pi16, rows=rows,
    )


STEP_NAMES = ["loss", "dW1", "dW2", "dW3", "dW4", "db1", "db2", "db3", "db4"]


@pytest.mark.parametrize("M", [97, 161])
def test_rows64_whole_step_matches_rows32(hip, data, dev, M):
    s32 = _step(hip, data, dev, M, 32)
    s64 = _step(hip, data, dev, M, 64)
    for name, a, b in zip(STEP_NAMES, s32, s64):
        err = (a.double() - b.double()).abs().max().item()
        print(f"M={M} {name}: |rows64 - rows32| {err:.3e} "
              f"bound {_bound(a):.3e}")
        assert err <= _bound(a), (name, M, err)
        # The wgrad kernels and the finalize read bit-identical dz/a
        # fragments and sum them in the same order at either slab size.
        if name in ("dW1", "dW2", "dW3"):
            assert torch.equal(a, b), (name, M)


@pytest.mark.parametrize("M", [97, 161])
def test_rows64_is_deterministic(hip, run, data, dev, M):
    """No atomics on this path: a second rows=64 call is bit-equal. (The
    db outputs of the stand-alone bwd_chain_bf16 binding go through the
    split slab reduce, which does combine with atomics; the whole step
    below reduces them in step_finalize, in fixed order.)"""
    first = run(M, False, 64)
    Ws, bs = data["Ws"], data["bs"]
    x = data["x"][:M].contiguous()
    again = dict(zip(FWD_NAMES, hip.fwd_chain_bf16(
        x, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], Ws[3].flatten(),
        bs[3], target=data["tgt"][:M].contiguous(), rows=64,
    )))
    for name in FWD_NAMES:
        assert torch.equal(first[name], again[name]), name
    b = hip.bwd_chain_bf16(
        first["dyb"], first["a3"], first["mask1"], first["mask2"],
        Ws[3].flatten(), Ws[2], Ws[1], rows=64,
    )
    for name, t in zip(BWD_NAMES[:3], b):
        assert torch.equal(first[name], t), name
    s0 = _step(hip, data, dev, M, 64)
    s1 = _step(hip, data, dev, M, 64)
    for name, a, c in zip(STEP_NAMES, s0, s1):
        assert torch.equal(a, c), name


def test_rows_argument_is_validated(hip, data):
    Ws, bs = data["Ws"], data["bs"]
    with pytest.raises(RuntimeError, match="32 or 64"):
        hip.fwd_chain_bf16(
            data["x"][:8].contiguous(), Ws[0], bs[0], Ws[1], bs[1], Ws[2],
            bs[2], Ws[3].flatten(), bs[3], rows=48,
        )
