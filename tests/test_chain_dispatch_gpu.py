"""GPU test of the chain launchers' dispatch (csrc/fwd_chain.hip,
launch_fwd_chain / launch_eval_chain): every instantiation of
fwd_chain_kernel<MT, PI16, LOSS, WEIGHTED> and eval_chain_kernel<MT, TASK,
WEIGHTED> is reachable through the bindings and is the one its arguments
name.

M = 65: three 32-row m-tiles, so the 64-row kernel's last workgroup has no
second tile and the row guard cuts inside a tile. Weights and data are the
``data`` fixture of tests/test_fused_weights_gpu.py. Every assertion is a
bit-equality or a shape. The reference point is (rows = 32, pi16 = False)
for each loss and each of {unweighted, weighted}; the numerics of that
point are checked by tests/test_fused_bce_gpu.py and
tests/test_fused_weights_gpu.py.
"""

import itertools

import pytest
import torch

from test_fused_weights_gpu import data, dev, hip  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

M = 65
ROWS = (32, 64)
NAMES = ["a1t", "mask1", "a2t", "mask2", "a3", "out", "dyb", "loss_part"]
WEIGHTS = ("none", "w", "ones")


def _bits(a):
    return a.view(torch.int16) if a.dtype == torch.bfloat16 else a


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _target(data, loss):
    return (data["reg"] if loss == 0 else data["tgt"])[:M].contiguous()


def _weight_kw(data, dev, wk):
    if wk == "none":
        return {}
    return {"weight": data["w"][:M].contiguous() if wk == "w"
            else torch.ones(M, device=dev)}


@pytest.fixture(scope="module")
def fwd(hip, data, dev):
    """{(rows, pi16, loss, weight kind): dict of the eight outputs}."""
    Wb, bs = data["Wb"], data["bs"]
    x = data["x"][:M].contiguous()
    res = {}
    for rows, pi16, loss, wk in itertools.product(
            ROWS, (False, True), (0, 1), WEIGHTS):
        out = hip.fwd_chain_bf16(
            x, Wb[0], bs[0], Wb[1], bs[1], Wb[2], bs[2], Wb[3].flatten(),
            bs[3], target=_target(data, loss), pi16=pi16, rows=rows,
            loss=loss, **_weight_kw(data, dev, wk))
        assert len(out) == 8
        res[rows, pi16, loss, wk] = dict(zip(NAMES, out))
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def ev(hip, data, dev):
    """{(rows, task, weight kind): (pred, part)} through step_prep staging."""
    stage = hip.step_prep([W.float().contiguous() for W in data["Wb"]])
    stage = [stage[i] for i in (0, 1, 2, 5)]
    x = data["x"][:M].contiguous()
    res = {}
    for rows, task, wk in itertools.product(ROWS, (0, 1), WEIGHTS):
        res[rows, task, wk] = hip.eval_chain_bf16(
            x, stage, data["bs"], target=_target(data, task), rows=rows,
            task=task, **_weight_kw(data, dev, wk))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("wk", ("none", "w"))
@pytest.mark.parametrize("loss", (0, 1))
@pytest.mark.parametrize("pi16", (False, True))
@pytest.mark.parametrize("rows", ROWS)
def test_forward_instantiation(fwd, rows, pi16, loss, wk):
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import (
        t_frag_unswizzle,
    )

    tag = f"rows={rows} pi16={pi16} loss={loss} weight={wk}"
    got, ref = fwd[rows, pi16, loss, wk], fwd[32, False, loss, wk]
    for nm in ("mask1", "mask2", "a3", "out", "dyb"):
        assert _same(got[nm], ref[nm]), (tag, nm)
    for nm, c in (("a1t", 512), ("a2t", 256)):
        assert _same(t_frag_unswizzle(got[nm], M, c, pi16),
                     t_frag_unswizzle(ref[nm], M, c, False)), (tag, nm)
    if pi16:
        # PI16 reached the kernel: the raw fragments are in another order,
        # on the valid rows too (the pad rows of a1t are not compared)
        assert not _same(got["a1t"], ref["a1t"]), tag
        assert not _same(t_frag_unswizzle(got["a1t"], M, 512, False),
                         t_frag_unswizzle(ref["a1t"], M, 512, False)), tag
    assert got["loss_part"].shape == ((M + rows - 1) // rows,), tag
    if rows == 32:
        assert _same(got["loss_part"], ref["loss_part"]), tag
    # LOSS reached the kernel
    assert not _same(got["dyb"], fwd[rows, pi16, 1 - loss, wk]["dyb"]), tag


@pytest.mark.parametrize("loss", (0, 1))
@pytest.mark.parametrize("pi16", (False, True))
@pytest.mark.parametrize("rows", ROWS)
def test_forward_weighted_kernel(fwd, data, rows, pi16, loss):
    """weight=ones runs the WEIGHTED instantiation and gives the
    unweighted bits; the real weights zero dyb where w = 0."""
    tag = f"rows={rows} pi16={pi16} loss={loss}"
    ones, plain = fwd[rows, pi16, loss, "ones"], fwd[rows, pi16, loss, "none"]
    for nm in NAMES:
        assert _same(ones[nm], plain[nm]), (tag, nm)
    w = data["w"][:M]
    dyb = fwd[rows, pi16, loss, "w"]["dyb"].flatten().float()
    assert bool((w == 0).any()) and bool((dyb[w == 0] == 0).all()), tag
    assert not _same(fwd[rows, pi16, loss, "w"]["dyb"], plain["dyb"]), tag


@pytest.mark.parametrize("wk", ("none", "w"))
@pytest.mark.parametrize("task", (0, 1))
@pytest.mark.parametrize("rows", ROWS)
def test_eval_instantiation(fwd, ev, rows, task, wk):
    tag = f"rows={rows} task={task} weight={wk}"
    pred, part = ev[rows, task, wk]
    assert _same(pred, ev[32, 0, "none"][0]), tag
    f = fwd[rows, False, task, wk]
    assert _same(pred.bfloat16().flatten(), f["out"].flatten()), tag
    grid = (M + rows - 1) // rows
    assert part.shape == (grid, 4 if wk == "none" else 8), tag
    assert _same(part[:, 0], f["loss_part"]), tag


@pytest.mark.parametrize("task", (0, 1))
@pytest.mark.parametrize("rows", ROWS)
def test_eval_weighted_kernel(ev, dev, rows, task):
    """weight=ones runs the WEIGHTED instantiation: the unweighted four
    partials, the slab's row count in column 4, zeros behind it."""
    tag = f"rows={rows} task={task}"
    pred, part = ev[rows, task, "ones"]
    plain = ev[rows, task, "none"][1]
    grid = (M + rows - 1) // rows
    assert part.shape == (grid, 8), tag
    assert _same(pred, ev[rows, task, "none"][0]), tag
    assert _same(part[:, :4], plain), tag
    count = torch.full((grid,), float(rows), device=dev)
    count[-1] = M - (grid - 1) * rows
    assert torch.equal(part[:, 4], count), (tag, part[:, 4])
    assert bool((part[:, 5:] == 0).all()), tag
