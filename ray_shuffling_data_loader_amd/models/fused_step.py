"""Fused train step for the fixed TabularMLP(100-512-256-128-1) — the
DEFAULT bench step (RSDL_FUSED_STEP=0 reverts to eager autocast).

No autograd graph; the step IS the schedule. On the default native path
(hip.fused_step_bf16, one extension call) it is 8 launches, no memset
and no copy:
  1. step_prep: fp32 master weights -> bf16 fragment-major W1s (K padded
     to 112), W2s, W3s, W2^T s, W3^T s, bf16 w4, fp32 target
  2. x swizzle (emits both x layouts)
  3. fwd chain (3 MFMA layers + head + loss/grad, MSE or binary
     cross-entropy with logits, optionally with per-row sample weights
     and a positive-class weight; emits a1^T/a2^T wgrad fragments +
     relu-mask words)
  4. bwd chain (dgrad chain from mask bits; emits dz^T fragments + db/dW4
     partials)
  5-7. three fragment-major wgrad kernels into per-slab partials
  8. step_finalize: all partials -> dW1 [512,100], dW2, dW3, dW4, db1..4
     and the scalar loss, fixed summation order, written in place
then the optimizer. With ``optimizer=`` (models/fused_optim.py, SGD or
AdamW) the optimizer is part of the schedule:
  1. step_prep only when the optimizer's staged weight buffers are not
     valid (first step, or the weights were changed behind its back) or
     the target is fp64 (then only the target blocks run)
  2-7. as above
  8. step_finalize_update: step_finalize, and the thread that stores a
     gradient element updates the fp32 master and the optimizer state in
     place and writes the bf16 image of the new weight into the staged
     buffers the next step reads
so a steady-state step is 7 launches (6 with the grouped wgrad) and no
optimizer kernels. Not capturable in a graph: the AdamW scalars that
depend on the step count are launch arguments. The composed path (FakeHip CPU mirror, grad_hook
staging, _NATIVE_GLUE off) runs the same heavy kernels through the three
older bindings with torch ops as glue (~28 launches).
Activations a1/a2 and gradients dz never exist in row-major form: the
producers emit the transposed fragment layout the wgrad kernel reads
(csrc/fwd_chain.hip, csrc/bwd_chain.hip, csrc/wgrad_frag.hip), and the
backward reads 1-bit relu masks instead of activation values.

Validated by tests/test_gpu_kernels.py (chain numerics + whole-step
parity vs eager autograd) and the lane-level CPU simulation in
tests/test_chain_sim.py.
"""

import os
from typing import Tuple

import torch

from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

# pi16 emission layout (RSDL_PI16=1): the chain kernels write each MFMA
# half-wave's packed pairs directly as the transposed-fragment runs
# under a shared intra-chunk M-permutation, dropping the cross-lane
# exchange from both epilogues. dW is invariant (M is the contraction
# dim of every consumer); schedule evidence in profiles/r02. Tests may
# override via fused_step._PI16.
_PI16 = os.environ.get("RSDL_PI16", "0") == "1"

# Rows per workgroup slab of the chain kernels (RSDL_CHAIN_ROWS=32|64):
# a 64-row workgroup issues every weight fragment it loads against two
# 32-row m-tiles, halving the weight traffic per row; only the grouping
# of the loss/db partials differs between the two (csrc/fwd_chain.hip).
# 0 = the extension's default (its own RSDL_CHAIN_ROWS latch, then the
# build's default). Tests may override via fused_step._CHAIN_ROWS.
_CHAIN_ROWS = int(os.environ.get("RSDL_CHAIN_ROWS", "0") or "0")

# Kernel variant of the three fragment wgrads (csrc/wgrad_frag.hip):
# 0 = the extension's default (its RSDL_WGRAD_LDS latch, then the
# per-shape default), 1 = the direct kernel, 2 = the LDS-ring kernel for
# all three. The partials are bit-identical either way. Tests may
# override via fused_step._WGRAD_VARIANT.
_WGRAD_VARIANT = 0

# Whether hip.fused_step_bf16 runs the three wgrads as one grouped launch
# (csrc/wgrad_frag.hip, wgrad_grouped_kernel) at variant 0: None = the
# extension's default (its RSDL_WGRAD_GROUPED latch, then the build's
# default), True / False = on / off for this process. Only the slab
# partition of the fp32 sums of dW1-dW3 differs. Tests may override via
# fused_step._WGRAD_GROUPED.
_WGRAD_GROUPED = None

# Native glue (default on; RSDL_NATIVE_GLUE=0 or fused_step._NATIVE_GLUE =
# False forces the composed path): the whole schedule runs inside one
# extension call, hip.fused_step_bf16, with the weight staging and the
# partial reductions in two kernels of csrc/step_glue.hip.
_NATIVE_GLUE = os.environ.get("RSDL_NATIVE_GLUE", "1") != "0"


def _layers(model: TabularMLP):
    """The four Linear modules of the fixed architecture, in order."""
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    assert len(lin) == 4, "fused_step requires the stock TabularMLP(100)"
    shapes = [(512, 100), (256, 512), (128, 256), (1, 128)]
    for m, (n, k) in zip(lin, shapes):
        assert m.weight.shape == (n, k), (m.weight.shape, (n, k))
    return lin


def _weight_buffers(model: TabularMLP, lin):
    """Persistent bf16 weight staging for the chain kernels: W1 pre-padded
    to [512,112], W2/W3/w4 in model layout, W2T/W3T pre-transposed for the
    dgrad B fragments. Allocated once; refreshed per step with plain
    cast-copies (the params change every optimizer step)."""
    buf = getattr(model, "_fused_buf", None)
    dev = lin[0].weight.device
    if buf is None or buf["W1p"].device != dev:
        bf = dict(dtype=torch.bfloat16, device=dev)
        buf = {
            "W1p": torch.zeros(512, 112, **bf),
            "W2": torch.empty(256, 512, **bf),
            "W3": torch.empty(128, 256, **bf),
            "w4": torch.empty(128, **bf),
        }
        model._fused_buf = buf
    # One multi-tensor cast-copy instead of four kernels.
    torch._foreach_copy_(
        [buf["W1p"][:, :100], buf["W2"], buf["W3"], buf["w4"]],
        [
            lin[0].weight.detach(),
            lin[1].weight.detach(),
            lin[2].weight.detach(),
            lin[3].weight.detach().view(-1),
        ],
    )
    return buf


# loss= of fused_step -> the chain kernels' compile-time selector
# (LOSS_MSE / LOSS_BCE of the extension). The loss enters the schedule in
# the forward chain's head epilogue only: everything after it is linear
# in dy, and step_finalize divides the summed partials by M either way.
_LOSSES = {"mse": 0, "bce": 1}


def _loss_kw(code: int) -> dict:
    """``loss=`` for the bindings; empty for MSE, as _rows_kw is at its
    default, so stand-ins that predate the argument stay callable."""
    return {"loss": code} if code else {}


def loss_head(out: torch.Tensor, target: torch.Tensor, m_rows: int,
              loss: str = "bce", sample_weight=None, pos_weight=None):
    """(dyb bf16 [M,1], loss_part fp32 [1]) of the head in torch, from the
    chain's bf16 ``out`` and with the kernel's formulas and grouping
    (csrc/fwd_chain.hip) — for stand-ins without LOSS_BCE or HEAD_WEIGHTS
    (FakeHip forms its MSE head from the bf16 ``out`` the same way).
    ``sample_weight`` fp32 [M] or None (every w = 1), ``pos_weight`` a
    float or None (BCE only). Normalisation is by M. With w = 1 and no
    pos_weight the results are those of the unweighted kernels / the
    stand-in's own MSE head, bit for bit."""
    o = out.float().reshape(-1, 1)
    t = target.float().reshape(-1, 1).to(o.device)
    inv_m = torch.tensor(1.0 / m_rows, dtype=torch.float32, device=o.device)
    if sample_weight is None:
        w = torch.ones_like(o)
    else:
        w = sample_weight.float().reshape(-1, 1).to(o.device)
    if loss == "mse":
        diff = o - t
        dyb = ((2.0 * inv_m * w) * diff).bfloat16()
        return dyb, (w * (diff * diff)).sum().reshape(1)
    e = torch.exp(-o.abs())
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sg = torch.where(o >= 0, big, small)
    if pos_weight is None or float(pos_weight) == 1.0:
        g = sg - t
        term = torch.clamp(o, min=0.0) - o * t + torch.log1p(e)
    else:
        pt = float(pos_weight) * t
        lp = torch.log1p(e)
        term = (pt * (torch.clamp(-o, min=0.0) + lp)
                + (1.0 - t) * (torch.clamp(o, min=0.0) + lp))
        # 1 - sg as sigmoid(-o), as the kernel forms it
        g = (1.0 - t) * sg - pt * torch.where(o >= 0, small, big)
    dyb = ((inv_m * w) * g).bfloat16()
    return dyb, (w * term).sum().reshape(1)


def bce_head(out: torch.Tensor, target: torch.Tensor, m_rows: int):
    """``loss_head`` for plain BCE: no weights, no pos_weight."""
    return loss_head(out, target, m_rows)


def _head_args(M: int, loss: str, sample_weight, pos_weight):
    """Validated (fp32 [M] weight or None, pos_weight float or None) of
    fused_step; a pos_weight of exactly 1 is no pos_weight."""
    if pos_weight is not None:
        if loss != "bce":
            raise ValueError(
                "fused_step: pos_weight needs loss='bce', got "
                f"loss={loss!r}")
        pos_weight = float(pos_weight)
        if not (pos_weight > 0.0 and pos_weight != float("inf")):
            raise ValueError(
                "fused_step: pos_weight must be finite and > 0, got "
                f"{pos_weight!r}")
        if pos_weight == 1.0:
            pos_weight = None
    if sample_weight is not None:
        if sample_weight.numel() != M:
            raise ValueError(
                f"fused_step: sample_weight has {sample_weight.numel()} "
                f"values for {M} rows")
        sample_weight = sample_weight.reshape(-1)
        if sample_weight.dtype != torch.float32:
            sample_weight = sample_weight.float()
        sample_weight = sample_weight.contiguous()
    return sample_weight, pos_weight


def _weight_kw(sample_weight, pos_weight) -> dict:
    """``weight=`` / ``pos_weight=`` for the bindings; empty when neither
    is given, so stand-ins that predate the arguments stay callable."""
    kw = {}
    if sample_weight is not None:
        kw["weight"] = sample_weight
    if pos_weight is not None:
        kw["pos_weight"] = pos_weight
    return kw


def _rows_kw() -> dict:
    """``rows=`` for the chain bindings; empty at the default, which also
    keeps the call valid for stand-ins that predate the argument."""
    return {"rows": _CHAIN_ROWS} if _CHAIN_ROWS else {}


def _wgrad_kw() -> dict:
    """``wgrad_variant=`` / ``wgrad_grouped=`` for hip.fused_step_bf16;
    empty at the defaults, as _rows_kw is."""
    kw = {"wgrad_variant": _WGRAD_VARIANT} if _WGRAD_VARIANT else {}
    if _WGRAD_GROUPED is not None:
        kw["wgrad_grouped"] = int(bool(_WGRAD_GROUPED))
    return kw


def _native_ok(hip, lin, x, target, grad_hook) -> bool:
    """Whether this call can take hip.fused_step_bf16: the extension has
    it, no staged grad_hook, and the stock fp32 model plus a bf16 batch
    sit on a GPU in the layouts the kernels read."""
    if not (_NATIVE_GLUE and grad_hook is None
            and hasattr(hip, "fused_step_bf16")):
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2
            and x.shape[0] > 0 and x.is_contiguous()):
        return False
    if not (target.is_cuda and target.numel() == x.shape[0]
            and target.dtype in (torch.float32, torch.float64)):
        return False
    return all(
        p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
        and p.data_ptr() % 16 == 0
        for m in lin for p in (m.weight, m.bias)
    )


def _flat_outs(lin):
    """The pre-created .grad views (flat-grad DP mode) in the order
    hip.fused_step_bf16 writes them, or None if any cannot be written in
    place (missing, not fp32/contiguous, weight view not 16-B aligned)."""
    outs = [m.weight.grad for m in lin] + [m.bias.grad for m in lin]
    for i, g in enumerate(outs):
        if g is None or g.dtype != torch.float32 or not g.is_contiguous():
            return None
        if i < 3 and g.data_ptr() % 16 != 0:
            return None
    return outs


def _world_size() -> int:
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


def fused_step(
    model: TabularMLP, x: torch.Tensor, target: torch.Tensor,
    grad_hook=None, loss: str = "mse", sample_weight=None,
    pos_weight=None, optimizer=None,
) -> Tuple[torch.Tensor, None]:
    """One manual fwd+bwd: computes the loss and POPULATES .grad on
    every parameter of ``model`` (fp32, ready for an optimizer step).
    ``x`` is the bf16 [M,100] feature batch; ``target`` is [M,1].
    Returns the (scalar fp32) loss.

    ``loss``: "mse" (default), or "bce" — binary cross-entropy with
    logits, mean over the batch; the model's output is the logit and
    ``target`` any value in [0, 1] (soft labels allowed).

    ``sample_weight``: per-row weights w, [M] or [M,1] in any float dtype
    (cast to fp32 once if needed). The loss is ``(w * l).sum() / M`` —
    normalised by M, as ``reduction="mean"`` with ``weight=`` in torch, not
    by the weight sum; pre-scale the weights for that. ``pos_weight``
    (BCE only): a Python float p > 0 multiplying the positive term,
    l = p t softplus(-o) + (1-t) softplus(o), as
    ``F.binary_cross_entropy_with_logits(pos_weight=)``. Both enter in the
    forward chain's head epilogue only; without them the step launches
    exactly what it always launched.

    ``grad_hook`` (flat-grad DP mode): called as grads become ready —
    ``grad_hook("bias")`` once every bias grad AND the head weight grad
    are in their views (right after the backward chain, BEFORE the
    wgrad kernels), then ``grad_hook("w1"|"w2"|"w3")`` after each weight
    grad copy. Lets the caller overlap per-slice gradient collectives
    with the remaining wgrad kernels (bench RSDL_OVERLAP_ALLREDUCE).

    ``optimizer``: a models.fused_optim.FusedOptimizer of ``model``. The
    step then also applies its update, bit-identical to this call without
    ``optimizer=`` followed by ``optimizer.step()`` — loss, ``.grad``
    (still populated), parameters, state and staged buffers — and on the
    native path inside the same extension call. Every other path (CPU
    stand-ins, ``grad_hook``, _NATIVE_GLUE off, flat-grad mode in a world
    larger than one, where the gradients must be reduced first) runs
    exactly that pair. None (the default) changes nothing."""
    if loss not in _LOSSES:
        raise ValueError(
            f"fused_step: loss must be 'mse' or 'bce', got {loss!r}")
    loss_code = _LOSSES[loss]
    M = x.shape[0]
    loss_name = loss
    sample_weight, pos_weight = _head_args(M, loss, sample_weight,
                                           pos_weight)
    weighted = sample_weight is not None or pos_weight is not None
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

    hip = _load_hip()
    lin = _layers(model)
    has_weights = bool(getattr(hip, "HEAD_WEIGHTS", 0))
    from ray_shuffling_data_loader_amd.ops.shuffle_ops import wgrad_frag

    native = _native_ok(hip, lin, x, target, grad_hook) and (
        not weighted or (has_weights and (
            sample_weight is None or sample_weight.device == x.device)))
    flat_mode = getattr(model, "_rsdl_flat_grads", False)
    outs = _flat_outs(lin) if native and flat_mode else None
    native = native and (not flat_mode or outs is not None)
    opt_kw = {}
    if optimizer is not None:
        if optimizer.model is not model:
            raise ValueError(
                "fused_step: optimizer was built for another model")
        params = optimizer._params()
        if not (native and optimizer._native(hip, params)
                and not (flat_mode and _world_size() > 1)):
            step_loss = fused_step(model, x, target, grad_hook, loss_name,
                                   sample_weight, pos_weight)
            optimizer.step()
            return step_loss
        opt_kw = {"opt": optimizer._opt_arg(params)}
    if native:
        res = hip.fused_step_bf16(
            x, target,
            [m.weight.detach() for m in lin],
            [m.bias.detach() for m in lin],
            pi16=_PI16, outs=outs, **_rows_kw(), **_loss_kw(loss_code),
            **_weight_kw(sample_weight, pos_weight), **_wgrad_kw(),
            **opt_kw,
        )
        if optimizer is not None:
            optimizer._updated(params)
        if outs is None:
            # dW1..dW4 then db1..db4, fresh fp32 tensors in the
            # parameters' shapes.
            for i, m in enumerate(lin):
                m.weight.grad = res[1 + i]
                m.bias.grad = res[5 + i]
        return res[0]

    buf = _weight_buffers(model, lin)
    b1, b2, b3, b4 = (m.bias.detach() for m in lin)
    # Forward chain: a1/a2 exist only TRANSPOSED (wgrad fragment-major)
    # plus 32-bit relu-mask words; loss + dy fold into the head epilogue.
    # The x swizzle emits BOTH x layouts (fwd fragments + wgrad x^T) in
    # one pass over x.
    mchunks = 2 * ((M + 31) // 32)
    xt = torch.empty(4 * mchunks * 512, dtype=torch.bfloat16,
                     device=x.device)
    if (loss_code and not hasattr(hip, "LOSS_BCE")) or (
            weighted and not has_weights):
        # a stand-in without the BCE head or without the weighted heads:
        # forward only, head in torch
        a1t, mask1, a2t, mask2, a3, out = hip.fwd_chain_bf16(
            x, buf["W1p"], b1, buf["W2"], b2, buf["W3"], b3, buf["w4"], b4,
            target=None, xt_out=xt, pi16=_PI16, **_rows_kw(),
        )
        dyb, loss_part = loss_head(out, target, M, loss_name,
                                   sample_weight, pos_weight)
    else:
        a1t, mask1, a2t, mask2, a3, out, dyb, loss_part = (
            hip.fwd_chain_bf16(
                x, buf["W1p"], b1, buf["W2"], b2, buf["W3"], b3, buf["w4"],
                b4, target=target, xt_out=xt, pi16=_PI16, **_rows_kw(),
                **_loss_kw(loss_code),
                **_weight_kw(
                    None if sample_weight is None
                    else sample_weight.to(x.device),
                    pos_weight),
            )
        )
    loss = loss_part.sum() / M
    # Backward chain: consumes the masks (never the activations), emits
    # dz^T fragments; dW4/db4 partials fold into its seed loop.
    dz1t, dz2t, dz3t, db1, db2, db3, db4, dw4 = hip.bwd_chain_bf16(
        dyb, a3, mask1, mask2, buf["w4"], buf["W3"], buf["W2"], pi16=_PI16,
        **_rows_kw(),
    )
    # The DP bench pre-creates .grad as views of one flat buffer (so the
    # gradient all-reduce is a single collective) and marks the model;
    # only then do we COPY into them. Otherwise assign the fresh tensors
    # (copying would add 8 small kernels per step at N=1).
    flat_mode = getattr(model, "_rsdl_flat_grads", False)
    if flat_mode and grad_hook is not None:
        # Bias + head grads are ready NOW — copy and signal so their
        # collective overlaps the wgrad kernels below.
        for m, gb in zip(lin, (db1, db2, db3, db4)):
            m.bias.grad.copy_(gb.reshape(m.bias.shape))
        lin[3].weight.grad.copy_(dw4)
        grad_hook("bias")
    # Weight grads: fragment-major MFMA wgrad kernel (csrc/wgrad_frag.hip)
    # reading the transposed fragments the producers emitted.
    dw1 = wgrad_frag(dz1t, xt, 512, 128, mchunks, _WGRAD_VARIANT)[:, :100].contiguous()
    if flat_mode and grad_hook is not None:
        lin[0].weight.grad.copy_(dw1)
        grad_hook("w1")
    dw2 = wgrad_frag(dz2t, a1t, 256, 512, mchunks, _WGRAD_VARIANT)
    if flat_mode and grad_hook is not None:
        lin[1].weight.grad.copy_(dw2)
        grad_hook("w2")
    dw3 = wgrad_frag(dz3t, a2t, 128, 256, mchunks, _WGRAD_VARIANT)
    if flat_mode and grad_hook is not None:
        lin[2].weight.grad.copy_(dw3)
        grad_hook("w3")
        return loss
    grads = [
        (dw1, db1),
        (dw2, db2),
        (dw3, db3),
        (dw4, db4),
    ]
    for m, (gw, gb) in zip(lin, grads):
        gb = gb.reshape(m.bias.shape)
        if flat_mode:
            m.weight.grad.copy_(gw)
            m.bias.grad.copy_(gb)
        else:
            m.weight.grad = gw.to(m.weight.dtype)
            m.bias.grad = gb.to(m.bias.dtype)
    return loss
