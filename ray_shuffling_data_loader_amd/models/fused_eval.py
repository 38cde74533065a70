"""Forward-only evaluation of the fixed TabularMLP(100-512-256-128-1)
through the project's own chain kernels — the scoring counterpart of
models/fused_step.py.

``fused_step`` trains the model with hand-written launches whose rounding
points (bf16 activations between layers, fp32 head) differ from
``model(x)`` under autocast, so a validation loss taken through hipBLASLt
is not the quantity the step minimises. This module scores the model with
the training forward's arithmetic and none of its by-products:

  native path (hip.eval_chain_bf16 + hip.eval_accumulate), per batch:
    1. x swizzle (forward layout only)
    2. eval chain (csrc/fwd_chain.hip, eval_chain_kernel): the three MFMA
       layers and the head of the training kernel, bit for bit, writing
       only fp32 predictions and/or four fp32 partials per workgroup
       {sum (o-t)^2, sum |o-t|, sum t, sum t^2} — no a1^T/a2^T fragments,
       no mask words, no a3, no dy (~450 MB per 250k-row batch)
    3. eval_accumulate (csrc/step_glue.hip): partials -> a persistent
       fp64 accumulator {rows, sse, sae, sum_t, sum_tt} on the GPU, in
       place, fixed order, no atomics
  The bf16 fragment-major weight stage (hip.step_prep) is cached on the
  evaluator and refreshed, with one launch, only when a weight tensor's
  ``_version`` or ``data_ptr()`` has changed — after every
  ``optimizer.step()``, without the caller saying so. Nothing syncs and
  nothing reads the host until ``compute()``.

  composed path (CPU stand-ins such as tests/_fake_hip.py, an extension
  without eval_chain_bf16, fused_step._NATIVE_GLUE off): calls
  ``hip.fwd_chain_bf16(..., target=None)`` and takes its ``out``, then
  accumulates the same five sums with torch ops in fp64. Its predictions
  are therefore bf16-ROUNDED (``out`` is bf16); the native path's are the
  unrounded fp32 head values.

The evaluator reads the parameters and nothing else: it never touches
``.grad``, never modifies a parameter and does not depend on
``model.training``.

Validated by tests/test_fused_eval_gpu.py (bit-equality with the training
forward, canaries, accumulator, staging, loader end to end) and
tests/test_fused_eval_cpu.py (composed path, gloo all-reduce).
"""

import math
from typing import Dict, Optional

import torch

from ray_shuffling_data_loader_amd.models import fused_step as _fs
from ray_shuffling_data_loader_amd.models.mlp import TabularMLP

# step_prep output order: W1s, W2s, W3s, W2^T s, W3^T s, w4 bf16; the eval
# chain reads these four.
_STAGE_IDX = (0, 1, 2, 5)
_STAGE_NUMEL = (512 * 112, 256 * 512, 128 * 256, 256 * 512, 128 * 256, 128)


def _check_x(x: torch.Tensor) -> None:
    """Reject what the training step's bindings reject, in their words."""
    if not (x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 100
            and x.is_contiguous()):
        raise RuntimeError(
            "fused_eval: x must be contiguous bf16 [M,100], got "
            f"{x.dtype} {tuple(x.shape)}"
        )


class FusedEvaluator:
    """Streaming regression metrics of ``model`` over loader batches.

    ``update(x, target)`` folds one batch into an on-device fp64
    accumulator (three launches at steady state on the native path, no
    sync, no host read); ``compute()`` reads it back once and returns
    ``{"rows", "mse", "rmse", "mae", "r2"}``; ``reset()`` zeroes it.
    ``predict(x)`` returns the fp32 [M,1] predictions of the same forward.
    ``rows`` is the chain kernels' slab size (32 or 64; 0 = the default of
    fused_step / the extension); it regroups the partial sums only.
    """

    def __init__(self, model: TabularMLP, rows: int = 0):
        self.model = model
        self._lin = _fs._layers(model)
        self.rows = int(rows)
        self._acc: Optional[torch.Tensor] = None
        self._bufs = None
        self._stage_key = None

    # -- plumbing ------------------------------------------------------
    def _hip(self):
        from ray_shuffling_data_loader_amd.ops import shuffle_ops

        return shuffle_ops._load_hip()

    def _rows_kw(self) -> dict:
        rows = self.rows or _fs._CHAIN_ROWS
        return {"rows": rows} if rows else {}

    def _native_ok(self, hip, x: torch.Tensor) -> bool:
        """The conditions of fused_step._native_ok that concern a forward:
        the extension has the eval bindings, and the stock fp32 model plus
        a contiguous bf16 batch sit on a GPU."""
        if not (_fs._NATIVE_GLUE and hasattr(hip, "eval_chain_bf16")
                and hasattr(hip, "eval_accumulate")
                and hasattr(hip, "step_prep")):
            return False
        if not x.is_cuda:
            return False
        return all(
            p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
            and p.data_ptr() % 16 == 0
            for m in self._lin for p in (m.weight, m.bias)
        )

    def _accumulator(self, device) -> torch.Tensor:
        if self._acc is None or self._acc.device != device:
            self._acc = torch.zeros(5, dtype=torch.float64, device=device)
        return self._acc

    def _stage(self, hip):
        """[W1s, W2s, W3s, w4b], re-staged with one step_prep launch when
        any weight tensor was written (``_version``) or replaced
        (``data_ptr()``) since the last staging. In-place updates
        (optimizer steps, ``p.mul_`` under no_grad) bump ``_version``; a
        write that bypasses the version counter (through ``p.data``) is
        not seen until the next one that does not."""
        ws = [m.weight for m in self._lin]
        key = tuple((w._version, w.data_ptr()) for w in ws)
        dev = ws[0].device
        if self._bufs is None or self._bufs[0].device != dev:
            self._bufs = [
                torch.empty(n, dtype=torch.bfloat16, device=dev)
                for n in _STAGE_NUMEL
            ]
            self._stage_key = None
        if key != self._stage_key:
            hip.step_prep([w.detach() for w in ws], outs=self._bufs)
            self._stage_key = key
        return [self._bufs[i] for i in _STAGE_IDX]

    def _biases(self):
        return [m.bias.detach() for m in self._lin]

    def _composed_out(self, hip, x: torch.Tensor) -> torch.Tensor:
        """bf16 [M,1] ``out`` of the training forward binding."""
        lin = self._lin
        W1, W2, W3 = (m.weight.detach().bfloat16() for m in lin[:3])
        w4 = lin[3].weight.detach().reshape(-1).bfloat16()
        b1, b2, b3, b4 = self._biases()
        res = hip.fwd_chain_bf16(
            x, W1, b1, W2, b2, W3, b3, w4, b4, target=None,
            **self._rows_kw(),
        )
        return res[5]

    # -- public --------------------------------------------------------
    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [M,1] predictions (bf16-rounded on the composed path)."""
        _check_x(x)
        M = x.shape[0]
        if M == 0:
            return torch.empty(0, 1, dtype=torch.float32, device=x.device)
        hip = self._hip()
        if self._native_ok(hip, x):
            pred, _ = hip.eval_chain_bf16(
                x, self._stage(hip), self._biases(), **self._rows_kw()
            )
            return pred.view(M, 1)
        return self._composed_out(hip, x).float().reshape(M, 1)

    def update(self, x: torch.Tensor, target: torch.Tensor) -> None:
        """Fold one batch into the accumulator. Never syncs."""
        _check_x(x)
        M = x.shape[0]
        if target.numel() != M:
            raise RuntimeError(
                f"fused_eval: target size mismatch ({target.numel()} "
                f"values for {M} rows)"
            )
        if M == 0:
            return
        hip = self._hip()
        acc = self._accumulator(x.device)
        if target.dtype not in (torch.float32, torch.float64):
            target = target.float()
        if self._native_ok(hip, x) and target.is_cuda:
            _, part = hip.eval_chain_bf16(
                x, self._stage(hip), self._biases(), target=target,
                want_pred=False, **self._rows_kw(),
            )
            hip.eval_accumulate(part, acc, M)
            return
        o = self._composed_out(hip, x).reshape(-1).double()
        # the kernels read the target as fp32
        t = target.reshape(-1).float().double().to(o.device)
        d = o - t
        acc += torch.stack([
            torch.full((), float(M), dtype=torch.float64, device=o.device),
            (d * d).sum(), d.abs().sum(), t.sum(), (t * t).sum(),
        ])

    def reset(self) -> None:
        if self._acc is not None:
            self._acc.zero_()

    def state(self) -> torch.Tensor:
        """A copy of the fp64 accumulator {rows, sse, sae, sum_t, sum_tt}
        (on the device; reading it is the caller's sync)."""
        if self._acc is None:
            # no batch yet: zeros where the model lives, so a collective
            # over the ranks' states still finds a tensor of its backend
            return torch.zeros(5, dtype=torch.float64,
                               device=self._lin[0].weight.device)
        return self._acc.clone()

    def compute(self, group=None) -> Dict[str, float]:
        """Read the accumulator back (the one host read) and derive the
        metrics. With torch.distributed initialised, or ``group`` given, a
        copy of the five sums is SUM-all-reduced first, so every rank
        returns the metrics of all ranks' rows. Zero rows give NaN
        metrics."""
        v = self.state()
        import torch.distributed as dist

        if group is not None or (dist.is_available()
                                 and dist.is_initialized()):
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
        rows, sse, sae, st, stt = v.tolist()
        nan = float("nan")
        if rows <= 0:
            return {"rows": 0, "mse": nan, "rmse": nan, "mae": nan,
                    "r2": nan}
        mse = sse / rows
        den = stt - st * st / rows
        return {
            "rows": int(rows),
            "mse": mse,
            "rmse": math.sqrt(mse),
            "mae": sae / rows,
            "r2": 1.0 - sse / den if den != 0.0 else nan,
        }


def fused_predict(model: TabularMLP, x: torch.Tensor) -> torch.Tensor:
    """fp32 [M,1] predictions of ``model`` for the bf16 [M,100] batch ``x``
    through the chain kernels (one weight staging launch per call; keep a
    FusedEvaluator and call ``predict`` to reuse the stage)."""
    return FusedEvaluator(model).predict(x)
