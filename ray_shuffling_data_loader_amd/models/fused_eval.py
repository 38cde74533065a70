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

``task="binary"`` scores a model trained with ``fused_step(loss="bce")``:
the head value is a logit o, and with e = exp(-|o|), sg = sigmoid(o) =
1/(1+e) or e/(1+e) by the sign of o, the four partials become
{sum l, sum (sg-t)^2, sum t, sum correct}, l = max(o,0) - o*t + log1p(e)
(the training kernel's expressions) and correct = ((o >= 0) == (t >=
0.5)); the accumulator then reads {rows, sum logloss, sum brier, sum t,
n_correct}. A streaming AUC rides in the same kernel: every row adds 1,
with a 64-bit integer atomic, to a persistent int64 [2][65536] histogram
at [t >= 0.5][key], key = the top 16 bits of the order-preserving
transform of the logit's bit pattern (bits ^ 0xFFFFFFFF if negative,
else bits ^ 0x80000000) — the logit truncated to bf16 precision, order
kept. Integer adds commute, so the histogram is independent of launch
and arrival order; it is still three launches per update. compute()
evaluates the tie-aware Mann-Whitney statistic over the keys in fp64.
Not handled: a NaN logit lands wherever its bits put it; ``logloss`` is
then NaN, and that is the signal.

``weighted=True`` scores with per-row sample weights w (those of
``fused_step(sample_weight=)``): the weighted chain kernel scales every
term by w and carries a fifth partial, sum w; the accumulator has six
entries {rows, c0..c3, sum w} and every mean is divided by sum w, not by
the row count. The histogram then adds llrint(w * 2^20) in place of 1 — a
fixed-point weight, so the adds stay integer and order-independent, and
the AUC, being scale-invariant, needs no change.

The evaluator reads the parameters and nothing else: it never touches
``.grad``, never modifies a parameter and does not depend on
``model.training``.

Validated by tests/test_fused_eval_gpu.py (bit-equality with the training
forward, canaries, accumulator, staging, loader end to end),
tests/test_fused_eval_cpu.py (composed path, gloo all-reduce) and, for
the binary task, tests/test_fused_bce_gpu.py / tests/test_fused_bce_cpu.py;
the weighted metrics by tests/test_fused_weights_gpu.py /
tests/test_fused_weights_cpu.py.
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


_TASKS = {"regression": 0, "binary": 1}
HIST_BINS = 1 << 16
# Fixed-point scale of a weighted histogram count: llrint(w * 2^20).
HIST_WEIGHT_SCALE = float(1 << 20)


def logit_keys(o: torch.Tensor) -> torch.Tensor:
    """int64 histogram keys of fp32 logits: the top 16 bits of the
    order-preserving transform of the bit pattern (the kernel's)."""
    bits = o.float().contiguous().view(torch.int32).to(torch.int64)
    bits = bits & 0xFFFFFFFF
    u = torch.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)
    return u >> 16


def auc_from_hist(hist: torch.Tensor) -> float:
    """Tie-aware Mann-Whitney AUC of an int64 [2, bins] histogram
    (row 0 negatives, row 1 positives, keys ascending with the score), in
    fp64: sum_b pos[b] * (neg_below[b] + neg[b] / 2) / (P * N). NaN when
    either class is absent."""
    neg = hist[0].double()
    pos = hist[1].double()
    n_pos, n_neg = pos.sum().item(), neg.sum().item()
    if n_pos <= 0 or n_neg <= 0:
        return float("nan")
    below = torch.cumsum(neg, 0) - neg
    return (pos * (below + 0.5 * neg)).sum().item() / (n_pos * n_neg)


def _check_x(x: torch.Tensor) -> None:
    """Reject what the training step's bindings reject, in their words."""
    if not (x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 100
            and x.is_contiguous()):
        raise RuntimeError(
            "fused_eval: x must be contiguous bf16 [M,100], got "
            f"{x.dtype} {tuple(x.shape)}"
        )


class FusedEvaluator:
    """Streaming metrics of ``model`` over loader batches.

    ``update(x, target)`` folds one batch into an on-device fp64
    accumulator (three launches at steady state on the native path, no
    sync, no host read); ``compute()`` reads it back once and returns
    ``{"rows", "mse", "rmse", "mae", "r2"}``; ``reset()`` zeroes it.
    ``predict(x)`` returns the fp32 [M,1] predictions of the same forward.
    ``rows`` is the chain kernels' slab size (32 or 64; 0 = the default of
    fused_step / the extension); it regroups the partial sums only.

    ``task="binary"``: the predictions are logits (``predict`` is
    unchanged), the accumulator is {rows, sum logloss, sum brier, sum t,
    n_correct} and ``compute()`` returns ``{"rows", "logloss", "accuracy",
    "brier", "base_rate", "auc"}``. ``auc=False`` drops the histogram (none
    is allocated or written) and the key.

    ``weighted=True``: ``update(x, target, sample_weight)`` requires the
    per-row weights ([M] or [M,1], any float dtype, cast to fp32), the
    accumulator is fp64 [6] = {rows, c0..c3, sum w}, and ``compute()``
    divides every mean by sum w: ``mse``, ``rmse``, ``mae`` and ``r2`` =
    1 - sum w d^2 / (sum w t^2 - (sum w t)^2 / sum w), or ``logloss``,
    ``accuracy``, ``brier``, ``base_rate`` and the weighted ``auc``.
    ``rows`` stays the row count and ``"weight_sum"`` is added; sum w <= 0
    gives NaN metrics. With ``weighted=False`` (default) nothing changes
    and passing ``sample_weight`` raises.

    Weighted AUC histogram: each row adds llrint(w * 2^20) to its int64
    bin, a fixed-point representation of the weight. The quantum is 2^-20
    (weights that are multiples of it are represented exactly, smaller
    ones round to nearest, ties to even); the capacity is 2^43 units of
    total weight per bin (2^63 / 2^20). Negative or non-finite weights are
    undefined and are not checked, because a check would need a sync.
    """

    def __init__(self, model: TabularMLP, rows: int = 0,
                 task: str = "regression", auc: bool = True,
                 weighted: bool = False):
        if task not in _TASKS:
            raise ValueError(
                "FusedEvaluator: task must be 'regression' or 'binary', "
                f"got {task!r}")
        self.model = model
        self._lin = _fs._layers(model)
        self.rows = int(rows)
        self.task = task
        self._binary = task == "binary"
        self.auc = bool(auc) and self._binary
        self.weighted = bool(weighted)
        self._nacc = 6 if self.weighted else 5
        self._hist: Optional[torch.Tensor] = None
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
            self._acc = torch.zeros(self._nacc, dtype=torch.float64,
                                    device=device)
        return self._acc

    def _histogram(self, device) -> Optional[torch.Tensor]:
        if not self.auc:
            return None
        if self._hist is None or self._hist.device != device:
            self._hist = torch.zeros(2, HIST_BINS, dtype=torch.int64,
                                     device=device)
        return self._hist

    def _native_ok_task(self, hip) -> bool:
        # the binary task needs the extension's task/hist arguments, the
        # weighted metrics its weighted heads
        if self.weighted and not getattr(hip, "HEAD_WEIGHTS", 0):
            return False
        return not self._binary or hasattr(hip, "LOSS_BCE")

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

    def update(self, x: torch.Tensor, target: torch.Tensor,
               sample_weight: Optional[torch.Tensor] = None) -> None:
        """Fold one batch into the accumulator. Never syncs.
        ``sample_weight``: required with ``weighted=True``, refused
        otherwise."""
        _check_x(x)
        M = x.shape[0]
        if target.numel() != M:
            raise RuntimeError(
                f"fused_eval: target size mismatch ({target.numel()} "
                f"values for {M} rows)"
            )
        if self.weighted:
            if sample_weight is None:
                raise ValueError(
                    "fused_eval: weighted=True needs update(x, target, "
                    "sample_weight)")
            if sample_weight.numel() != M:
                raise ValueError(
                    f"fused_eval: sample_weight has {sample_weight.numel()}"
                    f" values for {M} rows")
        elif sample_weight is not None:
            raise ValueError(
                "fused_eval: sample_weight needs "
                "FusedEvaluator(weighted=True)")
        if M == 0:
            return
        hip = self._hip()
        acc = self._accumulator(x.device)
        hist = self._histogram(x.device)
        if target.dtype not in (torch.float32, torch.float64):
            target = target.float()
        w32 = None
        if self.weighted:
            w32 = sample_weight.reshape(-1)
            if w32.dtype != torch.float32:
                w32 = w32.float()
            w32 = w32.contiguous()
        if (self._native_ok(hip, x) and target.is_cuda
                and self._native_ok_task(hip)
                and (w32 is None or w32.device == x.device)):
            kw = self._rows_kw()
            if w32 is not None:
                kw["weight"] = w32
            if self._binary:
                kw["task"] = 1
                if hist is not None:
                    kw["hist"] = hist
            _, part = hip.eval_chain_bf16(
                x, self._stage(hip), self._biases(), target=target,
                want_pred=False, **kw,
            )
            hip.eval_accumulate(part, acc, M)
            return
        out = self._composed_out(hip, x).reshape(-1)
        o = out.double()
        # the kernels read the target as fp32
        t = target.reshape(-1).float().double().to(o.device)
        # The kernels' sums in fp64 torch: every term scaled by w (the fp32
        # weight, widened; 1 when unweighted, an exact factor), and a
        # sixth sum for w that only the weighted accumulator keeps.
        if self.weighted:
            w32 = w32.to(o.device)
            w = w32.double()
        else:
            w = torch.ones_like(o)
        rows = torch.full((), float(M), dtype=torch.float64,
                          device=o.device)
        if self._binary:
            e = torch.exp(-o.abs())
            sg = torch.where(o >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            ll = torch.clamp(o, min=0.0) - o * t + torch.log1p(e)
            cls = t >= 0.5
            sums = [rows, (w * ll).sum(), (w * (sg - t) ** 2).sum(),
                    (w * t).sum(), (w * ((o >= 0) == cls).double()).sum(),
                    w.sum()]
        else:
            d = o - t
            sums = [rows, (w * d * d).sum(), (w * d.abs()).sum(),
                    (w * t).sum(), (w * t * t).sum(), w.sum()]
        acc += torch.stack(sums[:self._nacc])
        if hist is not None:
            # integer adds either way: 1 per row, or llrint(w * 2^20)
            # formed in fp32 as the weighted kernel forms it
            idx = cls.to(torch.int64) * HIST_BINS + logit_keys(out)
            if self.weighted:
                units = torch.round(w32 * HIST_WEIGHT_SCALE).to(torch.int64)
                hist.view(-1).index_add_(0, idx, units)
            else:
                hist += torch.bincount(
                    idx, minlength=2 * HIST_BINS).view(2, HIST_BINS)

    def reset(self) -> None:
        if self._acc is not None:
            self._acc.zero_()
        if self._hist is not None:
            self._hist.zero_()

    def hist_state(self) -> Optional[torch.Tensor]:
        """A copy of the int64 [2, 65536] AUC histogram (row 0 negatives,
        row 1 positives; on the device), or None when the evaluator keeps
        none (regression task, ``auc=False``)."""
        if not self.auc:
            return None
        if self._hist is None:
            return torch.zeros(2, HIST_BINS, dtype=torch.int64,
                               device=self._lin[0].weight.device)
        return self._hist.clone()

    def state(self) -> torch.Tensor:
        """A copy of the fp64 accumulator {rows, sse, sae, sum_t, sum_tt}
        — {rows, sum logloss, sum brier, sum_t, n_correct} for the binary
        task — (on the device; reading it is the caller's sync). With
        ``weighted=True`` every sum is weighted and a sixth entry holds
        sum w."""
        if self._acc is None:
            # no batch yet: zeros where the model lives, so a collective
            # over the ranks' states still finds a tensor of its backend
            return torch.zeros(self._nacc, dtype=torch.float64,
                               device=self._lin[0].weight.device)
        return self._acc.clone()

    def compute(self, group=None) -> Dict[str, float]:
        """Read the accumulator back (the one host read) and derive the
        metrics. With torch.distributed initialised, or ``group`` given, a
        copy of the five sums (six with ``weighted=True``, whose means are
        over sum w and whose result gains "weight_sum") is SUM-all-reduced
        first, so every rank returns the metrics of all ranks' rows. Zero
        rows give NaN
        metrics. The binary task returns {"rows", "logloss", "accuracy",
        "brier", "base_rate"} and, unless ``auc=False``, "auc" (its
        histogram is all-reduced the same way; NaN when a class is
        absent)."""
        v = self.state()
        h = self.hist_state()
        import torch.distributed as dist

        if group is not None or (dist.is_available()
                                 and dist.is_initialized()):
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
            if h is not None:
                dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        nan = float("nan")
        v = v.tolist()
        rows, c0, c1, c2, c3 = v[:5]
        # every mean is over n: the row count, or sum w when weighted
        n = v[5] if self.weighted else rows
        ok = n > 0.0
        res = {"rows": int(rows)}
        if self.weighted:
            res["weight_sum"] = n
        if self._binary:
            res.update({
                "logloss": c0 / n if ok else nan,
                "accuracy": c3 / n if ok else nan,
                "brier": c1 / n if ok else nan,
                "base_rate": c2 / n if ok else nan,
            })
            if h is not None:
                res["auc"] = auc_from_hist(h)
            return res
        mse = c0 / n if ok else nan
        den = c3 - c2 * c2 / n if ok else 0.0
        res.update({
            "mse": mse,
            "rmse": math.sqrt(mse) if ok else nan,
            "mae": c1 / n if ok else nan,
            "r2": 1.0 - c0 / den if den != 0.0 else nan,
        })
        return res


def fused_predict(model: TabularMLP, x: torch.Tensor) -> torch.Tensor:
    """fp32 [M,1] predictions of ``model`` for the bf16 [M,100] batch ``x``
    through the chain kernels (one weight staging launch per call; keep a
    FusedEvaluator and call ``predict`` to reuse the stage)."""
    return FusedEvaluator(model).predict(x)
