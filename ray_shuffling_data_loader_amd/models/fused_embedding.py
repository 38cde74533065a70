"""Fused multi-table embedding lookup (csrc/embed.hip): the categorical
columns of the reference DATA_SPEC -> one bf16 [B, T*D] activation.

  out[b, t*D:(t+1)*D] = bf16(W_t[max(idx_t[b], 0) % card_t])

``fused_embedding(indices, tables)`` replaces EmbeddingMLP's per-column
``clamp_min`` / ``%`` / ``nn.Embedding`` / ``torch.cat`` (about 80 launches
and an fp32 concat that autocast casts again) with one HIP launch, and its
19 ``embedding_dense_backward`` calls with a backward that has no float
atomics and a fixed summation order:

  * tables of at most ``_DENSE_MAX_ROWS`` rows: ``embed_bwd_onehot``, the
    one-hot product on the matrix cores, one fp32 partial per batch slab,
    folded in slab order;
  * larger tables: one stable ``torch.sort`` over int32 keys (flat gradient
    row of every (table, batch row)), then ``embed_bwd_runs`` sums every run
    of equal keys in ascending batch row.

The T gradients are views of one flat zero-initialised fp32 buffer and are
returned as ordinary dense gradients, so any torch optimizer and DDP keep
working. The tables stay separate fp32 ``nn.Embedding.weight`` parameters.

The kernels serve D in {8, 16, 32, 64, 128}. At 64 and 128 the one-hot
product is cut into 32-column slices, one workgroup each, so its slab stays
at the 512 rows of D = 32; these two widths need an extension with
``EMBED_WIDE``.

On CPU tensors, or for an input the kernels do not serve (any other D, more
than 64 tables, non-fp32 tables, B = 0), the same arithmetic runs as torch
ops: gather, cast and cat forward, an fp32 ``index_add_`` of the bf16
gradients backward (ascending batch row on CPU).

``fused_embedding(indices, tables, optimizer=opt)`` with a
``FusedEmbeddingOptimizer`` leaves the dense gradients out altogether: the
backward hands (dOut, wrapped indices) to ``opt`` and ``opt.step()`` writes
the new weights of the rows the batch touched (csrc/embed_optim.hip), so a
table needs no gradient memory next to it. See the class.
"""

import math
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

# Tables of at most this many rows take the one-hot MFMA backward, larger
# ones the sorted-runs backward (RSDL_EMBED_DENSE_MAX; sweep in
# profiles/PERF.md). Tests may override via fused_embedding._DENSE_MAX_ROWS.
_DENSE_MAX_ROWS = int(os.environ.get("RSDL_EMBED_DENSE_MAX", "256") or "256")

_MAX_TABLES = 64
_WIDTHS = (8, 16, 32)
# served as well once the loaded extension has EMBED_WIDE (_width_served)
_WIDE_WIDTHS = (64, 128)

# (device, cards, large) -> (table numbers, row offsets) of the sorted regime
_KEY_CACHE = {}


def _split(indices, T):
    """T index tensors from a list of [B] / [B,1] tensors or one [B,T]
    matrix; column views, never copies."""
    if isinstance(indices, torch.Tensor):
        if indices.dim() != 2 or indices.shape[1] != T:
            raise ValueError(
                f"fused_embedding: an index matrix must be [B, {T}], got "
                f"{tuple(indices.shape)}"
            )
        return list(indices.unbind(1))
    indices = list(indices)
    if len(indices) != T:
        raise ValueError(
            f"fused_embedding: {len(indices)} index tensors for {T} tables"
        )
    return indices


def _width_served(D) -> bool:
    """D is a width the loaded extension has kernels for: 64 and 128 came
    with ``EMBED_WIDE``, and a build from before it keeps the torch ops."""
    if D in _WIDTHS:
        return True
    if D not in _WIDE_WIDTHS:
        return False
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    return bool(getattr(shuffle_ops._load_hip(), "EMBED_WIDE", 0))


def _kernels_serve(idx, tables) -> bool:
    T = len(tables)
    w0 = tables[0]
    if not (1 <= T <= _MAX_TABLES) or not w0.is_cuda or w0.dim() != 2:
        return False
    D, B = w0.shape[1], idx[0].shape[0]
    if B < 1 or not _width_served(D):
        return False
    rows = 0
    for w, x in zip(tables, idx):
        if not (
            w.is_cuda
            and w.device == w0.device
            and w.dtype == torch.float32
            and w.dim() == 2
            and w.shape[1] == D
            and w.shape[0] >= 1
            and w.is_contiguous()
            and w.data_ptr() % 16 == 0
            and x.device == w0.device
            and x.dtype == torch.int64
            and (x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1))
            and x.shape[0] == B
            and x.stride(0) >= 0
        ):
            return False
        rows += w.shape[0]
    return rows < 2**31 and B * T < 2**31


def _row_offsets(cards):
    offs, r = [], 0
    for c in cards:
        offs.append(r)
        r += c
    return offs, r


def _forward(ctx, idx, tables, need):
    """The lookup; leaves cards, D, hip and (if ``need``) widx on ctx."""
    ctx.cards = [int(w.shape[0]) for w in tables]
    ctx.D = int(tables[0].shape[1])
    ctx.hip = _kernels_serve(idx, tables)
    if ctx.hip:
        from ray_shuffling_data_loader_amd.ops import shuffle_ops

        hip = shuffle_ops._load_hip()
        out, widx = hip.embed_concat_fwd(
            idx, [w.detach() for w in tables], need
        )
    else:
        wrapped = [
            x.reshape(-1).clamp_min(0) % c
            for x, c in zip(idx, ctx.cards)
        ]
        out = torch.cat(
            [w[i] for w, i in zip(tables, wrapped)], dim=1
        ).bfloat16()
        widx = torch.stack(wrapped, dim=1)
    ctx.widx = widx if need else None
    return out


class _FusedEmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, *args):
        idx, tables = list(args[:T]), list(args[T:])
        return _forward(ctx, idx, tables, any(ctx.needs_input_grad[1 + T:]))

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        cards, D, widx = ctx.cards, ctx.D, ctx.widx
        T = len(cards)
        offs, rows = _row_offsets(cards)
        dout = dout.to(torch.bfloat16).contiguous()
        # one memset for all T gradients
        flat = torch.zeros(rows, D, dtype=torch.float32, device=dout.device)
        if ctx.hip:
            _hip_backward(dout, widx, flat, cards, offs)
        else:
            for t in range(T):
                flat[offs[t]:offs[t] + cards[t]].index_add_(
                    0, widx[:, t], dout[:, t * D:(t + 1) * D].float()
                )
        grads = [
            flat[offs[t]:offs[t] + cards[t]]
            if ctx.needs_input_grad[1 + T + t]
            else None
            for t in range(T)
        ]
        return (None,) * (1 + T) + tuple(grads)


def _hip_backward(dout, widx, flat, cards, offs):
    from ray_shuffling_data_loader_amd.ops import shuffle_ops

    hip = shuffle_ops._load_hip()
    dense = [t for t, c in enumerate(cards) if c <= _DENSE_MAX_ROWS]
    large = [t for t, c in enumerate(cards) if c > _DENSE_MAX_ROWS]
    if dense:
        hip.embed_bwd_onehot(
            dout, widx, flat, dense,
            [cards[t] for t in dense], [offs[t] for t in dense],
        )
    if large:
        keys, pos = _sorted_keys(widx, cards, offs, large)
        hip.embed_bwd_runs(dout, widx, flat, keys, pos, large)


def _sorted_keys(widx, cards, offs, large):
    """(keys int32 ascending, pos int64) of the sorted regime's tables."""
    key = (widx.device, tuple(cards), tuple(large))
    if key not in _KEY_CACHE:
        _KEY_CACHE[key] = (
            torch.tensor(large, device=widx.device),
            torch.tensor([offs[t] for t in large], dtype=torch.int32,
                         device=widx.device)[:, None],
        )
    cols, roff = _KEY_CACHE[key]
    # int32 [L, B]: the flat gradient row of every (table, batch row)
    keys = widx.t().index_select(0, cols).add_(roff).reshape(-1)
    return torch.sort(keys, stable=True)


class _FusedEmbeddingOptFn(torch.autograd.Function):
    """The lookup whose backward gives the tables no gradient: it leaves
    (dOut, wrapped indices) with the optimizer."""

    @staticmethod
    def forward(ctx, opt, T, *args):
        ctx.opt = opt
        return _forward(ctx, list(args[:T]), list(args[T:]), True)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        ctx.opt._receive(
            dout.to(torch.bfloat16).contiguous(), ctx.widx, ctx.hip
        )
        return (None,) * (2 + 2 * len(ctx.cards))


_OPT_KINDS = {"sgd": 0, "adagrad": 1, "rowwise_adagrad": 2}


def _f32(v, device):
    """``v`` rounded to fp32 once, as the kernels receive it."""
    return torch.tensor(float(v), dtype=torch.float32, device=device)


def _check_opt_hyper(kind, lr, eps, initial_accumulator_value=0.0):
    if kind not in _OPT_KINDS:
        raise ValueError(
            "FusedEmbeddingOptimizer: kind must be 'sgd', 'adagrad' or "
            f"'rowwise_adagrad', got {kind!r}")
    vals = {"lr": lr, "eps": eps,
            "initial_accumulator_value": initial_accumulator_value}
    for name, v in vals.items():
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
            raise ValueError(
                f"FusedEmbeddingOptimizer: {name} must be finite and >= 0, "
                f"got {v!r}")
    if kind != "sgd" and not float(_f32(eps, "cpu")) > 0.0:
        raise ValueError(
            f"FusedEmbeddingOptimizer: {kind} needs eps > 0 in fp32 (a row "
            f"without gradient must not move), got {eps!r}")


class FusedEmbeddingOptimizer:
    """``FusedEmbeddingOptimizer(tables, kind="sgd" | "adagrad" |
    "rowwise_adagrad", lr=1e-2, eps=1e-10, initial_accumulator_value=0.0)``:
    the update of ``fused_embedding(indices, tables, optimizer=opt)``.

      out = fused_embedding(indices, tables, optimizer=opt)
      loss.backward()   # tables get no .grad; opt holds (dOut, indices)
      opt.step()        # sort + update kernels over the batch's rows

    The arithmetic, one fp32 IEEE operation per line, nothing fused, ``lr``
    and ``eps`` rounded to fp32 once; ``g`` is the row's fp32 sum of bf16
    dOut segments (ascending batch row inside 16-position chunks of the
    sorted keys, then chunks ascending; ascending batch slabs for tables of
    at most ``_DENSE_MAX_ROWS`` rows):

      sgd              p' = p - lr * g
      adagrad          h' = h + g * g                       (per element)
                       p' = p - lr * (g / (sqrt(h') + eps))
      rowwise_adagrad  s_l = ((gx*gx + gy*gy) + gz*gz) + gw*gw  per 4 elements
                       s   = xor-butterfly sum of the G = D/4 s_l, distances
                             1 .. G/2 ascending (1, 2, 4, 8, 16 at D = 128)
                       h' = h + s * (1/D)                   (one per row)
                       p' = p - lr * (g / (sqrt(h') + eps))

    A row with zero gradient comes out bit-identical under all three (hence
    ``eps > 0`` for the adagrads), so touching only the batch's rows is the
    dense optimizer's result: ``torch.optim.SGD`` without momentum or weight
    decay, ``torch.optim.Adagrad`` without ``lr_decay`` or weight decay.
    Momentum, weight decay and Adam-style lazy updates are not offered.

    ``opt`` is bound to ``tables`` by identity and order. ``lr`` and ``eps``
    are plain attributes read at every step. ``state[t]`` is table t's fp32
    state: ``{"sum": [card, D]}`` (adagrad), ``{"sum": [card]}`` (rowwise) or
    ``{}`` (sgd), filled with ``initial_accumulator_value``. One batch at a
    time: a second backward before ``step()`` raises, accumulation is not
    offered. ``step()`` refuses to run under ``torch.distributed`` with more
    than one process: sparse gradients are not exchanged.

    On CPU tensors, for inputs the kernels do not serve and with an
    extension without ``EMBED_OPTIM``, ``step()`` runs the same list as torch
    ops over the touched rows, with an ascending-batch-row fp32
    ``index_add_`` for ``g`` (for D that is no power of two times 4 the
    row's s is a plain fp32 sum); bit-identical to the kernels wherever the
    gradient sums are exact."""

    def __init__(self, tables, kind: str = "sgd", lr: float = 1e-2,
                 eps: float = 1e-10, initial_accumulator_value: float = 0.0):
        _check_opt_hyper(kind, lr, eps, initial_accumulator_value)
        self.tables = list(tables)
        if not self.tables:
            raise ValueError(
                "FusedEmbeddingOptimizer: needs at least one table")
        if len({id(w) for w in self.tables}) != len(self.tables):
            raise ValueError(
                "FusedEmbeddingOptimizer: a table is given twice")
        for w in self.tables:
            if w.dim() != 2 or w.shape[1] != self.tables[0].shape[1]:
                raise ValueError(
                    "FusedEmbeddingOptimizer: tables must be [card, D] with "
                    "one D")
        self.kind = kind
        self.lr = lr
        self.eps = eps
        self.initial_accumulator_value = initial_accumulator_value
        self.step_count = 0
        self._pending = None
        self.state = {
            t: {"sum": torch.full(self._state_shape(w),
                                  float(initial_accumulator_value),
                                  dtype=torch.float32, device=w.device)}
            if kind != "sgd" else {}
            for t, w in enumerate(self.tables)
        }

    def _state_shape(self, w):
        return tuple(w.shape) if self.kind == "adagrad" else (w.shape[0],)

    def _check_tables(self, tables):
        if len(tables) != len(self.tables) or any(
                a is not b for a, b in zip(tables, self.tables)):
            raise ValueError(
                "fused_embedding: optimizer= is bound to other tables")

    def _receive(self, dout, widx, hip):
        if self._pending is not None:
            raise RuntimeError(
                "FusedEmbeddingOptimizer: a second backward before step(); "
                "gradient accumulation is not offered")
        self._pending = (dout, widx, hip)

    def zero_grad(self, set_to_none: bool = True):
        """Drop a pending batch; there are no gradients to clear."""
        self._pending = None

    def _states(self):
        """The state tensors in table order, on the tables' devices (moved
        there once if the tables were moved)."""
        if self.kind == "sgd":
            return []
        for t, w in enumerate(self.tables):
            st = self.state[t]
            if st["sum"].device != w.device:
                st["sum"] = st["sum"].to(w.device)
        return [self.state[t]["sum"] for t in range(len(self.tables))]

    @torch.no_grad()
    def step(self):
        """Apply the pending batch to the tables, in place."""
        import torch.distributed as dist

        if (dist.is_available() and dist.is_initialized()
                and dist.get_world_size() > 1):
            raise RuntimeError(
                "FusedEmbeddingOptimizer.step: more than one process; "
                "sparse gradients are not exchanged")
        if self._pending is None:
            raise RuntimeError(
                "FusedEmbeddingOptimizer.step: no pending batch (run "
                "fused_embedding(optimizer=) and backward first)")
        _check_opt_hyper(self.kind, self.lr, self.eps)
        dout, widx, served = self._pending
        states = self._states()
        hip = None
        if served:
            from ray_shuffling_data_loader_amd.ops import shuffle_ops

            hip = shuffle_ops._load_hip()
        if hip is not None and getattr(hip, "EMBED_OPTIM", 0) and all(
                h.is_contiguous() and h.data_ptr() % 16 == 0
                for h in states):
            self._step_hip(hip, dout, widx, states)
        else:
            self._step_torch(dout, widx, states)
        self._pending = None
        self.step_count += 1

    def _step_hip(self, hip, dout, widx, states):
        tables = [w.detach() for w in self.tables]
        cards = [int(w.shape[0]) for w in tables]
        offs, _ = _row_offsets(cards)
        hyper = (_OPT_KINDS[self.kind], float(self.lr), float(self.eps))
        dense = [t for t, c in enumerate(cards) if c <= _DENSE_MAX_ROWS]
        large = [t for t, c in enumerate(cards) if c > _DENSE_MAX_ROWS]

        def of(ts, seq):
            return [seq[t] for t in ts] if seq else []

        if dense:
            hip.embed_onehot_update(
                dout, widx, dense, of(dense, tables), of(dense, states),
                *hyper)
        if large:
            keys, pos = _sorted_keys(widx, cards, offs, large)
            hip.embed_runs_update(
                dout, widx, keys, pos, large, of(large, offs),
                of(large, tables), of(large, states), *hyper)

    def _step_torch(self, dout, widx, states):
        """The class docstring's list as unfused torch ops over the touched
        rows. Every operand is fp32, so each op rounds once, as the
        kernels' do."""
        D = int(self.tables[0].shape[1])
        G = D // 4
        lanes = D % 4 == 0 and G & (G - 1) == 0
        for t, w in enumerate(self.tables):
            w = w.detach()
            lr, eps = _f32(self.lr, w.device), _f32(self.eps, w.device)
            rows, inv = torch.unique(widx[:, t].long(), return_inverse=True)
            g = torch.zeros(rows.shape[0], D, dtype=torch.float32,
                            device=w.device)
            g.index_add_(0, inv, dout[:, t * D:(t + 1) * D].float())
            p = w[rows].float()
            if self.kind == "sgd":
                u = lr * g
                w[rows] = (p - u).to(w.dtype)
                continue
            h = states[t][rows]
            if self.kind == "adagrad":
                gg = g * g
                h = h + gg
                hd = h
            else:
                if lanes:
                    q = g.view(-1, G, 4)
                    xx = q[:, :, 0] * q[:, :, 0]
                    yy = q[:, :, 1] * q[:, :, 1]
                    zz = q[:, :, 2] * q[:, :, 2]
                    ww = q[:, :, 3] * q[:, :, 3]
                    xy = xx + yy
                    xyz = xy + zz
                    s = xyz + ww
                    lane = torch.arange(G, device=w.device)
                    d = 1
                    while d < G:
                        s = s + s[:, lane ^ d]
                        d *= 2
                    s = s[:, 0]
                else:
                    s = (g * g).sum(1)
                m = s * _f32(1.0 / D, w.device)
                h = h + m
                hd = h[:, None]
            states[t][rows] = h
            # torch's fp32 sqrt is not correctly rounded on every backend;
            # the fp64 one rounded to fp32 is, and equals the kernels' sqrt
            sv = torch.sqrt(hd.double()).float()
            den = sv + eps
            r = g / den
            u = lr * r
            w[rows] = (p - u).to(w.dtype)

    # -- checkpointing --------------------------------------------------

    def state_dict(self):
        return {
            "kind": self.kind,
            "hyper": {
                "lr": self.lr, "eps": self.eps,
                "initial_accumulator_value": self.initial_accumulator_value,
            },
            "step": self.step_count,
            "state": [
                {s: v.detach().clone() for s, v in self.state[t].items()}
                for t in range(len(self.tables))
            ],
        }

    def load_state_dict(self, sd):
        """Adopt kind, hyper-parameters, step count and state of ``sd``
        (exact copies on the tables' devices). Everything is checked before
        anything changes; a pending batch is dropped."""
        hy = sd["hyper"]
        _check_opt_hyper(sd["kind"], hy["lr"], hy["eps"],
                         hy["initial_accumulator_value"])
        if len(sd["state"]) != len(self.tables):
            raise ValueError(
                f"FusedEmbeddingOptimizer.load_state_dict: {len(sd['state'])}"
                f" tables, expected {len(self.tables)}")
        slots = () if sd["kind"] == "sgd" else ("sum",)
        for t, (st, w) in enumerate(zip(sd["state"], self.tables)):
            shape = (tuple(w.shape) if sd["kind"] == "adagrad"
                     else (w.shape[0],))
            if tuple(st) != slots or any(
                    st[s].shape != shape or st[s].dtype != torch.float32
                    for s in slots):
                raise ValueError(
                    f"FusedEmbeddingOptimizer.load_state_dict: table {t} "
                    f"needs state {slots} as fp32 {shape}")
        self.kind = sd["kind"]
        self.lr = hy["lr"]
        self.eps = hy["eps"]
        self.initial_accumulator_value = hy["initial_accumulator_value"]
        self.step_count = int(sd["step"])
        self.state = {
            t: {s: sd["state"][t][s].detach().to(w.device, copy=True)
                .contiguous() for s in slots}
            for t, w in enumerate(self.tables)
        }
        self._pending = None


def fused_embedding(indices, tables, optimizer=None) -> torch.Tensor:
    """bf16 [B, T*D] concat of ``tables[t][max(indices[t], 0) % card_t]``.

    ``indices``: T int64 tensors [B] or [B,1] with any row stride (column
    views of a packed batch are read in place), or one [B,T] matrix.
    ``tables``: T fp32 [card_t, D] tensors, e.g. ``nn.Embedding.weight``;
    D in {8, 16, 32, 64, 128} runs in HIP on GPU tensors.
    ``optimizer``: a ``FusedEmbeddingOptimizer`` bound to these tables; the
    backward then gives them no ``.grad`` and ``optimizer.step()`` applies
    the batch."""
    tables = list(tables)
    if not tables:
        raise ValueError("fused_embedding: needs at least one table")
    idx = _split(indices, len(tables))
    if optimizer is not None:
        optimizer._check_tables(tables)
        return _FusedEmbeddingOptFn.apply(
            optimizer, len(tables), *idx, *tables
        )
    return _FusedEmbeddingFn.apply(len(tables), *idx, *tables)


class FusedEmbeddingConcat(nn.Module):
    """``fused_embedding`` over a ``ModuleList`` of ``nn.Embedding``,
    optionally with a ``FusedEmbeddingOptimizer`` bound to their weights."""

    def __init__(self, embeddings: nn.ModuleList, optimizer=None):
        super().__init__()
        self.embeddings = embeddings
        self.optimizer = optimizer

    def forward(self, indices) -> torch.Tensor:
        return fused_embedding(
            indices, [e.weight for e in self.embeddings],
            optimizer=self.optimizer,
        )

