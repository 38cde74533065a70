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

On CPU tensors, or for an input the kernels do not serve (D outside
{8, 16, 32}, more than 64 tables, non-fp32 tables, B = 0), the same
arithmetic runs as torch ops: gather, cast and cat forward, an fp32
``index_add_`` of the bf16 gradients backward (ascending batch row on CPU).
"""

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


def _kernels_serve(idx, tables) -> bool:
    T = len(tables)
    w0 = tables[0]
    if not (1 <= T <= _MAX_TABLES) or not w0.is_cuda or w0.dim() != 2:
        return False
    D, B = w0.shape[1], idx[0].shape[0]
    if D not in _WIDTHS or B < 1:
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


class _FusedEmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, *args):
        idx, tables = list(args[:T]), list(args[T:])
        ctx.cards = [int(w.shape[0]) for w in tables]
        ctx.D = int(tables[0].shape[1])
        ctx.hip = _kernels_serve(idx, tables)
        need = any(ctx.needs_input_grad[1 + T:])
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
        key = (dout.device, tuple(cards), tuple(large))
        if key not in _KEY_CACHE:
            _KEY_CACHE[key] = (
                torch.tensor(large, device=dout.device),
                torch.tensor([offs[t] for t in large], dtype=torch.int32,
                             device=dout.device)[:, None],
            )
        cols, roff = _KEY_CACHE[key]
        # int32 [L, B]: the flat gradient row of every (table, batch row)
        keys = widx.t().index_select(0, cols).add_(roff).reshape(-1)
        keys, pos = torch.sort(keys, stable=True)
        hip.embed_bwd_runs(dout, widx, flat, keys, pos, large)


def fused_embedding(indices, tables) -> torch.Tensor:
    """bf16 [B, T*D] concat of ``tables[t][max(indices[t], 0) % card_t]``.

    ``indices``: T int64 tensors [B] or [B,1] with any row stride (column
    views of a packed batch are read in place), or one [B,T] matrix.
    ``tables``: T fp32 [card_t, D] tensors, e.g. ``nn.Embedding.weight``."""
    tables = list(tables)
    if not tables:
        raise ValueError("fused_embedding: needs at least one table")
    idx = _split(indices, len(tables))
    return _FusedEmbeddingFn.apply(len(tables), *idx, *tables)


class FusedEmbeddingConcat(nn.Module):
    """``fused_embedding`` over a ``ModuleList`` of ``nn.Embedding``."""

    def __init__(self, embeddings: nn.ModuleList):
        super().__init__()
        self.embeddings = embeddings

    def forward(self, indices) -> torch.Tensor:
        return fused_embedding(
            indices, [e.weight for e in self.embeddings]
        )
