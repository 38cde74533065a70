"""Integer-valued cases and an exact fp64 oracle for the fused chain and
wgrad kernels (CPU only; shared by tests/test_exact_cases.py and
tests/test_chain_exact_gpu.py).

The kernels multiply bf16 values and accumulate in fp32. When every input
is a bf16-exact integer, every product is an integer, and when the sum of
the magnitudes of the terms of an accumulator (plus its bias) stays below
2^24, every partial sum in ANY order is an integer below 2^24 and hence
exact in fp32. What the kernel then emits is the bf16 rounding (round to
nearest, ties to even) of an exactly known number: it must equal this
oracle bit for bit, whatever the MFMA order, the split-K grouping or the
slab size. ``exactness_report`` measures the precondition;
tests/test_exact_cases.py asserts it for every case the GPU file runs.

The oracle is the network's mathematics in torch fp64 with a
``.float().bfloat16()`` wherever a kernel stores bf16:

    a_l  = bf16(relu(a_{l-1} W_l^T + b_l))         l = 1..3, a_0 = x
    out  = bf16(o),  o = a_3 w_4 + b_4             (o exact, fp32)
    dz_3 = bf16(dy w_4^T * [a_3 > 0])
    dz_l = bf16((dz_{l+1} W_{l+1}) * [a_l > 0])    l = 2, 1
    dW_l = dz_l^T a_{l-1},  dW_4 = dy^T a_3,  db_4 = sum dy

Bias gradients: csrc/bwd_chain.hip sums the fp32 value BEFORE its bf16
conversion (``colsum2 += v2`` ahead of ``bc_cvt_pk_bf16`` in bc_layer for
db1/db2; ``s3 += dz3v`` ahead of ``bc_f2b`` in the dz3 seed loop for db3),
so db_l here is the column sum of the unrounded masked dgrad. The sums of
the rounded dz are returned as ``db*_post``; the "wide" regime makes the two
differ, so the other reading fails.
"""

import functools

import torch

K0, N1, N2, N3 = 100, 512, 256, 128
LIMIT = float(2 ** 24)

# What tests/test_chain_exact_gpu.py runs and tests/test_exact_cases.py
# proves the precondition for.
SHAPES = [1, 31, 32, 33, 64, 65, 96, 97, 161]
FUSED_SHAPES = [64, 128]      # whole fused step: 2/M is a power of two
HEAD_SHAPES = [32, 64]        # stand-alone forward: dyb and loss_part exact
# Fragment wgrad: ring depth, chunk counts and shapes of
# tests/test_wgrad_lds_gpu.py; M = 16 * mchunks - 5 rows.
WGRAD_S = 6
WGRAD_MCHUNKS = [1, 2, WGRAD_S - 1, WGRAD_S, WGRAD_S + 1, 2 * WGRAD_S + 1,
                 1021, 4099]
WGRAD_SHAPES = [(256, 512, 1, 8), (128, 256, 1, 8), (512, 128, 2, 4)]
# The older GEMM kernels (wgrad_bf16: (m, n, k); relu_bwd_bias: (m, n)).
GEMM_SHAPES = [(1, 64, 100), (17, 1, 128), (255, 128, 256),
               (4099, 512, 100), (4099, 256, 512)]
RELU_BWD_SHAPES = [(3, 8), (257, 64), (4099, 512)]
INT_RANGE = 4                 # |entries| of the integer GEMM operands

# name -> draw parameters: symmetric integer ranges [-r, r] (biases b1..b4
# without 0; dy = (lo, hi) draws |dy| in [lo, hi] with a random sign, lo = 0
# the plain range; dy_big = (row, value) plants one large gradient).
REGIMES = {
    # nothing but a2, a3 and some dz1 pass 256; the head reaches 1.8e6
    "small": dict(x=4, W1=3, W2=2, W3=2, w4=2, balanced=False,
                  b=(8, 64, 512, 512), dy=(0, 2), dy_big=None, seed=1),
    # layer-1 outputs, dz2, dz1 (and, from row 20 on, a few dz3) also pass
    # 256 and get rounded; the weights are balanced (_balanced_weights) so
    # that the dW and head sums of 161 rows still stay under 2^24.
    "wide": dict(x=16, W1=5, w4=5, balanced=True, nnz2=8,
                 b=(64, 256, 512, 1024), dy=(18, 26), dy_big=(20, 101.0),
                 seed=1),
}


def _randint(g, r, *shape):
    return torch.randint(-r, r + 1, shape, generator=g).double()


def _balanced_weights(g, cfg):
    """Weights of the "wide" regime. With plain random draws a column of
    a2, a3 or dz2 carries a systematic part (all-positive activations times
    a row sum of W; dy w4^T W3 is rank one), and the largest column is 4-5x
    the mean: the dW sums of 161 rows then pass 2^24 long before 5 % of the
    elements pass 256. These draws have no such part:
      W2: ``nnz2`` entries per row, half +1 and half -1 (row sums 0);
      W3: rows in pairs (r, -r), r a permutation of equal counts of +1 and
          -1 and zeros (row sums 0); w4 equal within a pair, so that
          w4^T W3 = 0."""
    q = cfg["nnz2"] // 2
    pos = torch.rand(N2, N1, generator=g).argsort(1)
    W2 = torch.zeros(N2, N1, dtype=torch.float64)
    W2.scatter_(1, pos[:, :q], 1.0)
    W2.scatter_(1, pos[:, q:2 * q], -1.0)
    third = N2 // 3
    vals = torch.cat([torch.ones(third), -torch.ones(third),
                      torch.zeros(N2 - 2 * third)]).double()
    order = torch.rand(N3 // 2, N2, generator=g).argsort(1)
    base = vals[order]
    W3 = torch.stack([base, -base], 1).reshape(N3, N2)
    w4 = _randint(g, cfg["w4"], N3 // 2).repeat_interleave(2)
    return W2, W3, w4


def _bf16(t):
    return t.float().bfloat16()


@functools.lru_cache(maxsize=None)
def make_case(name, M, seed=None):
    """The case of regime ``name`` with M rows: a dict of
      x [M,100], W1 [512,100], W2 [256,512], W3 [128,256], w4 [128]  bf16
      b1 [512], b2 [256], b3 [128], b4 [1]                           fp32
      dy [M,1] bf16 (the backward's integer head gradient)
      d [M] fp64 (integers in [-8, 8]), target [M] fp32 = o - d, so the
        MSE head's diff is d
      eval_target [M] fp32: small integers, for the evaluator's sum t and
        sum t^2 partials to stay exact.
    Weights depend on (name, seed) alone; the per-row data is the leading
    M rows of one draw. Cached: treat the tensors as read-only."""
    cfg = REGIMES[name]
    seed = cfg["seed"] if seed is None else seed
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + 7)
    W1 = _randint(g, cfg["W1"], N1, K0)
    if not cfg["balanced"]:
        W2 = _randint(g, cfg["W2"], N2, N1)
        W3 = _randint(g, cfg["W3"], N3, N2)
        w4 = _randint(g, cfg["w4"], N3)
    else:
        W2, W3, w4 = _balanced_weights(g, cfg)
    bs = [_randint(g, r, n) for r, n in zip(cfg["b"], (N1, N2, N3, 1))]
    for b in bs:
        b[b == 0] = 1.0  # a dropped bias must change the result
    rows = max(M, 161)
    x = _randint(g, cfg["x"], rows, K0)
    lo, hi = cfg["dy"]
    if lo == 0:
        dy = _randint(g, hi, rows, 1)
    else:
        mag = torch.randint(lo, hi + 1, (rows, 1), generator=g).double()
        sign = torch.randint(0, 2, (rows, 1), generator=g).double() * 2 - 1
        dy = mag * sign
    if cfg["dy_big"] is not None:
        dy[cfg["dy_big"][0]] = cfg["dy_big"][1]
    # d in [-8, 8], a quarter of the rows uniform over the whole range and
    # the rest in [-2, 2]: keeps sum |d| a3 (dW4 of the whole fused step,
    # where dy = (2/M) d) under 2^24 at M = 128
    d = torch.where(torch.rand(rows, generator=g) < 0.25,
                    _randint(g, 8, rows), _randint(g, 2, rows))
    et = _randint(g, 256, rows)
    case = {
        "name": name, "M": M,
        "x": _bf16(x[:M]), "W1": _bf16(W1), "W2": _bf16(W2),
        "W3": _bf16(W3), "w4": _bf16(w4),
        "b1": bs[0].float(), "b2": bs[1].float(), "b3": bs[2].float(),
        "b4": bs[3].float(),
        "dy": _bf16(dy[:M]), "d": d[:M].clone(),
        "eval_target": et[:M].float(),
    }
    for k in ("x", "W1", "W2", "W3", "w4", "dy"):
        src = {"x": x[:M], "W1": W1, "W2": W2, "W3": W3, "w4": w4,
               "dy": dy[:M]}[k]
        assert torch.equal(case[k].double(), src), k  # bf16-exact draws
    o = _forward(case)["out_fp32"]
    case["target"] = (o.double() - case["d"]).float()
    assert torch.equal(case["target"].double(), o.double() - case["d"])
    return case


def fused_dy(case):
    """The MSE head's gradient for ``target``: bf16((2/M) d). Exact (and
    what the fused step feeds its backward) when M is a power of two."""
    M = case["M"]
    assert M & (M - 1) == 0
    return _bf16((2.0 / M) * case["d"]).reshape(M, 1)


def _forward(case):
    x = case["x"].double()
    z1 = x @ case["W1"].double().t() + case["b1"].double()
    a1 = _bf16(torch.relu(z1))
    z2 = a1.double() @ case["W2"].double().t() + case["b2"].double()
    a2 = _bf16(torch.relu(z2))
    z3 = a2.double() @ case["W3"].double().t() + case["b3"].double()
    a3 = _bf16(torch.relu(z3))
    o = a3.double() @ case["w4"].double() + case["b4"].double()
    return {
        "z1": z1, "z2": z2, "z3": z3, "a1": a1, "a2": a2, "a3": a3,
        "mask1": a1 > 0, "mask2": a2 > 0, "mask3": a3 > 0,
        "out_fp32": o.float(), "out": _bf16(o).reshape(-1, 1),
    }


def reference(case, dy=None):
    """Everything the kernels emit for ``case``, exactly (see the module
    docstring). ``dy`` [M,1] bf16 overrides the case's integer head
    gradient (``fused_dy(case)`` for the whole fused step). Also returns
    the unrounded stage values z1..z3 / dz*_pre (fp64) and db*_post."""
    r = _forward(case)
    assert torch.equal(r["out_fp32"].double(),
                       r["a3"].double() @ case["w4"].double()
                       + case["b4"].double())
    dy = (case["dy"] if dy is None else dy).double().reshape(-1, 1)
    w4 = case["w4"].double()
    pre3 = dy * w4.view(1, -1) * r["mask3"].double()
    dz3 = _bf16(pre3)
    pre2 = (dz3.double() @ case["W3"].double()) * r["mask2"].double()
    dz2 = _bf16(pre2)
    pre1 = (dz2.double() @ case["W2"].double()) * r["mask1"].double()
    dz1 = _bf16(pre1)
    r.update({
        "dy": dy, "dz3_pre": pre3, "dz2_pre": pre2, "dz1_pre": pre1,
        "dz3": dz3, "dz2": dz2, "dz1": dz1,
        "db1": pre1.sum(0), "db2": pre2.sum(0), "db3": pre3.sum(0),
        "db4": dy.sum(0),
        "db1_post": dz1.double().sum(0), "db2_post": dz2.double().sum(0),
        "db3_post": dz3.double().sum(0),
        "dW4": dy.t() @ r["a3"].double(),
        "dW3": dz3.double().t() @ r["a2"].double(),
        "dW2": dz2.double().t() @ r["a1"].double(),
        "dW1": dz1.double().t() @ case["x"].double(),
        # MSE head on ``target``: diff = d
        "loss_terms": case["d"] ** 2,
        "loss": (case["d"] ** 2).sum() / case["M"],
    })
    return r


def slab_sums(v, rows):
    """[M] -> the sums over consecutive slabs of ``rows`` rows (fp64)."""
    M = v.numel()
    n = (M + rows - 1) // rows
    pad = torch.zeros(n * rows, dtype=torch.float64)
    pad[:M] = v.double()
    return pad.view(n, rows).sum(1)


def rounding_stats(pre, post):
    """Share of elements the bf16 conversion changed, and the counts of
    exact ties (pre halfway between two bf16 neighbours) that went up and
    down in magnitude."""
    pre = pre.double()
    post = post.double()
    rounded = pre != post
    # pre is a tie iff its mirror image through pre of the chosen value is
    # the bf16 neighbour on the other side: a value strictly nearer to
    # post than half the gap mirrors into the open gap, where nothing is
    # bf16-exact (also across a power of two, where the gap below is half
    # the gap above).
    other = 2 * pre - post
    tie = rounded & (_bf16(other).double() == other)
    up = tie & (post.abs() > pre.abs())
    down = tie & (post.abs() < pre.abs())
    return {
        "rounded": rounded.double().mean().item(),
        "ties_up": int(up.sum()), "ties_down": int(down.sum()),
    }


def exactness_report(case, ref=None, granule=1.0):
    """For every accumulator class the largest sum of the magnitudes of its
    terms (plus |bias|), and per emitted bf16 tensor the rounding
    statistics. ``granule``: the power of two every backward quantity is a
    multiple of (1 for the integer dy; 2/M for ``fused_dy``); the backward
    bounds are reported in units of it, which is what must stay below
    2^24 for the sums to be exact."""
    ref = reference(case) if ref is None else ref
    A = torch.abs
    x, a1, a2, a3 = (case["x"].double(), ref["a1"].double(),
                     ref["a2"].double(), ref["a3"].double())
    W1, W2, W3, w4 = (case[k].double() for k in ("W1", "W2", "W3", "w4"))
    dy = ref["dy"]
    dz1, dz2, dz3 = (ref[k].double() for k in ("dz1", "dz2", "dz3"))
    m1, m2, m3 = (ref[k].double() for k in ("mask1", "mask2", "mask3"))
    bounds = {
        "fwd1": (A(x) @ A(W1).t() + A(case["b1"].double())).max(),
        "fwd2": (A(a1) @ A(W2).t() + A(case["b2"].double())).max(),
        "fwd3": (A(a2) @ A(W3).t() + A(case["b3"].double())).max(),
        "head": (A(a3) @ A(w4) + A(case["b4"].double())).max(),
        # o - target: both operands and the result are integers
        "head_diff": torch.maximum(A(ref["out_fp32"].double()),
                                   A(case["target"].double())).max(),
        "loss": slab_sums(ref["loss_terms"], 64).max(),
        "dgrad2": (A(dz3) @ A(W3)).max() / granule,
        "dgrad1": (A(dz2) @ A(W2)).max() / granule,
        "db1": A(ref["dz1_pre"]).sum(0).max() / granule,
        "db2": A(ref["dz2_pre"]).sum(0).max() / granule,
        "db3": A(ref["dz3_pre"]).sum(0).max() / granule,
        "db4": A(dy).sum() / granule,
        "dW4": (A(dy).t() @ A(a3)).max() / granule,
        "dW3": (A(dz3).t() @ A(a2)).max() / granule,
        "dW2": (A(dz2).t() @ A(a1)).max() / granule,
        "dW1": (A(dz1).t() @ A(x)).max() / granule,
    }
    # the evaluator's partials on eval_target, per 64-row slab (a 32-row
    # slab sums a subset)
    et = case["eval_target"].double()
    ed = ref["out_fp32"].double() - et
    bounds["eval_abs"] = slab_sums(A(ed), 64).max()
    bounds["eval_t"] = slab_sums(A(et), 64).max()
    bounds["eval_tt"] = slab_sums(et ** 2, 64).max()
    bounds = {k: float(v) for k, v in bounds.items()}
    rounding = {
        "a1": rounding_stats(torch.relu(ref["z1"]), ref["a1"]),
        "a2": rounding_stats(torch.relu(ref["z2"]), ref["a2"]),
        "a3": rounding_stats(torch.relu(ref["z3"]), ref["a3"]),
        "out": rounding_stats(ref["out_fp32"], ref["out"].reshape(-1)),
        "dz3": rounding_stats(ref["dz3_pre"], ref["dz3"]),
        "dz2": rounding_stats(ref["dz2_pre"], ref["dz2"]),
        "dz1": rounding_stats(ref["dz1_pre"], ref["dz1"]),
    }
    alive = {"a1": m1.mean().item(), "a2": m2.mean().item(),
             "a3": m3.mean().item()}
    return {"bounds": bounds, "rounding": rounding, "alive": alive}


def int_matrix(m, n, seed, r=INT_RANGE):
    """Seeded integer-valued bf16 [m, n] with entries in [-r, r]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    # drawn narrow: the largest operand has 3.4e7 entries
    return torch.randint(-r, r + 1, (m, n), generator=g,
                         dtype=torch.int8).to(torch.bfloat16)
