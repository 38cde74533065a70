"""Oracle of the fused optimizer (models/fused_optim.py, csrc/step_glue.hip),
written from the specification, not from the kernel: numpy, fp32, one
``np.float32`` operation per line.

  SGD    g = g*gs; g = g + wd*p (wd != 0); b = mu*b + g (mu != 0);
         d = g + mu*b if nesterov else b (d = g when mu == 0); p' = p - lr*d
  AdamW  host, fp64, rounded to fp32 once: c1 = 1 - lr*wd, a1 = 1 - beta1,
         a2 = 1 - beta2, s = lr / (1 - beta1^t), q = sqrt(1 - beta2^t)
         g = g*gs; p = p*c1; m' = m + a1*(g - m); v' = beta2*v + a2*(g*g);
         p' = p - s*(m' / (sqrt(v') / q + eps))

Also the fragment swizzles of the staged bf16 weight buffers as index
constructions (as _swz / _swz_t of tests/test_step_glue_gpu.py) and the
bf16 rounding as the integer formula of Tensor.bfloat16().

Parameter order everywhere: W1, W2, W3, w4, b1, b2, b3, b4.
"""

import math

import numpy as np

f32 = np.float32

SHAPES = [(512, 100), (256, 512), (128, 256), (1, 128), (512,), (256,),
          (128,), (1,)]


def sgd_hyper(grad_scale, lr, momentum=0.0, weight_decay=0.0,
              nesterov=False):
    return dict(gs=f32(grad_scale), lr=f32(lr), mu=f32(momentum),
                wd=f32(weight_decay), nesterov=bool(nesterov))


def adamw_hyper(t, grad_scale, lr, betas=(0.9, 0.999), eps=1e-8,
                weight_decay=0.0):
    b1, b2 = float(betas[0]), float(betas[1])
    lr = float(lr)
    return dict(
        gs=f32(grad_scale),
        c1=f32(1.0 - lr * float(weight_decay)),
        a1=f32(1.0 - b1),
        b2=f32(b2),
        a2=f32(1.0 - b2),
        s=f32(lr / (1.0 - b1 ** t)),
        q=f32(math.sqrt(1.0 - b2 ** t)),
        eps=f32(eps),
    )


def sgd(g, p, b, h):
    """(p', b') of fp32 arrays g, p, b (b ignored and returned as is when
    mu == 0)."""
    assert g.dtype == p.dtype == f32
    with np.errstate(all="ignore"):
        g = g * h["gs"]
        if h["wd"] != 0:
            wp = h["wd"] * p
            g = g + wp
        d = g
        if h["mu"] != 0:
            mb = h["mu"] * b
            b = mb + g
            if h["nesterov"]:
                nb = h["mu"] * b
                d = g + nb
            else:
                d = b
        u = h["lr"] * d
        p = p - u
    assert p.dtype == f32
    return p, b


def adamw(g, p, m, v, h):
    """(p', m', v') of fp32 arrays."""
    assert g.dtype == p.dtype == m.dtype == v.dtype == f32
    with np.errstate(all="ignore"):
        g = g * h["gs"]
        p = p * h["c1"]
        gm = g - m
        am = h["a1"] * gm
        m = m + am
        bv = h["b2"] * v
        gg = g * g
        ag = h["a2"] * gg
        v = bv + ag
        sv = np.sqrt(v)
        dq = sv / h["q"]
        den = dq + h["eps"]
        r = m / den
        u = h["s"] * r
        p = p - u
    assert p.dtype == m.dtype == v.dtype == f32
    return p, m, v


class Oracle:
    """Eight fp32 parameters, their state and the step count."""

    def __init__(self, kind, params, momentum=0.0, nesterov=False,
                 weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
        assert kind in ("sgd", "adamw")
        self.kind = kind
        self.p = [np.array(p, dtype=f32) for p in params]
        self.s1 = [np.zeros_like(p) for p in self.p]
        self.s2 = [np.zeros_like(p) for p in self.p]
        self.t = 0
        self.momentum, self.nesterov = momentum, nesterov
        self.weight_decay, self.betas, self.eps = weight_decay, betas, eps

    def step(self, grads, lr, grad_scale=1.0):
        self.t += 1
        if self.kind == "sgd":
            h = sgd_hyper(grad_scale, lr, self.momentum, self.weight_decay,
                          self.nesterov)
        else:
            h = adamw_hyper(self.t, grad_scale, lr, self.betas, self.eps,
                            self.weight_decay)
        for i, g in enumerate(grads):
            g = np.asarray(g, dtype=f32).reshape(self.p[i].shape)
            if self.kind == "sgd":
                self.p[i], self.s1[i] = sgd(g, self.p[i], self.s1[i], h)
            else:
                self.p[i], self.s1[i], self.s2[i] = adamw(
                    g, self.p[i], self.s1[i], self.s2[i], h)


# ---------------------------------------------------------------------
# bf16 images and fragment layouts
# ---------------------------------------------------------------------


def bf16_bits(x):
    """fp32 -> bf16 bits (uint16), round to nearest even, NaN -> 0x7FC0."""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, np.uint16(0x7FC0), r)


def swz(W):
    """[N,K] -> [N/32][K/16][2][32][8]: element (a,c,h,r,e) is
    W[a*32+r][c*16+h*8+e]."""
    N, K = W.shape
    return np.ascontiguousarray(
        W.reshape(N // 32, 32, K // 16, 2, 8).transpose(0, 2, 3, 1, 4)
    ).reshape(-1)


def swz_t(W):
    """Model-layout W [K,N] -> the fragment-major layout of W^T: element
    (a,c,h,r,e) is W[c*16+h*8+e][a*32+r]."""
    K, N = W.shape
    return np.ascontiguousarray(
        W.reshape(K // 16, 2, 8, N // 32, 32).transpose(3, 0, 1, 4, 2)
    ).reshape(-1)


def staged(params):
    """The six staged buffers (uint16 bf16 bits) of the fp32 weights:
    W1s (K padded 100 -> 112 with zeros), W2s, W3s, W2^T s, W3^T s, w4."""
    b = [bf16_bits(p) for p in params[:4]]
    w1p = np.zeros((512, 112), dtype=np.uint16)
    w1p[:, :100] = b[0]
    return [swz(w1p), swz(b[1]), swz(b[2]), swz_t(b[1]), swz_t(b[2]),
            b[3].reshape(-1)]


def w1s_pad(w1s):
    """The elements of a W1s buffer that image columns 100..111."""
    v = np.asarray(w1s).reshape(16, 7, 2, 32, 8)
    return np.concatenate([v[:, 6, 1].reshape(-1),
                           v[:, 6, 0, :, 4:].reshape(-1)])


def same_f32(got, want):
    """Bit equality of fp32 arrays, except that any NaN equals any NaN
    (payload and sign of a generated NaN differ between processors)."""
    got = np.ascontiguousarray(got, dtype=f32).reshape(-1)
    want = np.ascontiguousarray(want, dtype=f32).reshape(-1)
    if got.shape != want.shape:
        return False
    eq = got.view(np.uint32) == want.view(np.uint32)
    return bool(np.all(eq | (np.isnan(got) & np.isnan(want))))
