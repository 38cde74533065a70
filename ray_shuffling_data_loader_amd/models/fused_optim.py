"""SGD and AdamW for the fused train step of the stock
TabularMLP(100-512-256-128-1), applied by the step's own kernels
(csrc/step_glue.hip).

``fused_step(model, x, y, optimizer=opt)`` ends in step_finalize_update:
the thread that finishes a gradient element also owns the parameter
element, so it updates the fp32 master and the optimizer state in place
and writes the bf16 image of the new weight where step_prep would put it.
The step then needs no optimizer launch and, from the second step on, no
step_prep. ``opt.step()`` applies the same update from the parameters'
``.grad`` with one launch of step_update (finalize -> all-reduce ->
update, grad_hook steps, gradients from elsewhere); the two are
bit-identical.

The arithmetic, one fp32 IEEE operation per line, nothing fused (``h`` are
the hyper-parameters rounded to fp32; scalars that depend on the step
count t are formed in fp64 first and rounded once):

  SGD   (momentum mu, weight_decay wd, nesterov; no dampening)
    g  = g * grad_scale
    g  = g + wd * p                     (skipped when wd == 0)
    b  = mu * b + g                     (b starts as zeros; skipped when
                                         mu == 0)
    d  = g + mu * b  if nesterov else b (d = g when mu == 0)
    p' = p - lr * d

  AdamW (betas, eps, decoupled weight_decay; weight_decay=0 is Adam)
    c1 = 1 - lr*wd, a1 = 1 - beta1, a2 = 1 - beta2,
    s = lr / (1 - beta1^t), q = sqrt(1 - beta2^t)
    g  = g * grad_scale
    p  = p * c1
    m' = m + a1 * (g - m)
    v' = beta2 * v + a2 * (g * g)
    p' = p - s * (m' / (sqrt(v') / q + eps))

Staging validity. The optimizer owns six persistent bf16 buffers in the
layout of hip.step_prep and remembers the ``(_version, data_ptr())`` of the
four weights for which they hold the images. The update kernels keep
buffers and key current (the extension bumps the version counters of what
it wrote). A weight changed behind the optimizer's back — ``p.mul_``,
``load_state_dict``, a replaced tensor — no longer matches the key, and
the next fused step restages through step_prep once. A write through
``p.data`` bypasses the version counter and is not seen, as for
FusedEvaluator.

On CPU tensors, or with an extension without ``STEP_OPTIM``, ``step()``
runs the same list of operations as unfused torch ops (bit-identical to
the kernels, which tests/_optim_cases.py pins from both sides), and
``fused_step(optimizer=)`` is ``fused_step`` followed by ``step()``.

Not offered: graph capture of a step with ``optimizer=`` (the AdamW
scalars that depend on t are launch arguments), gradient clipping,
per-group hyper-parameters, dampening, amsgrad, feature widths other than
100.
"""

import math

import torch

from ray_shuffling_data_loader_amd.models import fused_step as _fs

_KINDS = {"sgd": 0, "adamw": 1}
# step_prep output order: W1s (K padded to 112), W2s, W3s, W2^T s, W3^T s,
# w4 bf16.
_STAGE_NUMEL = (512 * 112, 256 * 512, 128 * 256, 256 * 512, 128 * 256, 128)


def _f32(v: float) -> float:
    """``v`` rounded to fp32, as the kernels receive it."""
    return torch.tensor(float(v), dtype=torch.float32).item()


def _check_hyper(kind, lr, momentum, nesterov, weight_decay, betas, eps):
    if kind not in _KINDS:
        raise ValueError(
            f"FusedOptimizer: kind must be 'sgd' or 'adamw', got {kind!r}")
    vals = {"lr": lr, "momentum": momentum, "weight_decay": weight_decay,
            "eps": eps}
    for name, v in vals.items():
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
            raise ValueError(
                f"FusedOptimizer: {name} must be finite and >= 0, got {v!r}")
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(
            f"FusedOptimizer: betas must be two values in [0, 1), got "
            f"{betas!r}")
    if nesterov and (kind != "sgd" or _f32(momentum) == 0.0):
        raise ValueError(
            "FusedOptimizer: nesterov needs kind='sgd' and a momentum")


class FusedOptimizer:
    """``FusedOptimizer(model, kind="sgd"|"adamw", lr=, momentum=0,
    nesterov=False, weight_decay=0, betas=(0.9, 0.999), eps=1e-8)`` for
    the stock TabularMLP(100); see the module docstring.

    ``lr`` and the other scalars are plain attributes read at every step,
    so schedules work; only whether SGD has a momentum buffer is fixed at
    construction. ``state`` maps each parameter's name to its fp32 state
    tensors (``momentum_buffer`` / ``exp_avg``, ``exp_avg_sq``), zeros at
    the start."""

    def __init__(self, model, kind: str = "sgd", lr: float = 1e-3,
                 momentum: float = 0.0, nesterov: bool = False,
                 weight_decay: float = 0.0, betas=(0.9, 0.999),
                 eps: float = 1e-8):
        _check_hyper(kind, lr, momentum, nesterov, weight_decay, betas, eps)
        try:
            self._lin = _fs._layers(model)
        except AssertionError as e:
            raise ValueError(
                "FusedOptimizer: needs the stock TabularMLP(100)") from e
        self.model = model
        self.kind = kind
        self.lr = lr
        self.momentum = momentum
        self.nesterov = bool(nesterov)
        self.weight_decay = weight_decay
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = eps
        self.step_count = 0
        names = {id(p): n for n, p in model.named_parameters()}
        self._names = [names[id(p)] for p in self._params()]
        self.state = {}
        self._init_state()
        self._staged = None
        self._stage_key = None

    # -- parameters, state, staging ------------------------------------

    def _params(self):
        """W1, W2, W3, w4, b1..b4: the order of the extension."""
        return ([m.weight for m in self._lin]
                + [m.bias for m in self._lin])

    def _slots(self):
        if self.kind == "adamw":
            return ("exp_avg", "exp_avg_sq")
        return ("momentum_buffer",) if _f32(self.momentum) != 0.0 else ()

    def _init_state(self):
        slots = self._slots()
        self.state = {
            n: {s: torch.zeros_like(p, dtype=torch.float32,
                                    memory_format=torch.contiguous_format)
                for s in slots}
            for n, p in zip(self._names, self._params())
        }

    def _state_list(self, params):
        """State tensors slot-major in parameter order, on the parameters'
        device (moved there once if the model was moved)."""
        slots = tuple(next(iter(self.state.values())).keys())
        if slots != self._slots():
            raise RuntimeError(
                "FusedOptimizer: momentum changed between zero and "
                "non-zero after construction")
        for n, p in zip(self._names, params):
            st = self.state[n]
            for s in slots:
                if st[s].device != p.device:
                    st[s] = st[s].to(p.device)
        return [self.state[n][s] for s in slots for n in self._names]

    def _hyper(self, grad_scale: float, t: int):
        """h[] of csrc/step_glue.h for step ``t`` (1-based), in fp64; the
        extension (or _step_torch) rounds each to fp32 once."""
        if self.kind == "sgd":
            return [float(grad_scale), float(self.lr), float(self.momentum),
                    float(self.weight_decay), 1.0 if self.nesterov else 0.0]
        b1, b2 = self.betas
        lr = float(self.lr)
        return [
            float(grad_scale),
            1.0 - lr * float(self.weight_decay),
            1.0 - b1,
            b2,
            1.0 - b2,
            lr / (1.0 - b1 ** t),
            math.sqrt(1.0 - b2 ** t),
            float(self.eps),
        ]

    def _native(self, hip, params) -> bool:
        """Whether the update kernels can run: the extension has them and
        the fp32 parameters sit on a GPU as the kernels read them."""
        if not (_fs._NATIVE_GLUE and getattr(hip, "STEP_OPTIM", 0)):
            return False
        return all(
            p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
            and p.data_ptr() % 16 == 0
            for p in params
        )

    def _stage_bufs(self, dev):
        if self._staged is None or self._staged[0].device != dev:
            # zeros: W1s columns 100..111 are never written by the update
            self._staged = [
                torch.zeros(n, dtype=torch.bfloat16, device=dev)
                for n in _STAGE_NUMEL
            ]
            self._stage_key = None
        return self._staged

    @staticmethod
    def _key(params):
        return tuple((w._version, w.data_ptr()) for w in params[:4])

    def _opt_arg(self, params):
        """``opt=`` of hip.fused_step_bf16 for the step about to run."""
        bufs = self._stage_bufs(params[0].device)
        valid = (self._stage_key is not None
                 and self._stage_key == self._key(params))
        return (self._state_list(params), bufs, valid, _KINDS[self.kind],
                self._hyper(1.0, self.step_count + 1))

    def _updated(self, params):
        """After a native update: it counted as a step, and the staged
        buffers hold the images of the weights as they are now."""
        self.step_count += 1
        self._stage_key = self._key(params)

    # -- the update -----------------------------------------------------

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        """Apply the update from the parameters' ``.grad`` (each first
        multiplied by ``grad_scale``, e.g. 1/world after a summing
        all-reduce). One launch of hip.step_update on the native path."""
        from ray_shuffling_data_loader_amd.ops.shuffle_ops import _load_hip

        params = self._params()
        grads = [p.grad for p in params]
        if any(g is None for g in grads):
            raise RuntimeError("FusedOptimizer.step: a parameter has no .grad")
        hyper = self._hyper(grad_scale, self.step_count + 1)
        state = self._state_list(params)
        hip = _load_hip()
        if self._native(hip, params) and all(
                g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
                and (i >= 3 or g.data_ptr() % 16 == 0)
                for i, g in enumerate(grads)):
            hip.step_update(
                grads, [p.detach() for p in params[:4]],
                [p.detach() for p in params[4:]], state,
                self._stage_bufs(params[0].device), _KINDS[self.kind], hyper)
            self._updated(params)
            return
        self._step_torch(params, grads, state, hyper)
        self.step_count += 1
        self._stage_key = None

    def _step_torch(self, params, grads, state, hyper):
        """The module docstring's list as unfused torch ops, one per line.
        Every operand is fp32 (``h`` as 0-dim tensors), so each op rounds
        once, as the kernels' do."""
        n = len(params)
        for i, (p, g) in enumerate(zip(params, grads)):
            h = [torch.tensor(v, dtype=torch.float32, device=p.device)
                 for v in hyper]
            g = g.to(torch.float32) * h[0]
            if self.kind == "sgd":
                lr, mu, wd = h[1], h[2], h[3]
                if float(wd) != 0.0:
                    wp = wd * p
                    g = g + wp
                d = g
                if float(mu) != 0.0:
                    b = state[i]
                    mb = mu * b
                    b.copy_(mb + g)
                    if float(h[4]) != 0.0:
                        nb = mu * b
                        d = g + nb
                    else:
                        d = b
                u = lr * d
                p.copy_(p - u)
            else:
                m, v = state[i], state[n + i]
                pc = p * h[1]
                gm = g - m
                am = h[2] * gm
                m.copy_(m + am)
                bv = h[3] * v
                gg = g * g
                ag = h[4] * gg
                v.copy_(bv + ag)
                # torch's fp32 sqrt is not correctly rounded on every
                # backend; the fp64 one rounded to fp32 is (53 >= 2*24+2
                # bits), and equals the kernels' sqrt
                sv = torch.sqrt(v.double()).float()
                dq = sv / h[6]
                den = dq + h[7]
                r = m / den
                u = h[5] * r
                p.copy_(pc - u)

    def zero_grad(self, set_to_none: bool = False):
        """Nothing to do, and nothing launched: every step writes every
        gradient element."""

    # -- checkpointing --------------------------------------------------

    def state_dict(self):
        return {
            "kind": self.kind,
            "hyper": {
                "lr": self.lr, "momentum": self.momentum,
                "nesterov": self.nesterov,
                "weight_decay": self.weight_decay, "betas": self.betas,
                "eps": self.eps,
            },
            "step": self.step_count,
            "state": {
                n: {s: t.detach().clone() for s, t in st.items()}
                for n, st in self.state.items()
            },
        }

    def load_state_dict(self, sd):
        """Adopt kind, hyper-parameters, step count and state of ``sd``
        (exact copies, moved to the parameters' device). Everything is
        checked before anything changes; the staging is invalidated."""
        hy = sd["hyper"]
        _check_hyper(sd["kind"], hy["lr"], hy["momentum"], hy["nesterov"],
                     hy["weight_decay"], hy["betas"], hy["eps"])
        if sd["kind"] == "adamw":
            slots = ("exp_avg", "exp_avg_sq")
        else:
            slots = (("momentum_buffer",)
                     if _f32(hy["momentum"]) != 0.0 else ())
        params = self._params()
        if set(sd["state"]) != set(self._names):
            raise ValueError(
                "FusedOptimizer.load_state_dict: parameter names differ: "
                f"{sorted(sd['state'])} vs {sorted(self._names)}")
        for n, p in zip(self._names, params):
            st = sd["state"][n]
            if tuple(st) != slots:
                raise ValueError(
                    f"FusedOptimizer.load_state_dict: {n} has state "
                    f"{tuple(st)}, expected {slots}")
            for s in slots:
                if (st[s].shape != p.shape
                        or st[s].dtype != torch.float32):
                    raise ValueError(
                        f"FusedOptimizer.load_state_dict: {n}.{s} must be "
                        f"fp32 {tuple(p.shape)}")
        self.kind = sd["kind"]
        self.lr = hy["lr"]
        self.momentum = hy["momentum"]
        self.nesterov = bool(hy["nesterov"])
        self.weight_decay = hy["weight_decay"]
        self.betas = (float(hy["betas"][0]), float(hy["betas"][1]))
        self.eps = hy["eps"]
        self.step_count = int(sd["step"])
        self.state = {
            n: {s: sd["state"][n][s].detach().to(p.device, copy=True)
                .contiguous()
                for s in slots}
            for n, p in zip(self._names, params)
        }
        self._stage_key = None
