"""Optimizer-side fused ops: multi-tensor AdamW (K11) and grad-norm clip (K12).

`AdamW` matches `torch.optim.AdamW` semantics exactly (decoupled weight
decay, bias correction, state dict layout with `exp_avg`/`exp_avg_sq` per
param — the layout `optimizer_reset` relies on, reference
training_utils.py:305-361). On ROCm GPUs the step runs as one hand-written
multi-tensor HIP kernel per (device, dtype) group; elsewhere it uses
torch._foreach_* (still vectorized, used by CPU tests as the oracle).

`clip_grad_norm_` reproduces `torch.nn.utils.clip_grad_norm_(...,
error_if_nonfinite=True)` (reference torchrun_main.py:805-808) with a fused
multi-tensor L2-norm + scale on GPU.
"""

import math

import numpy as np
import torch

from relora_amd.ops import hip, philox

_ROUNDINGS = ("nearest", "stochastic")


def adamw_reference_update(p, g, m, v, *, lr, beta1, beta2, eps, wd, step,
                           math_dtype=torch.float32):
    """One AdamW update in `math_dtype`, unrounded: returns the new
    (param, exp_avg, exp_avg_sq) as `math_dtype` tensors, inputs untouched.

    In float32 this follows the kernels' operation order, with the scalars
    (decay, bias corrections, step size) formed in float32 as the kernel
    launch does; float64 gives tests a reference value."""
    f = np.float32 if math_dtype == torch.float32 else np.float64
    one = f(1)
    lr_, b1, b2, eps_, wd_ = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    bc1 = one - f(np.power(b1, f(step)))
    bc2 = one - f(np.power(b2, f(step)))
    decay = one - lr_ * wd_
    step_size = lr_ / bc1
    inv_bc2 = one / bc2
    pf = p.detach().to(math_dtype) * float(decay)
    gf = g.detach().to(math_dtype)
    mf = float(b1) * m.detach().to(math_dtype) + float(one - b1) * gf
    vf = float(b2) * v.detach().to(math_dtype) + float(one - b2) * gf * gf
    denom = (vf * float(inv_bc2)).sqrt() + float(eps_)
    return pf - float(step_size) * mf / denom, mf, vf


class AdamW(torch.optim.Optimizer):
    """AdamW with optional fp32 moments and stochastic rounding for bf16
    parameters.

    `state_dtype=torch.float32` keeps `exp_avg` / `exp_avg_sq` of bf16
    parameters in fp32 (`None`: the parameter's dtype). `rounding=
    "stochastic"` rounds every bf16 destination (the parameter, and bf16
    moments) stochastically instead of to nearest: the expectation of the
    stored value is the fp32 result, so updates far below one bf16 ulp still
    accumulate. The random bits are Philox4x32-10 keyed by `rounding_seed`
    with counter (element index, step, parameter ordinal) — a pure function
    of values a checkpoint holds, so resume is bit-exact and no generator
    state is consumed. A parameter's ordinal is its position over all param
    groups at construction; `add_param_group` extends the numbering.

    With both options at their defaults, and for fp32 parameters (nothing
    to round, moments already fp32), the step is the plain `fused_adamw`
    path with the plain state layout.

    `load_state_dict`: torch casts loaded state to the parameter's dtype,
    which would turn fp32 moments into bf16. With `state_dtype` set, the
    moments instead come back in `state_dtype` with their checkpointed
    bits; a bf16-moment checkpoint is upcast (exact). Without `state_dtype`,
    an fp32-moment checkpoint is downcast to the parameter's dtype with
    round-to-nearest (torch's behaviour).
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 state_dtype=None, rounding="nearest", rounding_seed=0):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if state_dtype not in (None, torch.float32):
            raise ValueError(f"state_dtype must be None or torch.float32, got {state_dtype!r}")
        if rounding not in _ROUNDINGS:
            raise ValueError(f"rounding must be one of {_ROUNDINGS}, got {rounding!r}")
        if (isinstance(rounding_seed, bool) or not isinstance(rounding_seed, int)
                or not -(1 << 63) <= rounding_seed < (1 << 63)):
            raise ValueError(f"rounding_seed must be a 64-bit integer, got {rounding_seed!r}")
        self.state_dtype = state_dtype
        self.rounding = rounding
        self.rounding_seed = rounding_seed
        # reference-math dtype of the CPU path for the non-default options
        self._math_dtype = torch.float32
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)

    # -- ordinals -----------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if not hasattr(self, "_ordinals"):  # first call comes from Optimizer.__init__
            self._ordinals = {}
        for p in self.param_groups[-1]["params"]:
            self._ordinals.setdefault(p, len(self._ordinals))

    def ordinal(self, p):
        """The fixed Philox counter word of parameter `p`."""
        return self._ordinals[p]

    def set_ordinals(self, ordinals):
        """Renumber all parameters, in param-group order (a sharded wrapper
        passes global positions so the bits do not depend on the sharding)."""
        params = [p for g in self.param_groups for p in g["params"]]
        ordinals = [int(o) for o in ordinals]
        if len(ordinals) != len(params) or len(set(ordinals)) != len(ordinals):
            raise ValueError("set_ordinals needs one distinct ordinal per parameter")
        if any(not 0 <= o < (1 << 32) for o in ordinals):
            raise ValueError("ordinals must fit in 32 bits")
        self._ordinals = dict(zip(params, ordinals))

    # -- state --------------------------------------------------------------
    def _moment_dtype(self, p):
        if self.state_dtype is not None and p.dtype == torch.bfloat16:
            return self.state_dtype
        return p.dtype

    def _uses_ex(self, p, exp_avg):
        """bf16 parameters with stochastic rounding or fp32 moments take the
        `_ex` path; everything else is the plain step."""
        return p.dtype == torch.bfloat16 and (
            self.rounding == "stochastic" or exp_avg.dtype == torch.float32)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self.state_dtype is None:
            return
        # torch cast the moments to the parameter's dtype; put them back in
        # state_dtype from the checkpointed tensors
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for saved_id, p in zip(saved_ids, params):
            saved = state_dict["state"].get(saved_id)
            if saved is None:
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                if key in saved:
                    self.state[p][key] = saved[key].detach().to(
                        device=p.device, dtype=self._moment_dtype(p), copy=True)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, steps = [], [], [], [], []
            ex = []  # (param, grad, exp_avg, exp_avg_sq, step) on the _ex path
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0)
                    if self._moment_dtype(p) == p.dtype:
                        state["exp_avg"] = torch.zeros_like(p)
                        state["exp_avg_sq"] = torch.zeros_like(p)
                    else:
                        state["exp_avg"] = torch.zeros_like(p, dtype=self._moment_dtype(p))
                        state["exp_avg_sq"] = torch.zeros_like(p, dtype=self._moment_dtype(p))
                state["step"] += 1
                if self._uses_ex(p, state["exp_avg"]):
                    ex.append((p, p.grad, state["exp_avg"], state["exp_avg_sq"],
                               int(state["step"].item())))
                    continue
                params.append(p)
                grads.append(p.grad)
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                steps.append(int(state["step"].item()))

            beta1, beta2 = group["betas"]
            lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
            if ex:
                self._ex_step(ex, beta1, beta2, lr, eps, wd)
            if not params:
                continue

            if params[0].is_cuda and hip.use_hip(params[0], "adamw"):
                # group by identical step count (true except after partial loads)
                by_step = {}
                for i, s in enumerate(steps):
                    by_step.setdefault(s, []).append(i)
                for s, idxs in by_step.items():
                    hip.ext().fused_adamw(
                        [params[i] for i in idxs],
                        [grads[i] for i in idxs],
                        [exp_avgs[i] for i in idxs],
                        [exp_avg_sqs[i] for i in idxs],
                        lr, beta1, beta2, eps, wd, s,
                    )
            else:
                self._foreach_step(params, grads, exp_avgs, exp_avg_sqs, steps,
                                   beta1, beta2, lr, eps, wd)
        return loss

    def _ex_step(self, ex, beta1, beta2, lr, eps, wd):
        """bf16 parameters with fp32 moments and/or stochastic rounding."""
        stochastic = self.rounding == "stochastic"
        if ex[0][0].is_cuda and hip.use_hip(ex[0][0], "adamw"):
            # one launch set per (step, moment dtype): the kernel takes one of each
            groups = {}
            for item in ex:
                groups.setdefault((item[4], item[2].dtype), []).append(item)
            for (s, _), items in groups.items():
                hip.ext().fused_adamw_ex(
                    [it[0] for it in items], [it[1] for it in items],
                    [it[2] for it in items], [it[3] for it in items],
                    lr, beta1, beta2, eps, wd, s,
                    stochastic, self.rounding_seed, [self._ordinals[it[0]] for it in items],
                )
            return
        for p, g, m, v, s in ex:
            new_p, new_m, new_v = adamw_reference_update(
                p, g, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd, step=s,
                math_dtype=self._math_dtype)
            words = None
            if stochastic:
                words = philox.element_words(self.rounding_seed, s, self._ordinals[p],
                                             np.arange(p.numel(), dtype=np.uint64))
            for dst, new, lane in ((m, new_m, philox.LANE_EXP_AVG),
                                   (v, new_v, philox.LANE_EXP_AVG_SQ),
                                   (p, new_p, philox.LANE_PARAM)):
                new = new.to(torch.float32)
                if dst.dtype == torch.bfloat16 and stochastic:
                    new = _round_with_words(new, words, lane)
                dst.copy_(new)  # fp32 unrounded; bf16 copy rounds to nearest

    @staticmethod
    def _foreach_step(params, grads, exp_avgs, exp_avg_sqs, steps, beta1, beta2, lr, eps, wd):
        if wd != 0:
            torch._foreach_mul_(params, 1 - lr * wd)
        torch._foreach_lerp_(exp_avgs, grads, 1 - beta1)
        torch._foreach_mul_(exp_avg_sqs, beta2)
        torch._foreach_addcmul_(exp_avg_sqs, grads, grads, 1 - beta2)
        # per-tensor bias correction (steps can differ after resets/loads)
        for p, m, v, s in zip(params, exp_avgs, exp_avg_sqs, steps):
            bc1 = 1 - beta1 ** s
            bc2 = 1 - beta2 ** s
            denom = (v.float() / bc2).sqrt_().add_(eps)
            p.data.add_(((-lr / bc1) * m.float() / denom).to(p.dtype))


def stochastic_round_bf16(x, seed, step, ordinal, lane):
    """Round the fp32 tensor `x` to bf16 stochastically, element `i` drawing
    the 16 bits of `lane` (0, 1 or 2) from the Philox counter (i, step,
    ordinal) under `seed` — the rule and bits of `AdamW(rounding=
    "stochastic")`. HIP kernel on the GPU, `ops.philox` elsewhere."""
    if x.dtype != torch.float32:
        raise ValueError(f"stochastic_round_bf16 rounds float32 tensors, got {x.dtype}")
    if lane not in (0, 1, 2):
        raise ValueError(f"lane must be 0, 1 or 2, got {lane}")
    if x.is_cuda and hip.use_hip(x, "adamw"):
        return hip.ext().stochastic_round_bf16(x.contiguous(), seed, step, ordinal, lane)
    return philox.stochastic_round_bf16(x, seed, step, ordinal, lane)


def _round_with_words(x, words, lane):
    """Stochastically round fp32 `x` to bf16 with already-drawn Philox words."""
    flat = x.detach().contiguous().view(-1).cpu()
    u = flat.view(torch.int32).numpy().view(np.uint32)
    out = philox.round_bits_to_bf16(u, philox.lane_bits(words, lane))
    out = torch.from_numpy(out.view(np.int16).copy()).view(torch.bfloat16)
    return out.view(x.shape).to(x.device)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=True):
    """Global L2-norm clip over `parameters` grads; returns the total norm."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if len(grads) == 0:
        return torch.tensor(0.0)
    assert norm_type == 2.0, "only L2 clipping is supported"
    device = grads[0].device

    if grads[0].is_cuda and hip.use_hip(grads[0], "clip"):
        total_norm = hip.ext().multi_tensor_l2norm(grads)
    else:
        total_norm = torch.linalg.vector_norm(
            torch.stack([torch.linalg.vector_norm(g.detach().float()) for g in grads])
        )

    if error_if_nonfinite and (torch.isnan(total_norm) or torch.isinf(total_norm)):
        raise RuntimeError(
            f"The total norm of order {norm_type} for gradients from `parameters` "
            f"is non-finite, so it cannot be clipped."
        )
    clip_coef = max_norm / (total_norm + 1e-6)
    if clip_coef < 1:
        if grads[0].is_cuda and hip.use_hip(grads[0], "clip"):
            hip.ext().multi_tensor_scale_(grads, float(clip_coef))
        else:
            torch._foreach_mul_(grads, clip_coef.to(device))
    return total_norm
