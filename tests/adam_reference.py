"""Plain float64 Adam: the arbiter the FusedAdam tests hold csrc/adam.hip to.

One step of torch.optim.Adam (amsgrad = False, maximize = False) evaluated in float64 from (normally fp32) state, with torch's
scalar semantics: the hyper-parameters are Python doubles, `1 - beta`, `beta ** step`, `lr / bc1` and `sqrt(bc2)` are formed in
double, and every scalar torch hands to an fp32 tensor op (weight decay, the lerp weight 1 - beta1, beta2, 1 - beta2, eps,
lr / bc1, sqrt(bc2)) is rounded to fp32 once, as torch's fp32 kernels do; the element arithmetic is exact.  The first moment is
torch's `lerp` (both branches), weight decay is added to the gradient.  `exponential_lr` is the
ExponentialLR recurrence (`lr *= gamma` in double, once per scheduler step).  tests/test_adam_reference.py pins both against
torch on the CPU.
"""
from __future__ import annotations

import math

import numpy as np


def adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step):
    """-> (p, exp_avg, exp_avg_sq) after Adam step number `step` (1-based), all float64 arrays"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if weight_decay != 0:
            g = g + _f32(weight_decay) * p
        w = _f32(1.0 - beta1)
        m = m + w * (g - m) if w < 0.5 else g - (g - m) * (1.0 - w)          # torch.lerp(m, g, w)
        v = v * _f32(beta2) + _f32(1.0 - beta2) * g * g
        return p - adam_update(m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step), m, v


def adam_update(m, v, *, lr, beta1, beta2, eps, step):
    """the amount Adam step `step` subtracts from the parameter, given that step's NEW moments (float64)"""
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    step_size, bc2_sqrt = step_scalars(lr, beta1, beta2, step)
    with np.errstate(all="ignore"):
        return _f32(step_size) * (m / (np.sqrt(v) / _f32(bc2_sqrt) + _f32(eps)))


def _f32(x):
    """a double scalar as an fp32 tensor op receives it"""
    return float(np.float32(x))


def step_scalars(lr, beta1, beta2, step):
    """(lr / (1 - beta1^step), sqrt(1 - beta2^step)) in double, as torch's single-tensor Adam forms them"""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return lr / bc1, math.sqrt(bc2)


def exponential_lr(lr, gamma, n):
    """the learning rates of n consecutive steps under ExponentialLR(gamma) starting at `lr`: [lr, lr*g, (lr*g)*g, ...]"""
    out = []
    for _ in range(n):
        out.append(lr)
        lr = lr * gamma
    return out


def ulp32(x):
    """the fp32 unit in the last place at |x| (x rounded to fp32 first; subnormals and zero: 2^-149)"""
    with np.errstate(over="ignore"):
        a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return np.spacing(np.where(np.isfinite(a), a, np.float32(np.finfo(np.float32).max))).astype(np.float64)


def ulp_error(got, ref, scale=None):
    """per element |got - ref| in fp32 ulps of max(|ref|, scale).  Non-finite entries count as exact when `got` equals the
    reference rounded to fp32 (same infinity, or both NaN) and as infinitely wrong otherwise."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(over="ignore"):
        ref32 = ref.astype(np.float32).astype(np.float64)
    mag = np.abs(ref) if scale is None else np.maximum(np.abs(ref), np.asarray(scale, dtype=np.float64))
    with np.errstate(all="ignore"):
        err = np.abs(got - ref) / ulp32(mag)
    special = ~np.isfinite(ref32) | ~np.isfinite(got)
    same = (got == ref32) | (np.isnan(got) & np.isnan(ref32))
    return np.where(special, np.where(same, 0.0, np.inf), err)


def lerp_scale(m, g, beta1, weight_decay=0.0, p=None):
    """the magnitudes torch's lerp forms the new first moment from: m and w (g' - m) when w = 1 - beta1 < 0.5, else g' and
    (1 - w)(g' - m).  An fp32 lerp rounds at the size of these terms, so where they cancel the result's own ulp is no measure
    of the arithmetic (torch's lerp included)"""
    m, g = np.asarray(m, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if weight_decay != 0:
        g = g + weight_decay * np.asarray(p, dtype=np.float64)
    w = 1.0 - beta1
    if w < 0.5:
        return np.maximum(np.abs(m), np.abs(w * (g - m)))
    return np.maximum(np.abs(g), np.abs((1.0 - w) * (g - m)))
