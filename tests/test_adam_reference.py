"""The float64 Adam of tests/adam_reference.py against torch.optim.Adam(foreach=False) + ExponentialLR on the CPU, so the arbiter
of the FusedAdam tests is itself checked.  Re-synchronised: every step starts the reference from torch's own fp32 state, and
torch's result is held to it element by element (torch rounds in fp32, the reference does not)."""
import numpy as np
import pytest
import torch

import adam_reference as ar

STEPS = 50


def _grads(n, seed):
    """mixed-sign gradients over many magnitudes, plus zeros and the extremes (g^2 below fp32's range, g^2 above it)"""
    r = np.random.default_rng(seed)
    g = r.standard_normal(n) * 10.0 ** r.uniform(-4, 2, n)
    kind = np.arange(n) % 8
    g[kind == 0] = 0.0
    g[kind == 1] = 1e-30 * np.sign(r.standard_normal(int((kind == 1).sum())))
    g[kind == 2] = 1e-20
    g[kind == 3] = -1e20
    return torch.from_numpy(g.astype(np.float32))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.99), (0.3, 0.5)])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_reference_matches_torch_adam_per_element(betas, wd):
    n, lr, gamma, eps = 4099, 1e-2, 0.97, 1e-8
    gen = torch.Generator().manual_seed(3)
    p = torch.nn.Parameter(torch.randn(n, generator=gen))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma)
    lrs = ar.exponential_lr(lr, gamma, STEPS + 1)
    worst = dict(m=0.0, v=0.0, dp=0.0)
    for t in range(1, STEPS + 1):
        assert opt.param_groups[0]["lr"] == lrs[t - 1]              # the recurrence, bit for bit in double
        p0 = p.detach().numpy().copy()
        st = opt.state[p]
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros(n, np.float32)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(n, np.float32)
        g = _grads(n, t)
        p.grad = g.clone()
        # torch rounds wd * p before adding it (two roundings), so where g ~ -wd p its fp32 g' carries an error of the size of
        # wd p: the reference starts from torch's g', which is itself held to g + wd p within the rounding of its terms
        gd = g.add(p.detach(), alpha=wd).numpy().astype(np.float64) if wd else g.numpy().astype(np.float64)
        exact = g.numpy().astype(np.float64) + wd * p0.astype(np.float64)
        assert (np.abs(gd - exact) <= 1.5 * ar.ulp32(np.maximum(np.abs(g.numpy()), np.abs(wd * p0)))).all()
        opt.step()
        sched.step()
        hyper = dict(lr=lrs[t - 1], beta1=betas[0], beta2=betas[1], eps=eps, step=t)
        _, m_ref, v_ref = ar.adam_step(p0, gd, m0, v0, weight_decay=0.0, **hyper)
        m1, v1, p1 = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), p.detach().numpy()
        em = ar.ulp_error(m1, m_ref, ar.lerp_scale(m0, gd, betas[0]))
        ev = ar.ulp_error(v1, v_ref)
        # the update, from torch's own new moments (their errors are held above): |dp - dp_ref| <= 1e-6 |dp_ref| + 1 ulp(p)
        d_ref = -ar.adam_update(m1, v1, **hyper)
        d_got = p1.astype(np.float64) - p0
        with np.errstate(all="ignore"):
            edp = np.abs(d_got - d_ref) / (1e-6 * np.abs(d_ref) + ar.ulp32(p1))
        edp = np.where(np.isnan(d_ref) & np.isnan(d_got), 0.0, edp)
        for k, e in (("m", em), ("v", ev), ("dp", edp)):
            worst[k] = max(worst[k], float(np.nan_to_num(e, nan=np.inf).max()))
    assert worst["m"] <= 2 and worst["v"] <= 3 and worst["dp"] <= 1, worst


def test_exponential_lr_and_step_scalars_follow_python():
    assert ar.exponential_lr(0.5, 0.5, 3) == [0.5, 0.25, 0.125]
    step_size, bc2_sqrt = ar.step_scalars(1e-3, 0.9, 0.999, 1)
    assert step_size == 1e-3 / (1 - 0.9) and bc2_sqrt == (1 - 0.999) ** 0.5
    assert ar.step_scalars(1e-3, 0.9, 0.999, 10 ** 5) == (1e-3 / (1 - 0.9 ** 10 ** 5), (1 - 0.999 ** 10 ** 5) ** 0.5)


def test_ulp_error_counts_subnormals_and_specials():
    tiny = np.float32(2.0 ** -149)
    assert ar.ulp32(0.0) == 2.0 ** -149 and ar.ulp32(1.0) == 2.0 ** -23
    assert ar.ulp_error(3 * tiny, 1 * tiny) == 2                   # subnormal spacing, not relative error
    assert ar.ulp_error(np.inf, 1e40) == 0 and ar.ulp_error(np.nan, np.nan) == 0
    assert ar.ulp_error(np.float32(3e38), 1e40) == np.inf and ar.ulp_error(1.0, np.nan) == np.inf
