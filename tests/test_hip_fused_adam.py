"""ls2fm.optim.FusedAdam (csrc/adam.hip through the C ABI) against torch.optim.Adam on the GPU: same trajectory over
several steps incl. an ExponentialLR schedule, weight decay, ragged sizes (non-multiples of 4, unaligned views) and a
state_dict round trip."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(1 << 20) + 3, (64, 35), (64,), (17, 64), (1,), (3, 64), (5,)]
    ps = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    big = torch.randn(1000, generator=g).to(DEV)
    ps.append(big[1:998])                       # a 4-byte aligned, not 16-byte aligned contiguous view
    return ps


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_follows_torch_adam(wd):
    from ls2fm.optim import FusedAdam
    a = [torch.nn.Parameter(p.clone()) for p in _params(1)]
    b = [torch.nn.Parameter(p.clone()) for p in _params(1)]
    oa = torch.optim.Adam(a, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=wd)
    ob = FusedAdam(b, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=wd)
    sa = torch.optim.lr_scheduler.ExponentialLR(oa, 0.9)
    sb = torch.optim.lr_scheduler.ExponentialLR(ob, 0.9)
    g = torch.Generator().manual_seed(7)
    for it in range(6):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g).to(DEV) * (10.0 ** (it - 3))
            pa.grad = gr.clone(); pb.grad = gr.clone()
        if it == 2:
            b[4].grad = None; a[4].grad = None           # a parameter without gradient keeps its own step count
        oa.step(); ob.step(); sa.step(); sb.step()
        if it == 3:                                      # state_dict round trip
            ob2 = FusedAdam(b, lr=1.0)
            ob2.load_state_dict(ob.state_dict())
            ob = ob2
            sb.optimizer = ob                            # the scheduler keeps driving the re-created optimizer's groups
    for pa, pb in zip(a, b):
        assert rel_err(pb.detach().cpu(), pa.detach().cpu()) < 2e-6
    for pa, pb in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert rel_err(ob.state[pb][k].cpu(), oa.state[pa][k].cpu()) < 2e-6, k
        assert int(ob.state[pb]["step"]) == int(oa.state[pa]["step"])


def test_fused_adam_refuses_cpu_tensors():
    from ls2fm.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError):
        FusedAdam([p]).step()


# ------------------------------------------------------------------------------------------------------------------------------
# Per element against the float64 Adam of tests/adam_reference.py.  Re-synchronised: before every step the kernel's own fp32
# state (p, exp_avg, exp_avg_sq, step) is read back, the reference takes ONE step from it in float64, and the kernel's result
# is held to that element by element, so no trajectory drift enters the bars:
#   exp_avg     within M_ULP fp32 ulps of max(|m_ref|, the terms torch's lerp forms it from: adam_reference.lerp_scale); the
#               fp32 lerp rounds g', g' - m, the product and the sum: at most ~2.6 of these ulps (2.45 seen)
#   exp_avg_sq  within V_ULP fp32 ulps of |v_ref| (subnormal spacing included; both terms are >= 0, nothing cancels); four
#               roundings plus g''s own, which the square doubles (3.14 seen).  Before ABI 11 (beta2 rounded to fp32 before
#               1 - beta2) this was ~150 ulps at beta2 = 0.999
#   p_new - p   within DP_REL |dp_ref| + DP_ULP ulp(p_new), dp_ref formed from the kernel's new moments of this step (their
#               own errors are held above)
#   an entry whose gradient is always 0 (no weight decay) keeps p, and exp_avg = exp_avg_sq = 0, exactly; NaN and inf where
#   the reference rounded to fp32 has them
import ctypes  # noqa: E402

import numpy as np  # noqa: E402

import adam_reference as ar  # noqa: E402

M_ULP, V_ULP, DP_REL, DP_ULP = 3.0, 4.0, 1e-6, 1.0
BETAS = [(0.9, 0.999), (0.9, 0.99), (0.3, 0.5), (0.0, 0.0)]
SIZES = [1, 2, 3, 4, 5, 6, 2047, 2048, 2049, (1 << 20) + 2, (1 << 20) + 3]
_WORST = {}


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _grad_values(n, seed, shift):
    """the gradient of one tensor at one step: entry k is, by (k + shift) % 8, exactly 0 (at every step), +-1e-30 (g^2 below
    fp32's range), 1e-20 (g^2 subnormal), +-1e20 (g^2 above fp32's range), or mixed-sign N(0, 1) x 10^U(-4, 2)"""
    r = np.random.default_rng(seed)
    g = r.standard_normal(n) * 10.0 ** r.uniform(-4, 2, n)
    kind = (np.arange(n) + shift) % 8
    sign = np.where(r.standard_normal(n) < 0, -1.0, 1.0)
    g[kind == 0] = 0.0
    g[kind == 1] = 1e-30 * sign[kind == 1]
    g[kind == 2] = 1e-20
    g[kind == 3] = 1e20 * sign[kind == 3]
    return torch.from_numpy(g.astype(np.float32))


def _zero_grad_mask(n, shift):
    return (np.arange(n) + shift) % 8 == 0


def _offset(n, offset, gen):
    """an fp32 tensor of n values whose data starts `offset` floats into its own allocation (offset 1: a 4-byte aligned view)"""
    base = torch.randn(n + offset, generator=gen).to(DEV)
    return base[offset:]


def _matrix_params(seed):
    """40 tensors: every size of SIZES 16-byte aligned and as a 4-byte offset view, plus 18 small ones -- more than the 32
    tensors of one adam_kernel launch"""
    gen = torch.Generator().manual_seed(seed)
    ts = []
    for n in SIZES:
        ts += [_offset(n, 0, gen), _offset(n, 1, gen)]
    for n in torch.randint(1, 300, (18,), generator=gen).tolist():
        ts.append(_offset(n, 0, gen))
    ps = [torch.nn.Parameter(t) for t in ts]
    assert len(ps) == 40 and {p.data_ptr() % 16 for p in ps[:22]} == {0, 4}
    return ps


def _set_grads(params, seed):
    for i, p in enumerate(params):
        g = _grad_values(p.numel(), seed * 1000 + i, i).to(DEV)
        if p.data_ptr() % 16:                   # an unaligned parameter gets an unaligned gradient as well
            buf = torch.empty(p.numel() + 1, device=DEV)
            buf[1:].copy_(g)
            g = buf[1:]
        p.grad = g


def _snapshot(opt):
    """the state every parameter with a gradient takes its next step from: (p, group, p0, g, m0, v0, step, lr)"""
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            if p.grad is None:
                continue
            st = opt.state.get(p) or {}
            zero = np.zeros(p.numel())
            m0 = _np(st["exp_avg"]).reshape(-1) if st else zero
            v0 = _np(st["exp_avg_sq"]).reshape(-1) if st else zero
            out.append((p, group, _np(p).reshape(-1), _np(p.grad).reshape(-1), m0, v0, int(st.get("step", 0)) + 1,
                        float(group["lr"])))
    return out


def _check(opt, snap, what, lr=None, zero_shift=None):
    """hold every parameter of `snap` (after opt.step()) to the float64 step from its snapshot"""
    worst = _WORST.setdefault(what, dict(m=0.0, v=0.0, dp=0.0))
    for i, (p, group, p0, g, m0, v0, step, lr_host) in enumerate(snap):
        st = opt.state[p]
        assert int(st["step"]) == step
        b1, b2 = group["betas"]
        hyper = dict(lr=lr_host if lr is None else lr[i], beta1=b1, beta2=b2, eps=group["eps"], step=step)
        wd = group["weight_decay"]
        _, m_ref, v_ref = ar.adam_step(p0, g, m0, v0, weight_decay=wd, **hyper)
        p1, m1, v1 = _np(p).reshape(-1), _np(st["exp_avg"]).reshape(-1), _np(st["exp_avg_sq"]).reshape(-1)
        em = ar.ulp_error(m1, m_ref, ar.lerp_scale(m0, g, b1, wd, p0))
        ev = ar.ulp_error(v1, v_ref)
        d_ref = -ar.adam_update(m1, v1, **hyper)
        with np.errstate(all="ignore"):
            d_got = p1 - p0
            edp = np.abs(d_got - d_ref) / (DP_REL * np.abs(d_ref) + DP_ULP * ar.ulp32(p1))
            ref_nan = np.isnan(p0 + d_ref)
        edp = np.where(ref_nan, np.where(np.isnan(p1), 0.0, np.inf), np.nan_to_num(edp, nan=np.inf))
        for k, e, bar in (("m", em, M_ULP), ("v", ev, V_ULP), ("dp", edp, 1.0)):
            w = float(e.max()) if e.size else 0.0
            worst[k] = max(worst[k], w)
            if w > bar:
                j = int(np.argmax(e))
                raise AssertionError(f"{what}: tensor {i} (numel {p.numel()}, step {step}) {k} error {w:.3g} > {bar} at {j}: "
                                     f"p0 {p0[j]!r} g {g[j]!r} m0 {m0[j]!r} v0 {v0[j]!r} -> p {p1[j]!r} m {m1[j]!r} "
                                     f"v {v1[j]!r}; ref m {m_ref[j]!r} v {v_ref[j]!r} dp {d_ref[j]!r}")
        if zero_shift is not None and wd == 0:
            z = _zero_grad_mask(p.numel(), zero_shift[i]) & (m0 == 0) & (v0 == 0)
            assert (p1[z] == p0[z]).all() and (m1[z] == 0).all() and (v1[z] == 0).all(), f"{what}: tensor {i}: zero moved"
    print(f"[adam worst] {what}: {worst}")


@pytest.mark.parametrize("betas", BETAS, ids=lambda b: f"b{b[0]}-{b[1]}")
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=lambda w: f"wd{w}")
@pytest.mark.parametrize("eps", [1e-8, 1e-15], ids=lambda e: f"eps{e}")
def test_fused_adam_matches_fp64_adam_per_element(betas, wd, eps):
    """40 tensors (aligned and 4-byte offset, numel 1 .. 2^20 + 3) through FusedAdam's host-step path: steps 1, 2, 1000 and a
    resume at step 10^5 through load_state_dict, each held per element to the float64 step from the kernel's own state"""
    from ls2fm.optim import FusedAdam
    ps = _matrix_params(11)
    shifts = list(range(len(ps)))
    hyper = dict(lr=1e-2, betas=betas, eps=eps, weight_decay=wd)
    opt = FusedAdam(ps, **hyper)
    what = f"host {betas} wd={wd} eps={eps}"
    for it in range(4):
        if it == 2:                                 # jump the step count: bias corrections near 1
            for p in ps:
                opt.state[p]["step"] = 999
        if it == 3:                                 # resume from a checkpoint at step 10^5 in a new optimizer
            sd = opt.state_dict()
            for st in sd["state"].values():
                st["step"] = 10 ** 5 - 1
            opt = FusedAdam(ps, lr=0.5)
            opt.load_state_dict(sd)
            assert opt.param_groups[0]["betas"] == betas and opt.param_groups[0]["lr"] == 1e-2
        _set_grads(ps, it)
        snap = _snapshot(opt)
        assert {s[6] for s in snap} == {(1, 2, 1000, 10 ** 5)[it]}
        opt.step()
        _check(opt, snap, what, zero_shift=shifts)


def test_fused_adam_nan_where_the_reference_is_nan():
    """eps = 0 and a zero gradient on zero moments: 0 / 0 -- NaN in the reference, NaN from the kernel (no silent clamp)"""
    from ls2fm.optim import FusedAdam
    p = torch.nn.Parameter(torch.ones(4099, device=DEV))
    g = torch.randn(4099, device=DEV)
    g[::3] = 0
    p.grad = g
    opt = FusedAdam([p], lr=1e-2, eps=0.0)
    snap = _snapshot(opt)
    opt.step()
    _check(opt, snap, "eps=0")
    assert torch.isnan(p[::3]).all() and not torch.isnan(p[1::3]).any()


def test_scheduled_adam_matches_fp64_adam_and_exponential_lr():
    """FusedAdam(scheduled_gamma=0.99), the form RenderStage uses: 200 steps of 20 parameter groups (more than the 16 schedules
    of one adam_advance_kernel / adam_decay_kernel launch), some groups idle on some steps -- 18 of them at once on one step.
    Every step is held per element to the float64 step at the learning rate of the ExponentialLR recurrence, and the device
    schedule of every group to the host's double recurrence: step and lr exactly, its step_size / bc2_sqrt floats equal to
    (float)(lr / bc1) and (float)sqrt(bc2) formed in double."""
    from ls2fm.optim import FusedAdam
    gamma, betas, n_groups, steps = 0.99, (0.9, 0.999), 20, 200
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 2, 3, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 2047, 2048, 2049, 4098, 4099, 8190, 8193]
    ps = [torch.nn.Parameter(_offset(n, i % 2, gen)) for i, n in enumerate(sizes)]
    lr0 = [1e-3 * (1 + gi) for gi in range(n_groups)]
    opt = FusedAdam([dict(params=[p], lr=lr) for p, lr in zip(ps, lr0)], betas=betas, eps=1e-15, scheduled_gamma=gamma)
    lrs = [ar.exponential_lr(lr, gamma, steps + 1) for lr in lr0]
    taken = [0] * n_groups
    for t in range(steps):
        idle = {gi for gi in range(n_groups) if (t + gi) % 7 == 3} if t != 100 else set(range(18))
        for gi, p in enumerate(ps):
            p.grad = None
        _set_grads([p for gi, p in enumerate(ps) if gi not in idle], t)
        snap = _snapshot(opt)
        active = [gi for gi in range(n_groups) if gi not in idle]
        opt.step()
        _check(opt, snap, "scheduled", lr=[lrs[gi][t] for gi in active])
        sched = {gi: opt._sched[gi].cpu() for gi in opt._sched}
        for gi in range(n_groups):
            taken[gi] += gi not in idle
            assert opt.param_groups[gi]["lr"] == lrs[gi][t + 1]
            s = sched[gi]
            assert float(s[0]) == taken[gi] and float(s[1]) == lrs[gi][t + 1] and float(s[2]) == gamma
            if gi in idle:
                continue
            step_size, bc2_sqrt = ar.step_scalars(lrs[gi][t], betas[0], betas[1], taken[gi])
            packed = s[3:].numpy().view(np.float32)
            assert packed[0] == np.float32(step_size) and packed[1] == np.float32(bc2_sqrt), (gi, t, packed)


def _table_floats_l16_t19():
    from ls2fm.hashgrid import build_grid_desc, n_table_floats, per_level_scale_from_bounds
    return n_table_floats(build_grid_desc(16, 2, 19, 16, per_level_scale_from_bounds(-1.0, 1.0, 16, 16)))


def _mirrored_tables(n, offset, seed):
    """two table Parameters wired to one entry-interleaved copy as ls2fm.fused does for a dual field; the copy starts as NaN in
    the halves the optimizer must write"""
    from ls2fm.fused import TableMirror
    gen = torch.Generator().manual_seed(seed)
    a, b = (torch.nn.Parameter(_offset(n, offset, gen)) for _ in range(2))
    rec = TableMirror()
    rec.table = torch.full((2 * n,), float("nan"), device=DEV)
    rec.ptrs = [a.data_ptr(), b.data_ptr()]
    a._ls2fm_mirror, b._ls2fm_mirror = (rec, 0), (rec, 1)
    return a, b, rec


def _interleave(a, b):
    return torch.stack([a.detach().view(-1, 2), b.detach().view(-1, 2)], dim=1).reshape(-1)


@pytest.mark.parametrize("case", ["full_l16_t19", "tail_2", "tail_6", "tail_4098", "unaligned", "lone"])
@pytest.mark.parametrize("gamma", [None, 0.9], ids=["host", "scheduled"])
def test_mirrored_tables_match_fp64_adam_and_their_interleave(case, gamma):
    """the two hash tables of a dual field with their entry-interleaved copy: the paired job at the shipped L16/T19 table size,
    paired tails of numel = 2 (mod 4), a pair with a 4-byte offset (single mirrored jobs) and a lone mirrored table (the other
    has no gradient).  Values are held to the float64 step; the copy equals the interleave of the Parameters bit for bit."""
    from ls2fm.optim import FusedAdam
    n = dict(full_l16_t19=_table_floats_l16_t19(), tail_2=2, tail_6=6, tail_4098=4098, unaligned=4098, lone=4098)[case]
    a, b, rec = _mirrored_tables(n, 1 if case == "unaligned" else 0, 21)
    if case == "lone":
        rec.table.view(-1, 2, 2)[:, 1].copy_(b.detach().view(-1, 2))         # b's half is not rewritten: keep its values
    opt = FusedAdam([dict(params=[a], lr=1e-2), dict(params=[b], lr=3e-3)], eps=1e-15, scheduled_gamma=gamma)
    for it in range(2):
        _set_grads([a, b], it + 7)
        if case == "lone":
            b.grad = None
        snap = _snapshot(opt)
        opt.step()
        _check(opt, snap, f"mirrored {case}")
        assert torch.equal(rec.table.view(torch.int32), _interleave(a, b).view(torch.int32)), f"{case}: copy != interleave"


def _abi_call(lib, ts, mirrors=None, lrs=None, scheds=None, betas=(0.9, 0.999), eps=1e-8, wd=0.0, step=1, n=None, numel=None):
    """ls2fm_adam_step_multi on tensors ts = [(p, g, m, v)]"""
    from ls2fm import _lib
    k = len(ts) if n is None else n
    ptrs = lambda i: (ctypes.c_void_p * k)(*[t[i].data_ptr() for t in ts])           # noqa: E731
    return lib.ls2fm_adam_step_multi(
        k, ptrs(0), ptrs(1), ptrs(2), ptrs(3), (ctypes.c_int64 * k)(*(numel or [t[0].numel() for t in ts])),
        None if mirrors is None else (ctypes.c_void_p * k)(*mirrors),
        None if lrs is None else (ctypes.c_double * k)(*lrs),
        None if scheds is None else (ctypes.c_void_p * k)(*[None if s is None else s.data_ptr() for s in scheds]),
        betas[0], betas[1], eps, wd, step, _lib.stream_ptr())


def _state(n, seed):
    """(p, g, m, v) mid-run: moments from earlier steps, a mixed gradient"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 1e-2
    v = torch.rand(n, generator=gen) * 1e-4
    return [p.to(DEV), _grad_values(n, seed, 0).to(DEV), m.to(DEV), v.to(DEV)]


def _clone(ts):
    return [[x.clone() for x in t] for t in ts]


def _bits(ts):
    return [torch.cat([x.view(torch.int32) for x in t]) for t in ts]


def test_every_launch_form_gives_the_same_bits():
    """the same inputs through the paired job, two single mirrored jobs, the unmirrored job, one launch for 40 tensors against
    one launch per tensor, and the host step against a device schedule: bit-identical p, exp_avg, exp_avg_sq (every form runs
    the same adam_one), and every copy holds the parameters' bits"""
    from ls2fm import _lib
    lib = _lib.load()
    n = (1 << 16) + 2                                       # a paired tail as well
    base = [_state(n, 31), _state(n, 32)]
    outs = {}
    # paired job: the two halves of one interleaved copy
    ts = _clone(base)
    mir = torch.full((2 * n,), float("nan"), device=DEV)
    assert _abi_call(lib, ts, mirrors=[mir.data_ptr(), mir.data_ptr() + 8], lrs=[1e-2, 3e-3], step=3) == 0
    assert torch.equal(mir.view(torch.int32), _interleave(ts[0][0], ts[1][0]).view(torch.int32))
    outs["pair"] = ts
    # two single mirrored jobs: each table has a copy of its own (not the two halves of one)
    ts = _clone(base)
    mirs = [torch.full((2 * n,), float("nan"), device=DEV) for _ in range(2)]
    assert _abi_call(lib, ts, mirrors=[mm.data_ptr() for mm in mirs], lrs=[1e-2, 3e-3], step=3) == 0
    for t, mm in zip(ts, mirs):
        assert torch.equal(mm.view(-1, 2, 2)[:, 0].reshape(-1).view(torch.int32), t[0].view(torch.int32))
    outs["single mirrored"] = ts
    ts = _clone(base)
    assert _abi_call(lib, ts, lrs=[1e-2, 3e-3], step=3) == 0
    outs["unmirrored"] = ts
    ts = _clone(base)
    for t, lr in zip(ts, [1e-2, 3e-3]):
        assert _abi_call(lib, [t], lrs=[lr], step=3) == 0
    outs["one call per tensor"] = ts
    # device schedules at step 2 -> the update runs at step 3 with lr = 1e-2 / 3e-3 (gamma applies after)
    ts = _clone(base)
    scheds = [torch.tensor([2.0, lr, 0.5, 0.0], device=DEV, dtype=torch.float64) for lr in (1e-2, 3e-3)]
    mir = torch.full((2 * n,), float("nan"), device=DEV)
    assert _abi_call(lib, ts, mirrors=[mir.data_ptr(), mir.data_ptr() + 8], scheds=scheds, step=0) == 0
    assert torch.equal(mir.view(torch.int32), _interleave(ts[0][0], ts[1][0]).view(torch.int32))
    outs["scheduled pair"] = ts
    ref = _bits(outs.pop("pair"))
    for k, ts in outs.items():
        assert all(torch.equal(x, y) for x, y in zip(_bits(ts), ref)), k
    # 40 tensors (aligned and offset) in one call -- two adam_kernel launches -- against one call per tensor
    gen = torch.Generator().manual_seed(33)
    many = []
    for i, sz in enumerate(SIZES[:9] * 4 + [4099] * 4):
        t = _state(sz + 1, 100 + i)
        many.append([x[i % 2:i % 2 + sz] for x in t])
    lrs = [1e-3 * (i + 1) for i in range(len(many))]
    one = _clone(many)
    assert _abi_call(lib, one, lrs=lrs, betas=(0.3, 0.5), wd=1e-2, step=2) == 0
    each = _clone(many)
    for t, lr in zip(each, lrs):
        assert _abi_call(lib, [t], lrs=[lr], betas=(0.3, 0.5), wd=1e-2, step=2) == 0
    assert all(torch.equal(x, y) for x, y in zip(_bits(one), _bits(each)))
    assert not torch.equal(one[0][0], many[0][0])


def test_adam_step_multi_refuses_bad_arguments_without_side_effects():
    """-1 (invalid argument) and nothing launched: more than 4096 tensors, an odd numel with a mirror, a mirror not 8-byte
    aligned, a beta outside [0, 1), step 0 without a schedule"""
    from ls2fm import _lib
    lib = _lib.load()
    t = _state(8, 41)
    t2 = _state(8, 42)
    sched = torch.tensor([4.0, 1e-2, 0.5, 0.0], device=DEV, dtype=torch.float64)
    before = ([x.clone() for x in t], [x.clone() for x in t2], sched.clone())
    mir = torch.zeros(64, device=DEV)
    bad = [
        dict(ts=[t] * 4097, lrs=[1e-2] * 4097),
        dict(ts=[t2, t], mirrors=[mir.data_ptr(), mir.data_ptr() + 32], scheds=[sched, sched], step=0, numel=[8, 7]),
        dict(ts=[t2, t], mirrors=[None, mir.data_ptr() + 4], scheds=[sched, sched], step=0),
        dict(ts=[t2, t], scheds=[sched, sched], step=0, betas=(1.0, 0.999)),
        dict(ts=[t2, t], scheds=[sched, sched], step=0, betas=(0.9, 1.0)),
        dict(ts=[t2, t], scheds=[sched, sched], step=0, betas=(-1e-3, 0.999)),
        dict(ts=[t2, t], scheds=[sched, sched], step=0, betas=(0.9, float("nan"))),
        dict(ts=[t2, t], lrs=[1e-2, 1e-2], step=0),
        dict(ts=[t2, t], lrs=[1e-2, 1e-2], scheds=[sched, None], step=0),
    ]
    for i, kw in enumerate(bad):
        assert _abi_call(lib, **kw) == -1, i
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(t + t2 + [sched], before[0] + before[1] + [before[2]]))
    assert _abi_call(lib, [t2, t], lrs=[1e-2, 1e-2], step=1) == 0 and not torch.equal(t[0], before[0][0])
