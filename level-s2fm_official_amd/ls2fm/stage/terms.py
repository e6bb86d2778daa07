"""The loss terms a stage loop forms OUTSIDE the render, each as one fused autograd node each way (include/ls2fm.h): in a captured
iteration every torch kernel of the lines they replace, and of their autograd mirror, is a graph node of >= 4.6 us whatever its
size.  The torch-op forms of the same terms stay beside their callers in `loops.py` (fp64 / CPU tensors, and the tests' references).
"""
from __future__ import annotations

import ctypes

import torch

from .. import _lib


def _f32(t, *shape):
    """a kernel operand: detached, (reshaped,) float32, contiguous -- no kernel when `t` already is all of that"""
    t = t.detach()
    return (t.reshape(*shape) if shape else t).float().contiguous()


class _TracingTerm(torch.autograd.Function):
    """the tracing-consistency sums of TracingConsistency.__call__ as one fused node (include/ls2fm.h: ls2fm_tracing_term_fwd /
    _bwd): (tracing_loss, sdf_surf) from the traced depths d [.., n] and, optionally, the last SDF values; differentiable w.r.t.
    both"""

    @staticmethod
    def forward(ctx, center, ray, d, target, live, sdf_last):
        lib = _lib.load()
        n = live.numel()
        c, r, t = _f32(center, -1, 3), _f32(ray, -1, 3), _f32(target)
        dd, lv = _f32(d, -1), _f32(live)
        sl = None if sdf_last is None else _f32(sdf_last, -1)
        out = torch.empty(3, device=d.device)
        _lib.check(lib.ls2fm_tracing_term_fwd(_lib.ptr(c), _lib.ptr(r), _lib.ptr(dd), _lib.ptr(t), _lib.ptr(lv), _lib.ptr(sl), n,
                                              _lib.ptr(out), _lib.stream_ptr()), "ls2fm_tracing_term_fwd")
        ctx.save_for_backward(c, r, dd, t, lv, out, *([] if sl is None else [sl]))
        ctx.shapes = (d.shape, None if sdf_last is None else sdf_last.shape)
        # the two terms as tensors of their own (views of `out` made HERE, outside autograd): indexing a stacked result afterwards
        # costs a zero fill + a copy per term in the backward -- graph nodes of a captured iteration
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_tl, g_sd):
        lib = _lib.load()
        c, r, dd, t, lv, out = ctx.saved_tensors[:6]
        sl = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        g_tl = None if g_tl is None else _f32(g_tl, 1)
        g_sd = None if g_sd is None else _f32(g_sd, 1)
        d_d = torch.empty_like(dd)
        d_s = None if sl is None else torch.empty_like(sl)
        _lib.check(lib.ls2fm_tracing_term_bwd(_lib.ptr(c), _lib.ptr(r), _lib.ptr(dd), _lib.ptr(t), _lib.ptr(lv), _lib.ptr(sl), lv.numel(),
                                              _lib.ptr(out), _lib.ptr(g_tl), _lib.ptr(g_sd), _lib.ptr(d_d), _lib.ptr(d_s), _lib.stream_ptr()),
                   "ls2fm_tracing_term_bwd")
        return None, None, d_d.view(ctx.shapes[0]), None, None, (None if d_s is None else d_s.view(ctx.shapes[1]))


class _WeightedPair(torch.autograd.Function):
    """wa a + wb b of two device scalars as one node each way (ls2fm_weighted_pair_fwd / _bwd).  The two gradients are the halves
    of ONE two-float buffer: a producer that returned `a` and `b` as the halves of one buffer too (_MatchTerm) gets its upstream
    back contiguous and needs no stacking kernel"""

    @staticmethod
    def forward(ctx, a, b, wa, wb):
        lib = _lib.load()
        out = torch.empty((), device=a.device)
        _lib.check(lib.ls2fm_weighted_pair_fwd(_lib.ptr(a.detach()), _lib.ptr(b.detach()), float(wa), float(wb), _lib.ptr(out),
                                               _lib.stream_ptr()), "ls2fm_weighted_pair_fwd")
        ctx.w = (float(wa), float(wb), a.shape, b.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        wa, wb, sa, sb = ctx.w
        d2 = torch.empty(2, device=g.device)
        _lib.check(lib.ls2fm_weighted_pair_bwd(_lib.ptr(_f32(g, 1)), wa, wb, _lib.ptr(d2), _lib.stream_ptr()), "ls2fm_weighted_pair_bwd")
        return d2[0].view(sa), d2[1].view(sb), None, None


def _weighted_pair(a, b, wa, wb):
    if a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.numel() == 1 and b.numel() == 1:
        return _WeightedPair.apply(a, b, wa, wb)
    return wa * a + wb * b


class _BATerms(torch.autograd.Function):
    """BA.run_ba's loss lines outside the render (pipelines/BA.py:160-170) as one fused node each way (include/ls2fm.h:
    ls2fm_ba_terms_fwd / _bwd): (sdf_surf, w_reproj, extra) with sdf_surf = mean |sdfs|, w_reproj = w_hi where the re-projection
    error exceeds `thresh` else w_lo (from the detached error), extra = w_reproj reproj + w_surf sdf_surf + w_add add.  Only
    `extra` carries a gradient (the other two are the log's)."""

    @staticmethod
    def forward(ctx, reproj, sdfs, add, thresh, w_lo, w_hi, w_surf, w_add):
        lib = _lib.load()
        r, s = _f32(reproj, 1), _f32(sdfs, -1)
        a = None if add is None else _f32(add, 1)
        surf, w, extra = (torch.empty((), device=s.device) for _ in range(3))
        _lib.check(lib.ls2fm_ba_terms_fwd(_lib.ptr(r), _lib.ptr(s), s.numel(), _lib.ptr(a), float(thresh), float(w_lo), float(w_hi),
                                          float(w_surf), float(w_add), _lib.ptr(surf), _lib.ptr(w), _lib.ptr(extra), _lib.stream_ptr()),
                   "ls2fm_ba_terms_fwd")
        ctx.save_for_backward(s, w)
        ctx.consts = (float(w_surf), float(w_add), reproj.shape, sdfs.shape, None if add is None else add.shape)
        ctx.mark_non_differentiable(surf, w)
        ctx.set_materialize_grads(False)
        return surf, w, extra

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_surf, g_w, g):
        lib = _lib.load()
        s, w = ctx.saved_tensors
        w_surf, w_add, shape_r, shape_s, shape_a = ctx.consts
        if g is None:
            return (None,) * 8
        g = _f32(g, 1)
        d_r, d_s = torch.empty(1, device=s.device), torch.empty_like(s)
        d_a = None if shape_a is None else torch.empty(1, device=s.device)
        _lib.check(lib.ls2fm_ba_terms_bwd(_lib.ptr(s), s.numel(), _lib.ptr(w), _lib.ptr(g), w_surf, w_add, _lib.ptr(d_r), _lib.ptr(d_s),
                                          _lib.ptr(d_a), _lib.stream_ptr()), "ls2fm_ba_terms_bwd")
        return d_r.view(shape_r), d_s.view(shape_s), (None if d_a is None else d_a.view(shape_a)), None, None, None, None, None


class _MatchTerm(torch.autograd.Function):
    """the explicit-match terms of the two-view initialisation as one fused node (include/ls2fm.h: ls2fm_match_term_fwd / _bwd):
    (reproj_error, sdf_surf) from the traced depths and last SDF values of each source view; `surface` receives the traced points"""

    @staticmethod
    def _pointers(tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    @staticmethod
    def forward(ctx, fixed, surface, *ds):
        lib = _lib.load()
        center, ray, uv_obs, poses, k_host, n = fixed
        S = len(ds) // 2
        d, sl = [_f32(t, -1) for t in ds[:S]], [_f32(t, -1) for t in ds[S:]]
        arr = _MatchTerm._pointers
        out = torch.empty(2, device=center.device)
        _lib.check(lib.ls2fm_match_term_fwd(_lib.ptr(center), _lib.ptr(ray), _lib.ptr(uv_obs), _lib.ptr(poses), k_host, S, n, arr(d), arr(sl),
                                            _lib.ptr(surface), _lib.ptr(out), _lib.stream_ptr()), "ls2fm_match_term_fwd")
        ctx.fixed, ctx.S = fixed, S
        ctx.shapes = [t.shape for t in ds]
        ctx.save_for_backward(*d, *sl)
        ctx.set_materialize_grads(False)
        return out[0], out[1]            # (tensors of their own: no select backward -- a fill + a copy per term -- behind them)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g0, g1):
        lib = _lib.load()
        center, ray, uv_obs, poses, k_host, n = ctx.fixed
        S = ctx.S
        saved = ctx.saved_tensors
        d, sl = list(saved[:S]), list(saved[S:])
        dd, dsl = [torch.empty_like(t) for t in d], [torch.empty_like(t) for t in sl]
        arr = _MatchTerm._pointers
        if g0 is not None and g1 is not None and g0.dtype == torch.float32 and g1.dtype == torch.float32 and \
                g1.data_ptr() == g0.data_ptr() + 4:
            g = g0                       # the halves of one buffer (_WeightedPair's backward): the kernel reads g[0], g[1] from there
        else:
            zero = torch.zeros((), device=center.device)
            g = torch.stack([(zero if t is None else t).reshape(()).float() for t in (g0, g1)])
        _lib.check(lib.ls2fm_match_term_bwd(_lib.ptr(center), _lib.ptr(ray), _lib.ptr(uv_obs), _lib.ptr(poses), k_host, S, n, arr(d), arr(sl),
                                            _lib.ptr(g), arr(dd), arr(dsl), _lib.stream_ptr()), "ls2fm_match_term_bwd")
        grads = [t.view(sh) for t, sh in zip(dd + dsl, ctx.shapes)]
        return (None, None, *grads)


class _Reproject(torch.autograd.Function):
    """ls2fm_reproject_fwd / _bwd: the re-projection term of a BA iteration (BA.py:126-147, 199-202) as one node
    -> (reproj scalar, counted bool [n])"""

    @staticmethod
    def forward(ctx, points, poses, view_start, k_host, obs_uv, sdf, bound):
        lib = _lib.load()
        x, ps = _f32(points), _f32(poses)
        _lib.require_device(x)
        n, n_views, dev = x.shape[0], ps.shape[0], x.device
        err = torch.empty(n, device=dev)
        on = torch.empty(n, device=dev, dtype=torch.uint8)
        sums = torch.empty(4, device=dev, dtype=torch.float64)
        ws = torch.empty(int(lib.ls2fm_reproject_workspace_bytes(n_views)) // 8, device=dev, dtype=torch.float64)
        sdf_c = None if sdf is None else _f32(sdf, -1)
        _lib.check(lib.ls2fm_reproject_fwd(_lib.ptr(x), _lib.ptr(ps), _lib.ptr(view_start), n_views, k_host, _lib.ptr(obs_uv), _lib.ptr(sdf_c),
                                           float(bound), n, _lib.ptr(err), _lib.ptr(on), _lib.ptr(sums), _lib.ptr(ws),
                                           _lib.stream_ptr()), "ls2fm_reproject_fwd")
        ctx.save_for_backward(x, ps, view_start, obs_uv, sdf_c if sdf_c is not None else x.new_empty(0), sums)
        ctx.k_host, ctx.bound, ctx.has_sdf = k_host, float(bound), sdf_c is not None
        counted = on.view(torch.bool)
        ctx.mark_non_differentiable(counted)
        ctx.set_materialize_grads(False)         # (no zero fill for the bool output's "gradient" in the backward)
        return sums[3].float(), counted

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_reproj, _):
        lib = _lib.load()
        x, ps, view_start, obs_uv, sdf_c, sums = ctx.saved_tensors
        if d_reproj is None:
            return (None,) * 7
        d_x, d_ps = torch.empty_like(x), torch.empty_like(ps)
        g = _f32(d_reproj, 1)
        _lib.check(lib.ls2fm_reproject_bwd(_lib.ptr(x), _lib.ptr(ps), _lib.ptr(view_start), ps.shape[0], ctx.k_host, _lib.ptr(obs_uv),
                                           _lib.ptr(sdf_c) if ctx.has_sdf else None, ctx.bound, x.shape[0], _lib.ptr(sums), _lib.ptr(g),
                                           _lib.ptr(d_x), _lib.ptr(d_ps), _lib.stream_ptr()), "ls2fm_reproject_bwd")
        return d_x, d_ps, None, None, None, None, None


def reprojection_term(points, poses, view_start, intrinsic_host, obs_uv, sdf=None, bound=float("inf")):
    """points [n,3] (observations sorted by view: view v owns rows view_start[v] : view_start[v + 1], int32 [V + 1] on the device),
    poses [V,3,4] world-to-camera, intrinsic_host: the 3 x 3 K as 9 host floats (`ctypes` array, see `host_intrinsic`), obs_uv
    [n,2] -> (reproj, counted [n] bool): 0.5 mean(2 log(1 + err^2 / 4)) + 0.5 mean(err) over the observations with
    |sdf| < bound and a finite projection (BA.py:126-147, 199-202); differentiable w.r.t. points and poses"""
    return _Reproject.apply(points, poses, view_start, intrinsic_host, obs_uv.float().contiguous(), sdf, bound)


def host_intrinsic(intrinsic):
    return (ctypes.c_float * 9)(*[float(v) for v in intrinsic.detach().reshape(-1).cpu().tolist()])
