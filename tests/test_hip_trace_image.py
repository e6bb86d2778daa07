"""GPU: sphere-traced depth and normal maps of whole images (ls2fm_trace_image through ls2fm.image) against the paths they replace:
SDF.sphere_tracing(static_trips=True) on the rays ls2fm_camera_rays forms for every pixel and SDF.gradient at the surface points,
bit for bit per view; the host-synchronising form; the CPU oracle; per-view trip counts, a full-size image, determinism, graph
capture and the Camera.get_depth drop-in with its fallbacks."""
import copy
import math

import pytest
import torch

from ls2fm import fused, image
from ls2fm.models.SDF import SDF
from ls2fm.options import make_options
from ls2fm.utils import camera as cam

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _field(ds="DTU", dual=True, levels=16, log2=19, seed=0, table_amp=0.1, w_std=0.05):
    enc = dict(n_levels=levels, n_features_per_level=2, log2_hashmap_size=log2, base_resolution=16)
    opt = make_options(ds, device=DEV, dual_field=dual, hash_encoding=enc)
    torch.manual_seed(seed)
    sdf = SDF(opt).to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in sdf.named_parameters():
            if name.endswith("embedder_obj.params"):
                p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * table_amp).to(DEV))
            if name.endswith("mlp.0.weight_v") and w_std > 0:
                p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=gen) * w_std).to(DEV)
    return opt, sdf


def _views(opt, H, W, V=1, seed=3, away=()):
    """V poses looking at the scene box from 4 half-sizes away, slightly turned: the box fills the middle, the corners miss it.
    Views listed in `away` are turned round (every ray misses the box)"""
    h = float(opt.data.bound_max[0])
    g = torch.Generator().manual_seed(seed)
    se3 = torch.cat([0.15 * torch.randn(V, 3, generator=g), 0.1 * h * torch.randn(V, 3, generator=g)], dim=1)
    se3[:, 5] += 4.0 * h
    for v in away:
        se3[v, 1] += math.pi
    poses = cam.lie.se3_to_SE3(se3.to(DEV)).contiguous()
    intr = torch.tensor([[1.0 * W, 0.0, W / 2.0], [0.0, 1.0 * W, H / 2.0], [0.0, 0.0, 1.0]], device=DEV)
    return poses, intr


def _rays(poses, intr, H, W):
    return cam.camera_rays(cam.host_inverse_intrinsic(intr), poses=poses, pix=torch.arange(H * W, device=DEV), width=W)


def _static(sdf, c, r):
    with torch.no_grad():
        d, last, _, fin = sdf.sphere_tracing(c, r, sdf, static_trips=True)
    return d.reshape(-1), last.reshape(-1), fin.reshape(-1), int(sdf.last_trips.item())


def _assert_view_equals_static(sdf, t, v, c, r):
    d, last, fin, k = _static(sdf, c, r)
    assert int(t.trips[v]) == k, "trips"
    assert torch.equal(t.depth[v, :, 0], d), "depth"
    assert torch.equal(t.sdf_last[v], last), "sdf_last"
    assert torch.equal(t.finish[v], fin), "finish"
    pts = c[0] + t.depth[v] * r[0]                        # the reference's surface points: a product, then a sum
    assert torch.equal(t.points[v], pts), "points"
    nrm = fused.query_points(sdf, t.points[v], want_normal=True)[2]
    assert torch.equal(t.gradient[v], nrm.detach()), "gradient"


CASES = [("DTU", True), ("DTU", False), ("ETH3D", True), ("ETH3D", False), ("BlendedMVS", True), ("BlendedMVS", False)]


@pytest.mark.parametrize("ds,dual", CASES)
def test_view_equals_static_tracing_and_gradient_bit_for_bit(ds, dual):
    opt, sdf = _field(ds, dual)
    H, W = 37, 53
    poses, intr = _views(opt, H, W)
    t = image.trace_image(sdf, poses[0], intr, H=H, W=W)
    assert t.depth.shape == (1, H * W, 1) and t.points.shape == (1, H * W, 3) and t.gradient.shape == (1, H * W, 3)
    assert t.finish.dtype == torch.bool and t.trips.dtype == torch.int32 and t.trips.shape == (1,)
    c, r = _rays(poses, intr, H, W)
    _assert_view_equals_static(sdf, t, 0, c, r)
    # some pixels miss the box (near = far = -1), some hit it
    with torch.no_grad():
        near, far, _, _, _ = fused.sphere_trace(sdf, c[0], r[0], sync=False)
    miss = far < 0
    assert 0 < int(miss.sum()) < H * W
    # the host-synchronising form (torch's sum over the track): the sequential sum's bar (test_traced_depth_node_equals_torch_tail)
    from conftest import rel_err
    with torch.no_grad():
        d_ref, last_ref, _, fin_ref = sdf.sphere_tracing(c, r, sdf)
    assert int(sdf.last_trips) == int(t.trips[0])
    assert rel_err(t.depth[0, :, 0], d_ref.reshape(-1)) < 2e-6
    assert torch.equal(t.sdf_last[0], last_ref.reshape(-1))


def test_per_view_trip_counts():
    """each view of a call gets the K a call over that view alone gets: a view whose rays all miss stops after one trip, a
    converging view after a few, a noisy one at iters_max; a call-global K would change the early views' depths"""
    opt, noisy = _field("DTU", True, seed=5)
    H, W = 29, 41
    poses, intr = _views(opt, H, W, V=3, away=(1,))
    _, smooth = _field("DTU", True, seed=5, table_amp=0.002, w_std=0.0)
    for sdf in (noisy, smooth):
        t = image.trace_image(sdf, poses, intr, H=H, W=W)
        c, r = _rays(poses, intr, H, W)
        for v in range(3):
            one = image.trace_image(sdf, poses[v], intr, H=H, W=W)
            for k in ("depth", "sdf_last", "finish", "points", "gradient", "t_end_k", "trips"):
                assert torch.equal(t[k][v], one[k][0]), (k, v)
            _assert_view_equals_static(sdf, t, v, c[v:v + 1], r[v:v + 1])
        assert int(t.trips[1]) <= 1 < int(t.trips[0])                  # the views' K differ
    # rays whose start end converged before the view's K still carry the terms up to K: their last track value repeats and the
    # depth is the sequential sum over all K of them
    t = image.trace_image(smooth, poses[0], intr, H=H, W=W)
    K = int(t.trips[0])
    assert K > 2
    c, r = _rays(poses[:1], intr, H, W)
    thr = float(smooth.sdf_threshold)
    with torch.no_grad():
        near, far, track, _, _ = fused.sphere_trace(smooth, c[0], r[0], sync=False)
        vals = smooth.infer_sdf(track[:, :K].reshape(-1, 3)).view(-1, K)
    early = (vals[:, :K - 1].abs() <= thr).any(dim=1) & (vals[:, K - 1] != 0) & (far > 0)
    assert bool(early.any())
    acc = torch.zeros_like(near)
    for k in range(K):
        acc = acc + vals[:, k]
    d = acc + near
    assert torch.equal(t.depth[0, :, 0][early], torch.where(d > far, far, d)[early])


def test_against_the_cpu_oracle_on_a_converging_field():
    from oracle import fields as OF
    from conftest import rel_err
    opt, sdf = _field("DTU", True, levels=8, log2=14, seed=7, table_amp=0.002, w_std=0.0)
    H, W = 12, 16
    poses, intr = _views(opt, H, W)
    t = image.trace_image(sdf, poses, intr, H=H, W=W)
    c, r = _rays(poses, intr, H, W)
    cfg = OF.dataset_config("DTU", n_levels=8, log2_hashmap_size=14)
    osd = {k: v.detach().cpu() for k, v in sdf.state_dict().items()}
    with torch.no_grad():
        d_o, last_o, _, fin_o, trips_o = OF.sphere_tracing(cfg, c.cpu(), r.cpu(), osd, rng=False)
    assert int(t.trips[0]) == int(trips_o)
    d = t.depth[0, :, 0].cpu()
    assert torch.allclose(d, d_o.reshape(-1).float(), rtol=1e-4, atol=1e-5)
    assert float((t.sdf_last[0].cpu() - last_o.reshape(-1)).abs().max()) < 1e-5 * float(opt.data.bound_max[0])
    g_o = OF.sdf_gradient(t.points[0].cpu().clone(), osd, cfg, cfg.table()).detach()
    assert rel_err(t.gradient[0].cpu(), g_o) < 1e-4


def test_full_size_dtu_view_and_bounded_memory():
    opt, sdf = _field("DTU", True)
    H, W = 1200, 1600
    poses, intr = _views(opt, H, W)
    image.trace_image(sdf, poses, intr, H=8, W=8)                      # K^-1 in place, first-call allocations
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = image.trace_image(sdf, poses, intr, H=H, W=W)
    torch.cuda.synchronize()
    outputs = (1 + 1 + 3 + 3 + 1) * 4 * H * W + H * W + 4                 # depth, sdf_last, points, gradient, t_end_k, finish, trips
    grow = torch.cuda.max_memory_allocated() - base
    assert grow <= outputs + (8 << 20), (grow, outputs)
    c, r = _rays(poses, intr, H, W)
    _assert_view_equals_static(sdf, t, 0, c, r)


def test_determinism_and_graph_capture():
    opt, sdf = _field("ETH3D", True)
    H, W = 31, 45
    poses, intr = _views(opt, H, W, V=3)
    a = image.trace_image(sdf, poses, intr, H=H, W=W)
    b = image.trace_image(sdf, poses, intr, H=H, W=W)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    pose = poses[0].clone()
    image.trace_image(sdf, pose, intr, H=H, W=W)                       # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            cap = image.trace_image(sdf, pose, intr, H=H, W=W)
    torch.cuda.current_stream().wait_stream(s)
    pose.copy_(poses[2])
    g.replay()
    torch.cuda.synchronize()
    eager = image.trace_image(sdf, poses[2], intr, H=H, W=W)
    for k in eager:
        assert torch.equal(cap[k], eager[k]), k


class _FakeCamera:
    """what the reference's Camera.get_depth reads: get_pose(), intrinsic, opt"""

    def __init__(self, opt, pose, intr):
        self.opt, self._pose, self.intrinsic = opt, pose, intr

    def get_pose(self):
        return self._pose


def _states():
    return torch.cuda.get_rng_state().clone(), torch.get_rng_state().clone()


def _compare(got, ref, norm_hw):
    """keys, shapes, and values: the device depth is the sequential sum (2e-6 of torch's); where the depth bits agree, so do the
    surface points and everything formed from them"""
    from conftest import rel_err
    assert set(got.keys()) == set(ref.keys()) == {"depth", "mask_finish", "norms", "pts_surface", "normals_value", "sdf_surf",
                                                  "sample_pts"}
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    assert got.norms.shape == (1, *norm_hw, 3)
    assert rel_err(got.depth, ref.depth) < 2e-6
    for k in ("mask_finish", "sdf_surf", "sample_pts"):
        assert torch.equal(got[k], ref[k].detach()), k
    same = (got.depth == ref.depth)[:, 0]
    assert float(same.float().mean()) > 0.5
    assert torch.equal(got.pts_surface.detach()[same], ref.pts_surface.detach()[same])
    assert torch.equal(got.normals_value[same], ref.normals_value.detach()[same])
    assert torch.equal(got.norms.view(-1, 3)[same], ref.norms.detach().view(-1, 3)[same])
    assert got.pts_surface.requires_grad                      # SDF.gradient marks the surface points


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_drop_in_get_depth(mode):
    opt, sdf = _field("DTU", True, levels=8, log2=14)
    H, W = 48, 64
    opt.H, opt.W = H, W
    opt.data.image_size = [H, W]
    poses, intr = _views(opt, H, W)
    camo = _FakeCamera(opt, poses[:1], intr)
    h, w = (H // 4, W // 4) if mode == "eval" else (H, W)
    ki = intr.clone()
    if mode == "eval":
        ki[:2] /= 4
        ki[2, 2] = 1.0
    torch.manual_seed(11)
    with torch.no_grad():
        got = image.get_depth(camo, sdf, mode=mode)
    st_got = _states()
    assert (opt.H, opt.W) == (H, W)
    # the reference's steps on the same rays (the kernels' rays: get_center_and_ray differs from them by a few ulp)
    c, r = _rays(poses[:1], ki, h, w)
    torch.manual_seed(11)
    with torch.no_grad():
        ref = image.depth_body(sdf, c, r, (h, w))
    st_ref = _states()
    assert torch.equal(st_got[0], st_ref[0]) and torch.equal(st_got[1], st_ref[1]), "generator states"
    _compare(got, ref, (h, w))


def test_get_depth_fallbacks():
    opt, sdf = _field("DTU", True, levels=8, log2=14)
    H, W = 24, 32
    opt.H, opt.W = H, W
    opt.data.image_size = [H, W]
    poses, intr = _views(opt, H, W)
    camo = _FakeCamera(opt, poses[:1], intr)
    # grad enabled: the reference's steps, with the graph of the traced depth
    torch.manual_seed(2)
    got = image.get_depth(camo, sdf, mode="train")
    assert got.depth.requires_grad
    grid = cam.mesh_grid(opt, device=DEV)
    c, r = cam.get_center_and_ray(opt, poses[:1], intr=intr, xy_grid=grid)
    torch.manual_seed(2)
    ref = image.depth_body(sdf, c, r, (H, W))
    for k in ref:
        assert torch.equal(got[k].detach(), ref[k].detach()), k
    # bg_sdf: the tracing kernels refuse it
    opt.data.bg_sdf = True
    assert not image.can_trace_image(sdf, poses)
    torch.manual_seed(2)
    with torch.no_grad():
        fb = image.get_depth(camo, sdf, mode="eval")
    assert fb.norms.shape == (1, H // 4, W // 4, 3) and (opt.H, opt.W) == (H, W)
    with pytest.raises(RuntimeError):
        image.trace_image(sdf, poses, intr, H=H, W=W)
    ki = copy.deepcopy(intr)
    ki[:2] /= 4
    ki[2, 2] = 1.0
    opt.H, opt.W = H // 4, W // 4
    c, r = cam.get_center_and_ray(opt, poses[:1], intr=ki)
    opt.H, opt.W = H, W
    torch.manual_seed(2)
    with torch.no_grad():
        ref = image.depth_body(sdf, c, r, (H // 4, W // 4))
    from conftest import rel_err
    for k in ref:                                 # the composed gradient is not bit-reproducible from call to call
        assert fb[k].shape == ref[k].shape, k
        if fb[k].dtype == torch.bool:
            assert torch.equal(fb[k], ref[k]), k
        else:
            assert rel_err(fb[k], ref[k]) < 1e-5, k
