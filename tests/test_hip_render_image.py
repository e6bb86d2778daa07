"""GPU: forward-only image rendering (ls2fm_render_image through ls2fm.image) against the training forward it must equal bit for
bit (Renderer.forward on the rays ls2fm_camera_rays forms for every pixel), the CPU oracle, and its own properties: any image
size in one call with a bounded workspace, several views, determinism, graph capture, the drop-in and the fallback."""
import math

import pytest
import torch

from ls2fm import _lib, fused, image
from ls2fm.models.RadF import RadF
from ls2fm.models.Renderer import Renderer
from ls2fm.models.SDF import SDF
from ls2fm.options import make_options
from ls2fm.utils import camera as cam

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _scene(ds="DTU", dual=True, n=128, levels=16, log2=19, seed=0):
    enc = dict(n_levels=levels, n_features_per_level=2, log2_hashmap_size=log2, base_resolution=16)
    opt = make_options(ds, device=DEV, dual_field=dual, sample_intvs=n, hash_encoding=enc)
    torch.manual_seed(seed)
    sdf, rad, ren = SDF(opt).to(DEV), RadF(opt).to(DEV), Renderer(opt)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in (sdf, rad):
            for name, p in mod.named_parameters():
                if name.endswith("embedder_obj.params"):
                    p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1).to(DEV))
                if name.endswith("mlp.0.weight_v") and "Rad_dec" not in name:
                    p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=gen) * 0.05).to(DEV)
    return opt, sdf, rad, ren


def _view(opt, H, W, V=1, seed=3):
    """V poses looking at the scene box from 4 half-sizes away, slightly turned: the box fills the middle of the image, the
    corners miss it (rays with no hit: background only)"""
    h = float(opt.data.bound_max[0])
    g = torch.Generator().manual_seed(seed)
    se3 = torch.cat([0.15 * torch.randn(V, 3, generator=g), 0.1 * h * torch.randn(V, 3, generator=g)], dim=1)
    se3[:, 5] += 4.0 * h
    poses = cam.lie.se3_to_SE3(se3.to(DEV)).contiguous()
    intr = torch.tensor([[1.0 * W, 0.0, W / 2.0], [0.0, 1.0 * W, H / 2.0], [0.0, 0.0, 1.0]], device=DEV)
    return poses, intr


def _sliced(ren, opt, sdf, rad, poses, intr, H, W, pix=None):
    """the training forward on the rays camera_rays forms for the pixels, in 8192-ray slices"""
    kinv = cam.host_inverse_intrinsic(intr)
    pix = torch.arange(H * W, device=DEV) if pix is None else pix
    c, r = cam.camera_rays(kinv, poses=poses, pix=pix, width=W)
    out = {"rgb": [], "depth_mlp": [], "normal_mlp": []}
    with torch.no_grad():
        for s in range(0, c.shape[1], 8192):
            ret = ren.forward(opt, c[:, s:s + 8192], r[:, s:s + 8192], sdf, rad)
            for k in out:
                out[k].append(ret[k])
    return {k: torch.cat(v, dim=1) for k, v in out.items()}


def _equal(img, ref, sel=slice(None)):
    assert torch.equal(img.rgb[:, sel], ref["rgb"]), "rgb"
    assert torch.equal(img.depth[:, sel], ref["depth_mlp"]), "depth"
    assert torch.equal(img.norm[:, sel], ref["normal_mlp"]), "normal"


CASES = [
    ("DTU", True, 128, "on"), ("DTU", True, 128, "off"), ("DTU", False, 128, "off"),
    ("ETH3D", False, 48, "off"), ("ETH3D", True, 48, "on"), ("ETH3D", True, 320, "on"),
    ("BlendedMVS", True, 128, "on"), ("BlendedMVS", False, 320, "off"), ("DTU", True, 48, "off"),
]


@pytest.mark.parametrize("ds,dual,n,table", CASES)
def test_image_equals_the_training_forward_bit_for_bit(ds, dual, n, table, monkeypatch):
    monkeypatch.setattr(fused, "_DUAL_TABLE", "version" if table == "on" else "off")
    opt, sdf, rad, ren = _scene(ds, dual, n)
    H, W = 40, 56
    poses, intr = _view(opt, H, W)
    img = image.render_image(ren, opt, sdf, rad, poses[0], intr, H=H, W=W, opacity=True)
    assert img.rgb.shape == (1, H * W, 3) and img.depth.shape == (1, H * W, 1) and img.norm.shape == (1, H * W, 3)
    ref = _sliced(ren, opt, sdf, rad, poses, intr, H, W)
    _equal(img, ref)
    bg = torch.tensor(ren.bg_host, device=DEV)
    miss = img.opacity[0, :, 0] == 0
    assert 0 < int(miss.sum()) < H * W, "the view must both hit and miss the scene box"
    assert torch.equal(img.rgb[0, miss], bg.expand(int(miss.sum()), 3)), "misses: background only"
    assert bool(((img.opacity >= 0) & (img.opacity <= 1.0 + 1e-6)).all())


def test_image_against_the_cpu_oracle():
    from oracle import fields as OF
    opt, sdf, rad, ren = _scene("ETH3D", True, 32, levels=8, log2=14)
    H, W = 12, 16
    poses, intr = _view(opt, H, W)
    img = image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W)
    # the torch ray construction agrees with the kernels' to a few ulp (the summation order of its 3- and 4-term products and
    # of `world - center`, test_hip_camera_rays.py); the oracle is fed the kernels' rays -- a ray that grazes a hash cell boundary or the box would
    # otherwise show an ulp of the ray as a different cell
    grid = cam.mesh_grid(H=H, W=W, device="cpu")
    c_t, r_t = cam.get_center_and_ray(None, poses.cpu(), intr=intr.cpu().unsqueeze(0), xy_grid=grid)
    c, r = cam.camera_rays(cam.host_inverse_intrinsic(intr), poses=poses, pix=torch.arange(H * W, device=DEV), width=W)
    c, r = c.cpu(), r.cpu()
    assert float((c - c_t).abs().max()) <= 1e-5 and float((r - r_t).abs().max()) <= 1e-5
    cfg = OF.dataset_config("ETH3D", dual_field=True, sample_intvs=32, n_levels=8, log2_hashmap_size=14)
    osd = {k: v.detach().cpu() for k, v in sdf.state_dict().items()}
    ord_ = {k: v.detach().cpu() for k, v in rad.state_dict().items()}
    with torch.no_grad():
        oret = OF.render(cfg, c, r, osd, ord_)
    for got, key in ((img.rgb, "rgb"), (img.depth, "depth_mlp"), (img.norm, "normal_mlp")):
        ref = oret[key].double()
        err = float((got.cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))
        assert err < 1e-4, f"{key}: {err:.2e}"


def test_large_image_in_one_call_with_a_bounded_workspace():
    opt, sdf, rad, ren = _scene("DTU", True, 128)
    H, W = 1200, 1600
    assert H * W * 128 > _lib.MAX_RENDER_POINTS
    poses, intr = _view(opt, H, W)
    image.render_image(ren, opt, sdf, rad, poses, intr, H=8, W=8)            # plan, interleaved table, K^-1 in place
    plan = fused._plan(ren, opt, sdf, rad)
    ws = plan.ws_bytes["image"]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    img = image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W)
    torch.cuda.synchronize()
    outputs = 7 * 4 * H * W
    grow = torch.cuda.max_memory_allocated() - base
    assert grow <= outputs + ws + (16 << 20), (grow, outputs, ws)
    # one 8192-ray slice of the sliced path allocates more than the whole image call's workspace
    kinv = cam.host_inverse_intrinsic(intr)
    c, r = cam.camera_rays(kinv, poses=poses, pix=torch.arange(8192, device=DEV), width=W)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        ret = ren.forward(opt, c, r, sdf, rad)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base > ws
    del ret
    # the whole image equals the sliced training forward (every chunk boundary included)
    ref = _sliced(ren, opt, sdf, rad, poses, intr, H, W)
    _equal(img, ref)
    rows = [0, H // 2, H - 1]
    for y in rows:
        sel = slice(y * W, (y + 1) * W)
        _equal(img, {k: v[:, sel] for k, v in ref.items()}, sel)


def test_views_determinism_and_graph_capture():
    opt, sdf, rad, ren = _scene("DTU", True, 128)
    H, W = 40, 56
    poses, intr = _view(opt, H, W, V=4)
    many = image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W, opacity=True)
    assert many.rgb.shape == (4, H * W, 3) and many.opacity.shape == (4, H * W, 1)
    for v in range(4):
        one = image.render_image(ren, opt, sdf, rad, poses[v], intr, H=H, W=W, opacity=True)
        for k in ("rgb", "depth", "norm", "opacity"):
            assert torch.equal(many[k][v], one[k][0]), (k, v)
    again = image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W, opacity=True)
    for k in ("rgb", "depth", "norm", "opacity"):
        assert torch.equal(many[k], again[k]), k
    # captured once, replayed after the pose is rewritten in place
    pose = poses[0].clone()
    image.render_image(ren, opt, sdf, rad, pose, intr, H=H, W=W)              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            cap = image.render_image(ren, opt, sdf, rad, pose, intr, H=H, W=W)
    torch.cuda.current_stream().wait_stream(s)
    pose.copy_(poses[2])
    g.replay()
    torch.cuda.synchronize()
    eager = image.render_image(ren, opt, sdf, rad, poses[2], intr, H=H, W=W)
    for k in ("rgb", "depth", "norm"):
        assert torch.equal(cap[k], eager[k]), k


class _FakeCamera:
    """what the reference's Camera.render_img_by_slices reads: get_pose(), intrinsic, opt"""

    def __init__(self, opt, pose, intr):
        self.opt, self._pose, self.intrinsic = opt, pose, intr

    def get_pose(self):
        return self._pose


def test_drop_in_and_the_fallback():
    opt, sdf, rad, ren = _scene("DTU", True, 64, levels=8, log2=14)
    H, W = 24, 32
    opt.H, opt.W = H, W
    poses, intr = _view(opt, H, W)
    camo = _FakeCamera(opt, poses, intr)
    ret = image.render_img_by_slices(camo, sdf, rad, ren)
    assert set(ret.keys()) == {"depth", "norm", "rgb"}
    assert ret.depth.shape == (1, H * W, 1) and ret.norm.shape == (1, H * W, 3) and ret.rgb.shape == (1, H * W, 3)
    novel = poses.repeat(3, 1, 1)
    ret3 = image.render_img_by_slices(camo, sdf, rad, ren, pose_input=novel)
    assert ret3.rgb.shape == (3, H * W, 3) and torch.equal(ret3.rgb[2], ret.rgb[0])
    # bg_sdf: the fused kernels refuse it -> the reference's loop (Renderer.forward per rand_rays slice)
    opt.data.bg_sdf = True
    assert not fused.supported(opt, sdf, rad)
    opt.Renderer.rand_rays = 200
    fb = image.render_image(ren, opt, sdf, rad, poses, intr, H=H, W=W)
    grid = cam.mesh_grid(H=H, W=W, device=DEV)
    c, r = cam.get_center_and_ray(opt, poses, intr=intr.unsqueeze(0), xy_grid=grid)
    with torch.no_grad():
        parts = [ren.forward(opt, c[:, s:s + 200], r[:, s:s + 200], sdf, rad) for s in range(0, H * W, 200)]
    # (the composed form is not bit-reproducible from call to call: held to the project's fp32 bar)
    for got, key in ((fb.rgb, "rgb"), (fb.depth, "depth_mlp"), (fb.norm, "normal_mlp")):
        ref = torch.cat([p[key] for p in parts], dim=1)
        assert got.shape == ref.shape
        err = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
        assert err < 1e-5, f"{key}: {err:.2e}"
    assert not math.isnan(float(fb.rgb.sum()))
