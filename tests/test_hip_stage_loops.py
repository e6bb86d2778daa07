"""The stage LOOPS (ls2fm.stage.InitLoop / RefineLoop / BALoop / GeoInitLoop) against K = 20 consecutive iterations
of the REFERENCE's own loops -- `Initializer.run` (pipelines/Initialization.py:139-226), `Refine.run`
(pipelines/rendering_refine.py:72-97), `BA.run_ba` (pipelines/BA.py:110-188, mode "sfm_refine") and `Registration.geo_init_nf`
(pipelines/Registration.py:133-296), run through the reference's Camera / CameraSet / Point3DSet objects with torch.optim.Adam + ExponentialLR and
recorded by tests/golden/make_golden_stage.py: per-iteration loss terms and PSNR, the final parameters (fields, poses), the
final points.  The RNG draws that pick a step's inputs (ray permutation head, the random view of the tracing consistency) are
replayed from the recording; everything else is the product's: fused render with the loss head inside, fused tracing and
point queries, FusedAdam with the schedule on the device, no host synchronisation inside an iteration.

Bars: the trajectory bars of test_stage_trajectory_matches_plain_torch (3e-3 on the total loss, 5e-2 on dense weights); a
20-step Adam trajectory amplifies last-bit differences of the field evaluation through sphere tracing's `t += sdf` and
through Adam's g / sqrt(v) on near-zero gradients, so single terms get their own, looser bars where noted."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import options_for
from ls2fm.models.SDF import SDF
from ls2fm.models.RadF import RadF
from ls2fm.models.Renderer import Renderer
from ls2fm import stage

pytestmark = pytest.mark.gpu
DEV = "cuda"


# Bars of _tables_close: relative L2 of the tables' UPDATE, fraction of entries further apart than a tenth of the largest update,
# fraction that moved in one run only.  Measured over the four loop goldens, eager and captured (gpurun_out -> profiles/r06_raw/
# c74_tables.txt): SDF grid 0.012 - 0.127 / 2e-4 - 4.3e-2 / 0, second grid 1.2e-3 - 3.1e-2 / 0 - 1.5e-3 / 1.5e-4 - 2.6e-4 -- twenty
# Adam steps turn a gradient that is rounding noise around zero into +-lr steps (the SDF grid's eikonal / tracing terms are such
# sums); WHICH entries receive a gradient at all is the structural check and agrees to 3e-4.
TABLE_BARS = {"sdf_final": (0.25, 0.08, 1e-3), "rad_final": (0.06, 5e-3, 1e-3)}


def _scene(g):
    meta = json.loads(bytes(g["meta_json"]).decode())
    meta["bg_sdf"] = None
    opt = options_for(meta, DEV)
    opt.Res = meta["Res"]
    sdf, rad, ren = SDF(opt).to(DEV), RadF(opt).to(DEV), Renderer(opt)
    sdf.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sdf0/")}, strict=True)
    rad.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("rad0/")}, strict=True)
    H, W = int(g["H"]), int(g["W"])
    images = torch.from_numpy(g["images"]).to(DEV)                                 # [V,3,H,W] as the reference's Camera keeps them
    images = images.reshape(images.shape[0], 3, -1).permute(0, 2, 1).contiguous()  # Camera.render: img_gt.view(3,-1).permute(1,0)
    kp = [torch.from_numpy(k).to(DEV) for k in g["kypts"]]
    ids = [torch.arange(k.shape[0], device=DEV) for k in kp]
    views = stage.TrackedViews(torch.from_numpy(g["poses"]).to(DEV), torch.from_numpy(g["intrinsic"]).to(DEV), images, kp, ids,
                               torch.from_numpy(g["xyzs"]).to(DEV).clone(), H, W)
    cams = g["cam_pick"] if len(g["cam_pick"]) else np.zeros(meta["iters"], np.int32)      # the init loop draws no view
    picks = [(torch.from_numpy(g["rays_idx"][i]).to(DEV), int(cams[i])) for i in range(meta["iters"])]
    return meta, opt, sdf, rad, ren, views, picks


def _close(name, got, ref, rtol, atol=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    ok = err <= rtol * np.abs(ref) + atol
    assert ok.all(), f"{name}: worst {err.max():.3g} at iteration {int(err.argmax())}: {got[err.argmax()]:.6g} vs {ref[err.argmax()]:.6g}"


def _dense_close(mod, g, prefix, tol=5e-2):
    for k, v in mod.state_dict().items():
        if k.endswith("embedder_obj.params"):
            continue                                            # tables: Adam turns every non-zero gradient into a +-lr step
        ref = torch.from_numpy(g[f"{prefix}/{k}"])
        assert float((v.cpu() - ref).abs().max()) <= tol * float(ref.abs().max()) + 1e-6, (prefix, k)


def _tables_close(mod, g, prefix0, prefix, l2_bar, far_bar, touched_bar):
    """the hash tables after the loop, through the UPDATE they received (final - initial; the tables themselves are dominated by
    their initial values).  Adam turns every non-zero gradient into a step of ~lr whatever its size, so an entry whose gradient is
    rounding noise around zero moves by +-lr per iteration in either run: the update is held in the relative L2 norm, by the
    fraction of entries further apart than a tenth of the largest update, and by the set of entries that moved at all"""
    for k, v in mod.state_dict().items():
        if not k.endswith("embedder_obj.params"):
            continue
        t0 = torch.from_numpy(g[f"{prefix0}/{k}"]).double()
        d_ref = torch.from_numpy(g[f"{prefix}/{k}"]).double() - t0
        d_got = v.detach().cpu().double() - t0
        l2 = float((d_got - d_ref).norm() / d_ref.norm())
        far = float(((d_got - d_ref).abs() > 0.1 * d_ref.abs().max()).double().mean())
        moved = float(((d_got != 0) != (d_ref != 0)).double().mean())
        print(f"[tables {prefix}/{k}] update: relative L2 {l2:.3e}, further apart than 0.1 max|update| {far:.3e}, "
              f"moved in one run only {moved:.3e} (moved in the reference: {float((d_ref != 0).double().mean()):.3f})")
        assert l2 <= l2_bar and far <= far_bar and moved <= touched_bar, (prefix, k, l2, far, moved)


@pytest.mark.parametrize("case", ["stage_refine_dtu_dual", "stage_refine_eth3d_single"])
@pytest.mark.parametrize("capture", [False, True])
def test_refine_loop_vs_reference_loop(case, capture):
    g = load_golden(case)
    meta, opt, sdf, rad, ren, views, picks = _scene(g)
    o = meta["optim"]
    loop = stage.RefineLoop(opt, ren, sdf, rad, views, weights=meta["weights"], lr_sdf=o["lr_sdf"], lr_sdf_end=o["lr_sdf_end"],
                            lr_color=o["lr_color"], max_iter=o["max_iter"], rand_rays=meta["rand_rays"], capture=capture)
    logs = {k: v.cpu().numpy() for k, v in loop.run(picks=picks).items()}
    print(f"[{case} capture={capture}] loss {logs['all'][0]:.4f} -> {logs['all'][-1]:.4f} (reference {g['log/all'][0]:.4f} -> "
          f"{g['log/all'][-1]:.4f}); PSNR {logs['PSNR'][-1]:.4f} vs {g['log/PSNR'][-1]:.4f}")
    _close("loss.all", logs["all"], g["log/all"], 3e-3)
    _close("PSNR", logs["PSNR"], g["log/PSNR"], 3e-3)
    _close("rgb_loss", logs["rgb_loss"], g["log/rgb_loss"], 3e-3)
    _close("eikonal_loss", logs["eikonal_loss"], g["log/eikonal_loss"], 1e-2)
    # tracing terms: sums over a few dozen key points whose tracks end at the iteration cap on a still random-ish field
    _close("sdf_surf", logs["sdf_surf"], g["log/sdf_surf"], 2e-2, atol=2e-4)
    _close("tracing_loss", logs["tracing_loss"], g["log/tracing_loss"], 2e-2, atol=2e-4)
    _close("DC_loss", logs["DC_loss"], g["log/DC_loss"], 5e-2, atol=5e-4)
    _dense_close(sdf, g, "sdf_final")
    _dense_close(rad, g, "rad_final")
    _tables_close(sdf, g, "sdf0", "sdf_final", *TABLE_BARS["sdf_final"])
    _tables_close(rad, g, "rad0", "rad_final", *TABLE_BARS["rad_final"])


def test_captured_refine_loop_reproduces_the_eager_one_bit_for_bit():
    """a race detector for the captured step: its kernels run on three streams (tracing beside the render's forward, the depth
    branch and the weight-gradient chain beside the scatter) with the dependencies of a hipGraph only -- a missing edge or a
    block recycled while another stream still uses it shows up as a run-to-run difference (it did: tensors of the tracing call
    freed in Python ahead of the join)"""
    g = load_golden("stage_refine_dtu_dual")
    runs = []
    for capture in (False, True, True):
        meta, opt, sdf, rad, ren, views, picks = _scene(g)
        o = meta["optim"]
        loop = stage.RefineLoop(opt, ren, sdf, rad, views, weights=meta["weights"], lr_sdf=o["lr_sdf"], lr_sdf_end=o["lr_sdf_end"],
                                lr_color=o["lr_color"], max_iter=o["max_iter"], rand_rays=meta["rand_rays"], capture=capture)
        logs = loop.run(picks=picks)
        runs.append({k: v.cpu() for k, v in logs.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[1][k], runs[2][k]), k


def _synthetic_views(extent, H, W, n_kp, seed):
    """two cameras on the -z side of a [-extent, extent]^3 scene looking at its centre, smooth images inside (0.05, 0.95) (every
    ray is in mask_bg), random key points that observe random scene points"""
    import math
    gen = torch.Generator().manual_seed(seed)
    poses = []
    for ang in (-0.12, 0.15):
        c, s_ = math.cos(ang), math.sin(ang)
        R = torch.tensor([[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]])
        center = torch.tensor([2.5 * extent * math.sin(ang), 0.05 * extent, -2.5 * extent * math.cos(ang)])
        poses.append(torch.cat([R, (-R @ center).view(3, 1)], dim=1))          # world-to-camera [R | t]
    focal = 1.6 * W
    intr = torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, H / 2.0], [0.0, 0.0, 1.0]])
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    imgs = torch.stack([torch.stack([0.5 + 0.4 * torch.sin(3 * xx + v), 0.5 + 0.4 * torch.cos(2 * yy - v), 0.3 + 0.4 * xx * yy], dim=-1)
                        for v in range(2)]).reshape(2, H * W, 3).clamp(0.06, 0.94)
    kp = [torch.stack([torch.rand(n_kp, generator=gen) * (W - 1), torch.rand(n_kp, generator=gen) * (H - 1)], dim=-1) for _ in range(2)]
    ids = [torch.arange(n_kp) for _ in range(2)]
    xyzs = (torch.rand(n_kp, 3, generator=gen) - 0.5) * extent
    return stage.TrackedViews(torch.stack(poses).to(DEV), intr.to(DEV), imgs.to(DEV), [k.to(DEV) for k in kp], [t.to(DEV) for t in ids],
                              xyzs.to(DEV), H, W)


def test_full_size_refine_loop_captured_equals_eager():
    """The shipped grid size (L16 / F2 / T19, options/LevelS2fM.yaml:66-90) at the pipeline's 8192 rays over 2 views (:134), 128
    samples: five iterations of `RefineLoop` -- ray pick, key-point tracing consistency, render + tracing + losses, backward, Adam
    + schedule -- captured as one hipGraph reproduce the eager loop BIT FOR BIT (the goldens above use reduced grids; since the
    point-split coarse levels of the table scatter are combined in fixed point by a ticket instead of float atomics, the product
    repeats itself at this size too), stay finite and lower the loss."""
    from test_hip_fused_render import _randomized
    from ls2fm.options import make_options
    runs = []
    for capture in (False, True):
        opt = make_options("DTU", device=DEV, dual_field=True, sample_intvs=128)
        opt.Res = 100
        sdf, rad, ren = _randomized(opt, 5)
        assert sdf.embed_fn.embedder_obj.desc.n_levels == 16 and max(sdf.embed_fn.embedder_obj.desc.size[:16]) == 1 << 19
        views = _synthetic_views(1.0, 96, 128, 256, seed=9)
        w = dict(rgb=3, eikonal_loss=1, DC_Loss=0, tracing_loss=1, sdf_surf=1)
        loop = stage.RefineLoop(opt, ren, sdf, rad, views, weights=w, lr_sdf=1e-3, lr_sdf_end=5e-4, lr_color=1e-3, max_iter=5,
                                rand_rays=8192, capture=capture)
        gen = torch.Generator().manual_seed(17)
        picks = [(torch.randperm(96 * 128, generator=gen)[:4096].to(DEV), it % 2) for it in range(5)]
        logs = {k: v.cpu() for k, v in loop.run(picks=picks).items()}
        assert (loop.stage._graph is not None) == capture
        runs.append((logs, [p.detach().clone() for p in loop.stage.params]))
    (eager, p_e), (captured, p_c) = runs
    for k in eager:
        assert bool(torch.isfinite(eager[k]).all()), k
        assert torch.equal(eager[k], captured[k]), (k, eager[k], captured[k])
    for a, b in zip(p_e, p_c):
        assert torch.equal(a, b)
    assert float(eager["all"][-1]) < float(eager["all"][0])
    print(f"[full-size refine loop] loss {float(eager['all'][0]):.4f} -> {float(eager['all'][-1]):.4f}, PSNR {float(eager['PSNR'][-1]):.3f}")


@pytest.mark.parametrize("capture", [False, True])
def test_ba_loop_vs_reference_loop(capture):
    g = load_golden("stage_ba_dtu_dual")
    meta, opt, sdf, rad, ren, views, picks = _scene(g)
    o = meta["optim"]
    views.poses = torch.from_numpy(g["se3"]).to(DEV)            # the loop optimises the se(3) parameters
    loop = stage.BALoop(opt, ren, sdf, rad, views, weights=meta["weights"], lr_sdf=o["lr_sdf"], lr_sdf_end=o["lr_sdf_end"],
                        lr_color=o["lr_color"], lr_pose_r=o["lr_pose_r"], lr_pose_t=o["lr_pose_t"], max_iter=o["max_iter"],
                        rand_rays=meta["rand_rays"], capture=capture)
    logs = {k: v.cpu().numpy() for k, v in loop.run(picks=picks).items()}
    assert (loop.stage._graph is not None) == capture
    print(f"[ba capture={capture}] loss {logs['all'][0]:.4f} -> {logs['all'][-1]:.4f} (reference {g['log/all'][0]:.4f} -> {g['log/all'][-1]:.4f}); "
          f"reproj {logs['reproj_error'][0]:.4f} -> {logs['reproj_error'][-1]:.4f} (reference {g['log/reproj_error'][-1]:.4f})")
    assert np.array_equal(10.0 ** g["log/w_reproj"], logs["w_reproj"]), "adaptive re-projection weight (BA.py:163-166)"
    _close("loss.all", logs["all"], g["log/all"], 3e-3)
    _close("PSNR", logs["PSNR"], g["log/PSNR"], 3e-3)
    _close("reproj_error", logs["reproj_error"], g["log/reproj_error"], 1e-2)
    # the render poses go through SE(3) -> se(3) -> SE(3) here (the loop owns se(3) parameters): last-bit differences of that
    # round trip move the sample positions by ~1e-7, and the normal of a hash field amplifies a position change by the finest
    # level's scale -- already at iteration 0 the eikonal term (a mean of | |n| - 1 | over ~70 rays x 24 samples) differs by
    # ~1e-3 relative; it carries 10^2 of a total loss of ~480, which holds its 3e-3 bar above
    _close("eikonal_loss", logs["eikonal_loss"], g["log/eikonal_loss"], 3e-2)
    _close("sdf_surf", logs["sdf_surf"], g["log/sdf_surf"], 2e-2, atol=2e-4)
    _close("tracing_loss", logs["tracing_loss"], g["log/tracing_loss"], 2e-2, atol=2e-4)
    se3 = loop.poses_se3().cpu()
    ref = torch.from_numpy(g["se3_final"])
    assert float((se3 - ref).abs().max()) <= 2e-3 * float(ref.abs().max()), "poses after 20 Adam steps"
    xyz = loop.xyzs_all.cpu()
    # 20 successive projections p <- p - n / |n| sdf(p) (a Newton step on a still noisy field) amplify last-bit differences for the
    # points that sit where the field is rough (measured: most points agree to 1e-5, a handful drift by up to 2e-2): half of
    # the points within 2e-3 of the scene scale, 90 % within 1e-2, every point within 5e-2
    err = (xyz - torch.from_numpy(g["xyzs_final"])).norm(dim=-1)
    scale = float(np.abs(g["xyzs_final"]).max())
    assert float(err.median()) <= 2e-3 * scale and float(err.quantile(0.9)) <= 1e-2 * scale and float(err.max()) <= 5e-2 * scale, \
        (float(err.median()), float(err.quantile(0.9)), float(err.max()))
    assert torch.equal(views.xyzs.cpu(), torch.from_numpy(g["xyzs"])), "the point set itself does not move during the loop"
    _dense_close(sdf, g, "sdf_final")
    _dense_close(rad, g, "rad_final")
    _tables_close(sdf, g, "sdf0", "sdf_final", *TABLE_BARS["sdf_final"])
    _tables_close(rad, g, "rad0", "rad_final", *TABLE_BARS["rad_final"])


@pytest.mark.parametrize("capture", [False, True])
def test_init_loop_vs_reference_loop(capture):
    """`Initializer.run` (pipelines/Initialization.py:139-226), K = 20, and the two-view triangulation after it"""
    g = load_golden("stage_init_dtu_dual")
    meta, opt, sdf, rad, ren, views, picks = _scene(g)
    o = meta["optim"]
    inl = torch.from_numpy(g["inliers"]).to(DEV)
    m = torch.from_numpy(g["matches"].astype(np.int64)).to(DEV)
    kp = [views.keypoints[0][m[:, 0]][inl], views.keypoints[1][m[:, 1]][inl]]             # Camera.py:125, 176-177
    two = stage.TrackedViews(views.poses, views.intrinsic, views.images, kp, [torch.arange(k.shape[0], device=DEV) for k in kp],
                             torch.zeros(kp[0].shape[0], 3, device=DEV), views.H, views.W)
    loop = stage.InitLoop(opt, ren, sdf, rad, two, weights=meta["weights"], lr_sdf=o["lr_sdf"], lr_sdf_end=o["lr_sdf_end"],
                          lr_color=o["lr_color"], max_iter=o["max_iter"], rand_rays=meta["rand_rays"], capture=capture)
    logs = {k: v.cpu().numpy() for k, v in loop.run(picks=[p[0] for p in picks]).items()}
    print(f"[init capture={capture}] loss {logs['all'][0]:.4f} -> {logs['all'][-1]:.4f} (reference {g['log/all'][0]:.4f} -> "
          f"{g['log/all'][-1]:.4f}); reproj {logs['reproj_error'][-1]:.4f} vs {g['log/reproj_error'][-1]:.4f}")
    _close("loss.all", logs["all"], g["log/all"], 3e-3)
    _close("PSNR", logs["PSNR"], g["log/PSNR"], 3e-3)
    _close("rgb_loss", logs["rgb_loss"], g["log/rgb_loss"], 3e-3)
    _close("eikonal_loss", logs["eikonal_loss"], g["log/eikonal_loss"], 1e-2)
    _close("reproj_error", logs["reproj_error"], g["log/reproj_error"], 1e-2)
    _close("sdf_surf", logs["sdf_surf"], g["log/sdf_surf"], 2e-2, atol=2e-4)
    _close("DC_loss", logs["DC_loss"], g["log/DC_loss"], 5e-2, atol=5e-4)
    _dense_close(sdf, g, "sdf_final")
    _dense_close(rad, g, "rad_final")
    _tables_close(sdf, g, "sdf0", "sdf_final", *TABLE_BARS["sdf_final"])
    _tables_close(rad, g, "rad0", "rad_final", *TABLE_BARS["rad_final"])
    # the triangulation block (Initialization.py:182-213): which matches become 3-D points, and where
    pts, kept = loop.triangulate()
    ref_kept = torch.from_numpy(g["tri_kept"])[m[:, 0].cpu()][inl.cpu()]
    assert torch.equal(kept.cpu(), ref_kept), (kept.cpu().tolist(), ref_kept.tolist())
    ref_pts = torch.from_numpy(g["tri_xyzs"])
    err = (pts[kept].cpu() - ref_pts).norm(dim=-1)
    scale = float(ref_pts.abs().max())
    assert float(err.max()) <= 2e-3 * scale, (float(err.max()), scale)


def _geoinit_run(g, perturb=0.0, capture=False, n_iters=None):
    meta = json.loads(bytes(g["meta_json"]).decode())
    meta["bg_sdf"] = None
    opt = options_for(meta, DEV)
    opt.Res = meta["Res"]
    sdf = SDF(opt).to(DEV)
    sdf.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sdf0/")}, strict=True)
    if perturb:
        with torch.no_grad():
            for p in sdf.parameters():
                p.mul_(1 + perturb)
    kp = torch.from_numpy(g["kypts"]).to(DEV)
    inl = torch.from_numpy(g["inliers"]).to(DEV)
    n, n_exist = kp.shape[1], int(g["n_exist"])
    pid = torch.where(torch.arange(n, device=DEV) < n_exist, torch.arange(n, device=DEV), torch.full((n,), -1, device=DEV))
    pairs = [dict(view=v, kp_new=kp[2][inl], kp_src=kp[v][inl], point_id=pid[inl]) for v in (0, 1)]
    o = meta["optim"]
    loop = stage.GeoInitLoop(opt, sdf, torch.from_numpy(g["poses"]).to(DEV), torch.from_numpy(g["intrinsic"]).to(DEV), new_view=2,
                             pairs=pairs, xyzs=torch.from_numpy(g["xyzs"]).to(DEV), weights=meta["weights"], lr_sdf=o["lr_sdf"],
                             lr_sdf_end=o["lr_sdf_end"], max_iter=o["max_iter"], capture=capture)
    assert loop.n_iters == meta["iters"]
    draws = [torch.from_numpy(u).to(DEV) for u in g["sample_u"]]
    logs = {k: v.cpu().numpy().astype(np.float64) for k, v in loop.run(n_iters=n_iters, draws=draws).items()}
    return loop, sdf, logs, torch.arange(n)[inl.cpu()]


def test_geoinit_loop_vs_reference_loop():
    """`Registration.geo_init_nf` (pipelines/Registration.py:133-296): 20 iterations of the reference's loop for a new view against
    two registered ones (SDF field only; the `torch.rand_like` draw of sphere_tracing's sampled points replayed from the recording)
    and the triangulation block after it.

    This loop is CHAOTIC at the 1e-2 level (until round 4 not even the product repeated itself bit for bit from run to run: the
    point-split coarse levels of the table scatter were flushed with float atomics; they are now combined in fixed point, and the
    test below holds two runs of this loop to identical logs): its rays do not converge within
    iters_max trips on the still random-ish field, the eikonal term sits on random along-ray points whose range is the far
    tracer's end point, and the normal of a hash field amplifies position changes by the finest level's scale.  The first three
    iterations -- before Adam's g / sqrt(v) has fed differences back -- must match the reference tightly (3e-4 per term).  Over
    the whole run the bars are what the loop's own sensitivity allows: the test measures it (the same loop from weights perturbed
    by 1e-6 relative; printed, and required to be >= 5e-3 on the total -- if the loop ever stops being chaotic these bars are too
    loose) -- observed over repeated runs: own sensitivity 2.5e-2..3.6e-2 (total) / 7.5e-2 (eikonal), deviation from the
    reference 2.9e-2..3.7e-2 / 7.9e-2."""
    g = load_golden("stage_geoinit_dtu")
    loop, sdf, logs, kp_index = _geoinit_run(g)
    loop_pert, sdf_pert, pert, _ = _geoinit_run(g, perturb=1e-6)
    print(f"[geoinit] loss {logs['all'][0]:.4f} -> {logs['all'][-1]:.4f} (reference {g['log/all'][0]:.4f} -> {g['log/all'][-1]:.4f}); "
          f"reproj {logs['reproj_error'][-1]:.4f} vs {g['log/reproj_error'][-1]:.4f}")
    bars = dict(all=8e-2, reproj_error=6e-2, tracing_loss=6e-2, sdf_surf=6e-2, eikonal_loss=2e-1)
    for k, bar in bars.items():
        ref = g[f"log/{k}"]
        _close(f"{k} (first iterations)", logs[k][:3], ref[:3], 3e-4)
        dev = np.abs(logs[k] / ref - 1).max()
        env = np.abs(pert[k] / logs[k] - 1).max()
        print(f"   {k:14s} max deviation from the reference {dev:.2e}; own sensitivity to a 1e-6 perturbation {env:.2e}")
        assert dev <= bar, (k, dev, env)
        if k == "all":
            assert env >= 5e-3, ("the loop is no longer chaotic: tighten the bars", env)
    for k, v in sdf.state_dict().items():               # dense weights: 20 Adam steps of +-lr on near-zero gradients
        if k.endswith("embedder_obj.params"):
            continue
        ref = torch.from_numpy(g[f"sdf_final/{k}"])
        assert float((v.cpu() - ref).abs().max()) <= 0.25 * float(ref.abs().max()) + 1e-6, k
    # the block after the loop: per pair, which new matches become points (new-view key point indices) and where; after 20
    # chaotic iterations a match that sits on the threshold may fall on the other side (a few per pair), and the traced points
    # themselves have moved by ~1e-2 of the scene scale
    for pair, (pts, kept) in zip((0, 1), loop.triangulate()):
        sel = g["tri_src_view"] == pair
        got, want = set(kp_index[kept.cpu()].tolist()), set(g["tri_kp_new"][sel].tolist())
        assert len(got ^ want) <= 3, (pair, sorted(got), sorted(want))
        both = sorted(got & want)
        ref = torch.from_numpy(g["tri_xyzs"][sel])[[list(g["tri_kp_new"][sel]).index(k) for k in both]]
        mine = pts.cpu()[[kp_index.tolist().index(k) for k in both]]
        err = (mine - ref).norm(dim=-1)
        scale = float(ref.abs().max())
        assert float(err.median()) <= 2e-2 * scale and float(err.max()) <= 1e-1 * scale, (pair, float(err.median()), float(err.max()))


def test_geoinit_loop_repeats_itself_bit_for_bit():
    """the product's own determinism on the loop that exposes it most (chaotic after three iterations): two runs from the same
    state and draws give IDENTICAL per-iteration terms and final weights -- every table-gradient entry is an exactly rounded,
    order-independent sum (csrc/bin_scatter.hip; ls2fm_set_scatter_mode(1), the default)"""
    g = load_golden("stage_geoinit_dtu")
    torch.manual_seed(7)                       # (the loop's own random pick of track points: same draws in both runs)
    _, sdf_a, logs_a, _ = _geoinit_run(g)
    torch.manual_seed(7)
    _, sdf_b, logs_b, _ = _geoinit_run(g)
    for k in logs_a:
        assert np.array_equal(logs_a[k], logs_b[k]), k
    for (k, va), vb in zip(sdf_a.state_dict().items(), sdf_b.state_dict().values()):
        assert torch.equal(va, vb), k


def test_captured_geoinit_loop_vs_reference_loop():
    """`GeoInitLoop(capture=True)`: the whole `geo_init_nf` iteration as ONE hipGraph (tracing, fixed-shape sample points + mask,
    the three point-query nodes, every term, backward, Adam + schedule on the device), the iteration's uniform draws written into
    a persistent buffer before each replay.  Held to the reference's own loop at the bar of the eager form's first iterations
    (3e-4 per term -- afterwards the loop is chaotic, see above) and, over the whole run, to the eager form's bars."""
    g = load_golden("stage_geoinit_dtu")
    loop, sdf, logs, _ = _geoinit_run(g, capture=True)
    assert loop._graph is not None
    _, _, eager, _ = _geoinit_run(g, n_iters=3)
    bars = dict(all=8e-2, reproj_error=6e-2, tracing_loss=6e-2, sdf_surf=6e-2, eikonal_loss=2e-1)
    for k, bar in bars.items():
        ref = g[f"log/{k}"]
        _close(f"{k} (first iterations, captured)", logs[k][:3], ref[:3], 3e-4)
        _close(f"{k} (captured vs eager)", logs[k][:3], eager[k][:3], 3e-4)
        assert np.isfinite(logs[k]).all()
        assert np.abs(logs[k] / ref - 1).max() <= bar, k
    stepped = [int(st["step"]) for st in loop.optim.state.values() if st]
    assert stepped and all(n == loop.n_iters for n in stepped)
    assert len(loop.triangulate()) == 2


def test_static_sphere_tracing_samples_have_the_reference_structure():
    """`sampled_pts` of SDF.sphere_tracing (SDF.py:216-224) in the capturable form: fixed shape + device mask; the masked rows
    are exactly what the synchronising form returns for the same draws' structure: track points of <= 4096 random rays (first K
    columns), then one point per ray between near and min(1.5 t_end, far)."""
    g = load_golden("stage_refine_eth3d_single")
    meta, opt, sdf, rad, ren, views, picks = _scene(g)
    centers, rays, _ = stage.loops._pick_rays(views, views.poses, picks[0][0])
    o, d = centers.reshape(1, -1, 3), rays.reshape(1, -1, 3)
    n_rays, it = o.shape[1], int(sdf.iters_max)
    d_a, last_a, samp, fin_a = sdf.sphere_tracing(o, d, sdf, static_trips=True, want_samples=True)
    mask = sdf.last_sample_mask
    k = int(sdf.last_trips.item())
    assert samp.shape == (1, min(4096, n_rays) * it + n_rays, 3) and mask.shape == (samp.shape[1],)
    assert int(mask.sum()) == min(4096, n_rays) * max(k, 1) + n_rays
    d_b, last_b, samp_b, fin_b = sdf.sphere_tracing(o, d, sdf)
    assert samp_b.shape[1] == int(mask.sum())                              # the reference's (K-dependent) shape
    assert torch.allclose(d_a, d_b, rtol=1e-5, atol=1e-6) and torch.equal(fin_a, fin_b)
    # the along-ray samples lie on their rays, inside [near, far]
    from ls2fm import fused
    near, far, _, _, _ = fused.sphere_trace(sdf, o[0], d[0], sync=False)
    tail = samp[0, -n_rays:]
    t = ((tail - o[0]) * d[0]).sum(-1) / (d[0] * d[0]).sum(-1)
    hit = far > 0
    assert bool(((t >= near - 1e-4) & (t <= far + 1e-4))[hit].all())
    assert torch.allclose(o[0] + t[:, None] * d[0], tail, atol=1e-4 * float(far.abs().max() + 1))


def test_geo_init_shaped_step_is_capturable():
    """The step of `geo_init_nf` (pipelines/Registration.py:188-277) on this path -- sphere tracing of key-point rays, eikonal on
    the tracing's sample points (`sdf_func.gradient(sample_pts).norm()`, :202), sdf_surf on the track ends, the tracing
    distance to existing points -- as ONE hipGraph: eager steps and replays of the captured step walk the same trajectory."""
    from ls2fm.graph import CapturedStep
    from ls2fm.optim import FusedAdam
    g = load_golden("stage_refine_dtu_dual")

    def build():
        meta, opt, sdf, rad, ren, views, picks = _scene(g)
        c, r = stage.keypoint_rays(views.poses[0], views.intrinsic, views.kp_pad[0])
        target = views.xyzs[views.id_pad[0]]
        optim = FusedAdam(list(sdf.parameters()), lr=1e-3, scheduled_gamma=0.99)
        gen_state = torch.cuda.get_rng_state()

        def step():
            for p in sdf.parameters():
                p.grad = None
            d, sdf_surf, samples, _ = sdf.sphere_tracing(c, r, sdf, static_trips=True, want_samples=True)
            w = sdf.last_sample_mask.float()
            grad_norm = sdf.gradient(samples[0].clone()).norm(dim=-1)
            eik = ((grad_norm - 1).abs() * w).sum() / w.sum()
            surface = c[0] + r[0] * d.reshape(-1, 1)
            loss = 10.0 * (target - surface).norm(dim=-1).mean() + 100.0 * sdf_surf.abs().mean() + 100.0 * eik
            loss.backward()
            optim.step()
            return loss.detach()
        return sdf, optim, step, gen_state

    sdf_a, _, step_a, _ = build()
    torch.manual_seed(3)
    eager = [float(step_a()) for _ in range(4)]
    sdf_b, optim_b, step_b, _ = build()
    snap = [p.detach().clone() for p in sdf_b.parameters()]
    cap = CapturedStep(step_b, params=list(sdf_b.parameters()), warmup=2)
    with torch.no_grad():                      # undo the warm-up / capture steps, restart the schedule
        for p, q in zip(sdf_b.parameters(), snap):
            p.copy_(q)
        for st in optim_b.state.values():
            st["step"] = 0; st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        for t in optim_b._sched.values():
            t.copy_(torch.tensor([0.0, 1e-3, 0.99, 0.0], dtype=torch.float64))
    torch.manual_seed(3)                       # a replay takes its Philox offsets from the generator's state, as an eager step does
    replayed = [float(cap.replay()) for _ in range(4)]
    print(f"[geo-init step] eager {eager} replayed {replayed}")
    assert np.isfinite(replayed).all() and replayed[-1] < replayed[0]
    # same seed, same number of draws per step: the replays see the eager run's sample points
    np.testing.assert_allclose(replayed, eager, rtol=2e-3)


def test_pass_gradient_sharing_gives_the_same_gradients():
    """one gradient buffer per backward pass (ls2fm.fused.pass_gradient_sharing): point-query nodes issued AHEAD of the render add
    into the render's buffer in its wake -- every parameter gradient of a BA-shaped step equals the one autograd sums from separate
    buffers (LS2FM_SHARE_GRADS=0 semantics), to summation-order round-off"""
    from ls2fm import fused
    g = load_golden("stage_ba_dtu_dual")
    out = []
    for share in (False, True):
        meta, opt, sdf, rad, ren, views, picks = _scene(g)
        o = meta["optim"]
        views.poses = torch.from_numpy(g["se3"]).to(DEV)
        loop = stage.BALoop(opt, ren, sdf, rad, views, weights=meta["weights"], lr_sdf=o["lr_sdf"], lr_sdf_end=o["lr_sdf_end"],
                            lr_color=o["lr_color"], lr_pose_r=o["lr_pose_r"], lr_pose_t=o["lr_pose_t"], max_iter=o["max_iter"],
                            rand_rays=meta["rand_rays"])
        loop.stage.share_gradients = share
        loop.stage.optim.step = lambda: None                     # keep the gradients: no update
        loop.step(*picks[0])
        out.append({n: p.grad.detach().clone() for n, p in list(sdf.named_parameters()) + [("rot", loop.rot), ("trans", loop.trans)]
                    if p.grad is not None})
    assert out[0].keys() == out[1].keys()
    for n in out[0]:
        scale = float(out[0][n].abs().max()) + 1e-20
        assert float((out[0][n] - out[1][n]).abs().max()) <= 2e-5 * scale, n
