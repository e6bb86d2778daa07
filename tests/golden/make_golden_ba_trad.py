#!/usr/bin/env python
"""Golden vectors of the CLASSICAL bundle adjustment (`pipelines/BA_Trad.py`: `BA.run_ba`, the loop behind `Ablate_config.ba_trad`):
the REFERENCE's own `BA_Trad.BA`, driven through the reference's own `CameraSet` / `Point3DSet`, `torch.optim.Adam` and
`ExponentialLR`, imported from the reference tree where it lies.  Build container only (stubs as in make_golden_stage.py).

    python tests/golden/make_golden_ba_trad.py [case ...]   ->  tests/golden/stage_ba_trad_<case>.npz   (data only)

Every case is run TWICE: as the reference runs it (fp32), and with every tensor in fp64 (default dtype float64, the same input
values).  The distance between the two trajectories is the yardstick of every tolerance in tests/test_bundle_adjust_host.py and
tests/test_hip_bundle_adjust.py: it is printed here and stored in the fixture as `gap/<quantity>`.

  local    3 picked views of 6 (cam_pick [4, 1, 3]: not sorted), ~10^3 observations, 20 iterations: points seen once, points
           seen from all three picked views, unpicked points, key points without a 3-D point
  global   all 6 views, 20 iterations
  single   one picked camera: max_iter is halved (10 iterations), which changes gamma
  heavy    a large initial error: reproj > 10 for the first iterations, below 10 inside the window -- both weights and the switch
  long     the `global` scene for 1000 iterations: log and final state only

Recorded: the scene (se3 of every view, K, per view the key points and idx2d_to_3d with its -1 entries, all points), cam_pick,
the observation list of `util.get_idx3d_camset` as the loop holds it, per iteration reproj_loss / weight / mean(err), the final
r, t and points (the STEPPED state: the parameters after the last Adam step), and what the loop writes back after its last
iteration (`se3_refine`, `xyzs_forward` and the returned mean(err): the state that ENTERED the last iteration).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_VIEWS, N_POINTS, H, W = 6, 400, 480, 640
OPTIM_BA = dict(lr_sdf=1e-4, lr_sdf_end=5e-5, lr_pose=1e-2, lr_pose_end=5e-3, lr_pose_r=5e-3, lr_pose_t=1e-2)     # LevelS2fM.yaml
LR_XYZS = 1e-2
CASES = [
    # name, cam_pick, optim.ba.max_iter, initial noise: rotations (rad), translations, points (scene units)
    ("local", [4, 1, 3], 20, 0.004, 0.02, 0.02),
    ("global", None, 20, 0.004, 0.02, 0.02),
    ("single", [2], 20, 0.004, 0.02, 0.02),
    ("heavy", None, 20, 0.030, 0.10, 0.02),
    ("long", None, 1000, 0.004, 0.02, 0.02),
]


def scene(seed, rot_noise, trans_noise, point_noise, ref_camera):
    """6 views on an arc looking at a blob of 400 points; key points = projections + 1 px noise; initial poses and points are
    the true ones perturbed.  Visibility is random per (view, point) with a few points forced to a single view / to all views;
    every view also carries key points that have no 3-D point (idx2d_to_3d == -1)."""
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand(N_POINTS, 3, generator=gen) * 2 - 1) * torch.tensor([1.5, 1.0, 1.0])
    poses = []
    for v in range(N_VIEWS):
        ang = -0.5 + 0.2 * v
        eye = torch.tensor([5.0 * np.sin(ang), 0.3 * (v % 2), -5.0 * np.cos(ang)], dtype=torch.float32)
        fwd = -eye / eye.norm()
        up = torch.tensor([0.0, 1.0, 0.0])
        right = torch.linalg.cross(up, fwd); right = right / right.norm()
        up2 = torch.linalg.cross(fwd, right)
        R = torch.stack([right, up2, fwd], dim=0)
        poses.append(torch.cat([R, (-R @ eye)[:, None]], dim=1))
    poses = torch.stack(poses)
    intr = torch.tensor([[520.0, 0.0, W / 2], [0.0, 520.0, H / 2], [0.0, 0.0, 1.0]])
    se3_true = ref_camera.lie.SE3_to_se3(poses)
    noise = torch.cat([rot_noise * torch.randn(N_VIEWS, 3, generator=gen), trans_noise * torch.randn(N_VIEWS, 3, generator=gen)], dim=1)
    se3 = (se3_true + noise).float()
    vis = torch.rand(N_VIEWS, N_POINTS, generator=gen) < 0.8
    vis[:, :20] = False
    for j in range(20):                       # points 0..19: seen from exactly one view
        vis[j % N_VIEWS, j] = True
    vis[:, 20:60] = True                      # points 20..59: seen from every view
    kypts, idx = [], []
    for v in range(N_VIEWS):
        ids = torch.nonzero(vis[v])[:, 0]
        ids = ids[torch.randperm(ids.shape[0], generator=gen)]           # a view's key points are in no particular point order
        cam = pts[ids] @ poses[v, :, :3].T + poses[v, :, 3]
        uv = cam @ intr.T
        uv = uv[:, :2] / uv[:, 2:] + 1.0 * torch.randn(ids.shape[0], 2, generator=gen)
        n_free = 15                                                       # key points without a 3-D point, interleaved
        free = torch.stack([torch.rand(n_free, generator=gen) * W, torch.rand(n_free, generator=gen) * H], dim=-1)
        kp = torch.cat([uv, free])
        id_all = torch.cat([ids, torch.full((n_free,), -1, dtype=torch.long)])
        perm = torch.randperm(kp.shape[0], generator=gen)
        kypts.append(kp[perm].float())
        idx.append(id_all[perm].numpy().astype(np.int64))
    xyzs = (pts + point_noise * torch.randn(N_POINTS, 3, generator=gen)).float()
    return dict(se3=se3, intr=intr, kypts=kypts, idx=idx, xyzs=xyzs)


def run_reference(MG, RefCamera, RefPoint3D, RefBATrad, sc, cam_pick, max_iter, dtype):
    """one run of the reference's loop in `dtype` -> dict of recorded arrays (float64 numpy)"""
    torch.set_default_dtype(dtype)
    try:
        hash_json = MG.write_hash_json(4, 10)
        opt = MG.make_opt("DTU", hash_json, False, 8)
        os.unlink(hash_json)
        opt.H, opt.W = H, W
        opt.data.image_size = [H, W]
        opt.camera = MG.AttrDict(model="perspective")
        opt.Renderer = MG.AttrDict(rand_rays=64)
        opt.optim = MG.AttrDict(json.loads(json.dumps(dict(algo="Adam", sched=dict(type="ExponentialLR"), lr_xyzs=LR_XYZS,
                                                          ba=dict(max_iter=max_iter, **OPTIM_BA)))))
        opt.loss_weight = MG.AttrDict(dict(ba=dict(reproj_error=0)))
        cset = RefCamera.CameraSet(opt)
        pset = RefPoint3D.Point3DSet(opt)
        intr = sc["intr"].to(dtype)
        for v in range(N_VIEWS):
            cset.add_camera(id=v, img_gt=torch.zeros(3, 1, 1), kypts2D=sc["kypts"][v].to(dtype), pose_gt=None, Match_mask=None,
                            Inlier_mask=None, Intrinsic=intr, Extrinsic=sc["se3"][v:v + 1].to(dtype), idx2d_to_3d=sc["idx"][v].copy())
        tracks = [[] for _ in range(N_POINTS)]
        for v in range(N_VIEWS):
            for k, j in enumerate(sc["idx"][v]):
                if j >= 0:
                    tracks[j].append((v, k))
        for j in range(N_POINTS):
            pset.add_point3d(sc["xyzs"][j:j + 1].to(dtype).clone(), tracks[j])
        # instance-level wrappers (the loop code itself is the reference's): the constructor's render-data pick reads the fields,
        # which this loop never uses; the write-back and the loss lines are logged
        cset.get_ren_data = lambda *a, **kw: (None, None, None)
        wrote = {}
        pset.update_xyzs = lambda idxs, xyzs_new: wrote.update(ids=np.asarray(idxs).copy(), xyzs=xyzs_new.detach().clone())
        stage = RefBATrad.BA(opt, cset, pset, None, None, cam_pick_ids=None if cam_pick is None else list(cam_pick))
        log = dict(reproj=[], weight=[], err_mean=[])
        ref_cam = RefBATrad.camera
        summarize_orig = stage.summarize_loss

        def summarize_logged(o, loss):
            log["weight"].append(10.0 ** float(o.loss_weight.ba.reproj_error))
            log["reproj"].append(float(loss["reproj_error"].detach().double()))
            # `reproj_loss_tem` (BA_Trad.py:108) is a local of the loop: the same expression on the state the iteration holds (the
            # parameters are not stepped yet), with the reference's own projection functions
            with torch.no_grad():
                x = stage.xyzs_all[stage.pts_pick_ids]
                cam = RefBATrad.world2cam(x.unsqueeze(1), ref_cam.lie.se3_to_SE3(stage.se3_refine[stage.pose_idx]))
                uv = RefBATrad.cam2img(cam, cset.cameras[0].intrinsic.repeat(cam.shape[0], 1, 1))
                uv = (uv / (uv[..., 2:] + RefBATrad.epsilon))[..., :2].squeeze(1)
                log["err_mean"].append(float(torch.norm(uv - stage.kypts2D_forward, dim=-1).mean().double()))
            return summarize_orig(o, loss)
        stage.summarize_loss = summarize_logged
        ret = stage.run_ba(None, None, None)
        assert len(log["reproj"]) == stage.max_iter
        out = dict(reproj=np.asarray(log["reproj"], np.float64), weight=np.asarray(log["weight"], np.float64),
                   err_mean=np.asarray(log["err_mean"], np.float64),
                   r_final=stage.r_paras().detach().double().numpy(), t_final=stage.t_paras().detach().double().numpy(),
                   xyzs_final=stage.xyzs_paras().detach().double().numpy(),
                   se3_written=torch.cat([cset(c).se3_refine.data for c in stage.cam_pick_ids]).detach().double().numpy(),
                   xyzs_written=wrote["xyzs"].double().numpy(), err_returned=np.float64(float(ret)),
                   obs_point=np.asarray(stage.pts_pick_ids, np.int64), obs_view=np.asarray(stage.pose_idx, np.int64),
                   obs_uv=stage.kypts2D_forward.detach().double().numpy(), cam_pick=np.asarray(stage.cam_pick_ids, np.int64),
                   max_iter=np.int64(stage.max_iter))
        assert (wrote["ids"] == out["obs_point"]).all()
        return out
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    import make_golden_caller as MC
    MG, _SDF, _RadF, _Renderer, RefCamera, _RefBA = MC.import_reference_pipelines()
    from pipelines import BA_Trad as RefBATrad
    from pipelines import Point3D as RefPoint3D
    import utils.camera as ref_camera

    only = set(sys.argv[1:])
    for ci, (name, cam_pick, max_iter, rot_noise, trans_noise, point_noise) in enumerate(CASES):
        if only and name not in only:
            continue
        seed = 4100 + (1 if name == "long" else ci)               # `long` runs the `global` scene
        sc = scene(seed, rot_noise, trans_noise, point_noise, ref_camera)
        r32 = run_reference(MG, RefCamera, RefPoint3D, RefBATrad, sc, cam_pick, max_iter, torch.float32)
        r64 = run_reference(MG, RefCamera, RefPoint3D, RefBATrad, sc, cam_pick, max_iter, torch.float64)
        for k in ("obs_point", "obs_view", "cam_pick", "weight"):
            assert (r32[k] == r64[k]).all(), f"{name}: fp32 and fp64 runs disagree on {k}"
        # ---- the yardstick: fp32 against fp64, per quantity (absolute, max over elements; the log relative to the fp64 value)
        gap = dict(reproj=float(np.max(np.abs(r32["reproj"] - r64["reproj"]) / np.abs(r64["reproj"]))),
                   err_mean=float(np.max(np.abs(r32["err_mean"] - r64["err_mean"]) / np.abs(r64["err_mean"]))),
                   err_returned=float(abs(r32["err_returned"] - r64["err_returned"]) / abs(r64["err_returned"])),
                   se3_final=float(max(np.abs(r32["r_final"] - r64["r_final"]).max(), np.abs(r32["t_final"] - r64["t_final"]).max())),
                   xyzs_final=float(np.abs(r32["xyzs_final"] - r64["xyzs_final"]).max()),
                   se3_written=float(np.abs(r32["se3_written"] - r64["se3_written"]).max()),
                   xyzs_written=float(np.abs(r32["xyzs_written"] - r64["xyzs_written"]).max()))
        n_iter = int(r32["max_iter"])
        print(f"{name}: {len(r32['obs_point'])} observations, {n_iter} iterations, weights {sorted(set(r32['weight'].tolist()))}, "
              f"reproj {r32['reproj'][0]:.4f} -> {r32['reproj'][-1]:.4f}, returned mean err {float(r32['err_returned']):.4f}")
        print("   fp32-vs-fp64 gap: " + ", ".join(f"{k} {v:.3e}" for k, v in gap.items()))
        if name == "heavy":
            w = r32["weight"]
            assert w[0] == 10.0 and w[-1] == 1.0, f"heavy: the weight switch is not inside the window: {w}"
            margin = float(np.min(np.abs(r64["reproj"] - 10.0)))
            print(f"   heavy: switch at iteration {int(np.argmax(w == 1.0))}, closest recorded loss to 10: {margin:.4f} away")
            assert margin > 100 * gap["reproj"] * 10.0, "heavy: a recorded loss lies within the fp32 gap of the threshold"
        out = {"se3": sc["se3"].numpy(), "intrinsic": sc["intr"].numpy(), "xyzs": sc["xyzs"].numpy(),
               "kypts": np.concatenate([k.numpy() for k in sc["kypts"]]), "idx2d_to_3d": np.concatenate(sc["idx"]),
               "kypts_start": np.cumsum([0] + [k.shape[0] for k in sc["kypts"]]).astype(np.int64),
               "cam_pick": r32["cam_pick"], "cam_pick_given": np.asarray([-1] if cam_pick is None else cam_pick, np.int64),
               "obs_point": r32["obs_point"], "obs_view": r32["obs_view"], "obs_uv": r32["obs_uv"].astype(np.float32)}
        for tag, r in (("f32", r32), ("f64", r64)):
            for k in ("reproj", "weight", "err_mean", "r_final", "t_final", "xyzs_final", "se3_written", "xyzs_written", "err_returned"):
                out[f"{tag}/{k}"] = r[k]
        for k, v in gap.items():
            out[f"gap/{k}"] = np.float64(v)
        meta = dict(case=name, max_iter_opt=max_iter, iters=n_iter, lr_xyzs=LR_XYZS, optim=OPTIM_BA, H=H, W=W)
        out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(HERE, f"stage_ba_trad_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"   {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
