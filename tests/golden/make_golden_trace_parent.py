#!/usr/bin/env python
"""Record tests/golden/trace_parent.json: every output of ls2fm_sphere_trace, ls2fm_trace_image, ls2fm_sdf_eval (its five launch
choices), ls2fm_sdf_eval_prepared and ls2fm_sdf_volume on an MI355X, for tests/test_hip_trace_bits.py.  Run it with the library
whose bits are to be kept (LS2FM_LIB names another build than the tree's).  Inputs come from seeded CPU generators, so they are
the same everywhere; the outputs of a call over at most WHOLE rays or points are stored whole (the hex of their bytes), those of a
larger call as shape, dtype and the SHA-256 of their bytes.
    python tests/golden/make_golden_trace_parent.py [--out tests/golden]"""
import argparse
import ctypes
import functools
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "level-s2fm_official_amd")]

from ls2fm import _lib, fused, image  # noqa: E402
from ls2fm._lib import check, ptr, stream_ptr  # noqa: E402
from ls2fm.models.SDF import SDF  # noqa: E402
from ls2fm.options import make_options  # noqa: E402
from ls2fm.utils import camera as cam  # noqa: E402

DEV = "cuda:0"
WHOLE = 64
# wave kernel: one workgroup, and the last shape it serves; wide: a last workgroup of one live ray and seven clamped ones, and its last
# shape; narrow: an odd count, the last wave half live
RAY_COUNTS = (1, 2048, 2049, 20000, 20001)
FIELDS = ("levels16", "levels8_bg_outside")
TRACE_CASES = [(f, n, it) for f in FIELDS for n in RAY_COUNTS for it in ("default", 0)]
POINT_CASES = ["sdf", "sdf_feat_wide", "sdf_feat_normal_wide", "thread_per_point", "thread_per_point_normal", "prepared", "volume"]
IMAGE_CASES = ["two_views_7x5", "one_view_1x1", "two_views_7x5_all_converged"]


@functools.lru_cache(maxsize=None)
def field(name):
    """levels16: the DTU preset (inside), 16 levels.  levels8_bg_outside: the ETH3D preset (inside = False), 8 levels, and the background
    sphere switched on in the descriptor (the Python front end only offers it with inside = True).  Random tables and first-layer
    encoding weights: the field does not converge, ends cross and keep stepping on stale values"""
    ds, levels, seed = ("DTU", 16, 31) if name == "levels16" else ("ETH3D", 8, 37)
    enc = dict(n_levels=levels, n_features_per_level=2, log2_hashmap_size=15, base_resolution=16)
    opt = make_options(ds, device=DEV, dual_field=True, hash_encoding=enc)
    torch.manual_seed(seed)
    sdf = SDF(opt).to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    w_std = 0.05 if name == "levels16" else 0.004          # the second field is near the geometric initialisation: ends converge
    with torch.no_grad():
        for pname, p in sdf.named_parameters():
            if pname.endswith("embedder_obj.params"):
                p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1).to(DEV))
            if pname.endswith("mlp.0.weight_v"):
                p[:, 3:] = (torch.randn(p[:, 3:].shape, generator=gen) * w_std).to(DEV)
    fdesc = fused.field_desc(opt)
    if name != "levels16":
        fdesc.bg_sdf, fdesc.inside = 1, 0
        fdesc.bg_rad = 1.2 * float(opt.data.bound_max[0])
    return sdf, fdesc


def rays(n, s, seed):
    """tests/test_hip_sphere_trace_parity.py::_rays' seeded family: eight misses and eight origins inside the box where n allows"""
    gen = torch.Generator().manual_seed(seed)
    c = torch.tensor([0.0, 0.0, -2.5 * s]).repeat(n, 1) + 0.05 * s * torch.randn(n, 3, generator=gen)
    d = torch.tensor([0.0, 0.0, 1.0]).repeat(n, 1) + 0.15 * torch.randn(n, 3, generator=gen)
    if n >= 16:
        d[:8] = torch.tensor([0.0, 1.0, -0.2]) + 0.05 * torch.randn(8, 3, generator=gen)
        c[8:16] = 0.3 * s * torch.randn(8, 3, generator=gen)
    return c.float().contiguous().to(DEV), d.float().contiguous().to(DEV)


def _call_args(sdf, fdesc):
    keep, pstruct = fused._sdf_only_params(sdf)
    return keep, pstruct, ctypes.byref(fdesc), ctypes.byref(sdf.embed_fn.embedder_obj.desc)


def sphere_trace(sdf, fdesc, o, d, iters_max):
    """ls2fm_sphere_trace with all five outputs -> near, far, track, t_end, track_sdf, trips and the workspace it packed"""
    lib = _lib.load()
    n, it = o.shape[0], int(iters_max)
    near, far = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    track = torch.empty(n, it + 1, 3, device=DEV)
    t_end, track_sdf = torch.empty(n, it + 1, device=DEV), torch.empty(n, it + 1, device=DEV)
    trips = torch.empty(1, device=DEV, dtype=torch.int32)
    ws = fused._sdf_workspace(DEV)
    keep, pstruct, f, g = _call_args(sdf, fdesc)
    check(lib.ls2fm_sphere_trace(f, g, ctypes.byref(pstruct), ptr(o), ptr(d), n, float(sdf.sdf_threshold), it, ptr(near), ptr(far),
                                 ptr(track), ptr(t_end), ptr(track_sdf), ptr(trips), ptr(ws), stream_ptr()), "ls2fm_sphere_trace")
    torch.cuda.synchronize()
    return dict(near=near, far=far, track=track, t_end=t_end, track_sdf=track_sdf, trips=trips), ws


def sdf_eval(sdf, fdesc, p, want_feat, want_normal, prepared_ws=None):
    lib = _lib.load()
    n = p.shape[0]
    out = dict(sdf=torch.empty(n, device=DEV))
    if want_feat:
        out["feat"] = torch.empty(n, _lib.FEAT + 1, device=DEV)
    if want_normal:
        out["normal"] = torch.empty(n, 3, device=DEV)
    keep, pstruct, f, g = _call_args(sdf, fdesc)
    if prepared_ws is not None:
        check(lib.ls2fm_sdf_eval_prepared(f, g, ctypes.byref(pstruct), ptr(p), n, ptr(out["sdf"]), ptr(prepared_ws), stream_ptr()),
              "ls2fm_sdf_eval_prepared")
    else:
        ws = fused._sdf_workspace(DEV)
        check(lib.ls2fm_sdf_eval(f, g, ctypes.byref(pstruct), ptr(p), n, ptr(out["sdf"]), ptr(out.get("feat")), ptr(out.get("normal")),
                                 ptr(ws), stream_ptr()), "ls2fm_sdf_eval")
    torch.cuda.synchronize()
    return out


def run_trace(name, n, it):
    sdf, fdesc = field(name)
    s = float(sdf.opt.data.bound_max[0])
    o, d = rays(n, s, seed=100 + n % 97)
    out, _ = sphere_trace(sdf, fdesc, o, d, sdf.iters_max if it == "default" else it)
    return out


def points17(sdf):
    """17 points: one full 16-lane group row and a partial one; the first three outside the box, beyond the background sphere"""
    s = float(sdf.opt.data.bound_max[0])
    gen = torch.Generator().manual_seed(41)
    p = (torch.rand(17, 3, generator=gen) * 2 - 1) * s
    p[:3] *= 1.3
    return p.float().contiguous().to(DEV)


def run_points(which):
    """the five launch choices of ls2fm_sdf_eval (LS2FM_POINTS_KERNEL is read per call), on both fields; the prepared call after a
    trace; the lattice sweep with both index arithmetics"""
    out = {}
    for name in FIELDS:
        sdf, fdesc = field(name)
        p = points17(sdf)
        if which == "volume":
            s = float(sdf.opt.data.bound_max[0])
            if name == "levels16":
                for ref in (0, 1):
                    out[f"ref_indexing{ref}"] = fused.sdf_volume(sdf, 5, [0.45 * s] * 3, [-0.9 * s] * 3, reference_indexing=bool(ref))
            continue
        if which == "prepared":
            o, d = rays(16, float(sdf.opt.data.bound_max[0]), seed=7)
            _, ws = sphere_trace(sdf, fdesc, o, d, 2)
            got = sdf_eval(sdf, fdesc, p, False, False, prepared_ws=ws)
        else:
            feat, normal, force = dict(sdf=(False, False, None), sdf_feat_wide=(True, False, "2"), sdf_feat_normal_wide=(True, True, "2"),
                                       thread_per_point=(True, False, "1"), thread_per_point_normal=(True, True, "1"))[which]
            before = os.environ.pop("LS2FM_POINTS_KERNEL", None)
            try:
                if force:
                    os.environ["LS2FM_POINTS_KERNEL"] = force
                got = sdf_eval(sdf, fdesc, p, feat, normal)
            finally:
                os.environ.pop("LS2FM_POINTS_KERNEL", None)
                if before is not None:
                    os.environ["LS2FM_POINTS_KERNEL"] = before
        out.update({f"{name}/{k}": v for k, v in got.items()})
    torch.cuda.synchronize()
    return out


def views(opt, H, W, V, seed, away=()):
    """tests/test_hip_trace_image.py::_views: poses looking at the box from 4 half-sizes away, those in `away` turned round"""
    h = float(opt.data.bound_max[0])
    g = torch.Generator().manual_seed(seed)
    se3 = torch.cat([0.15 * torch.randn(V, 3, generator=g), 0.1 * h * torch.randn(V, 3, generator=g)], dim=1)
    se3[:, 5] += 4.0 * h
    for v in away:
        se3[v, 1] += np.pi
    poses = cam.lie.se3_to_SE3(se3.to(DEV)).contiguous()
    intr = torch.tensor([[1.0 * W, 0.0, W / 2.0], [0.0, 1.0 * W, H / 2.0], [0.0, 0.0, 1.0]], device=DEV)
    return poses, intr


def run_image(which):
    """two views of 7 x 5 pixels (70 rays: the view boundary falls inside a wave), the second turned away so the trip counts differ;
    one view of one pixel; and the two views with a threshold above every value, so K = 0"""
    sdf, _ = field("levels16")
    H, W, V = (1, 1, 1) if which == "one_view_1x1" else (5, 7, 2)
    poses, intr = views(sdf.opt, H, W, V, seed=3, away=(1,) if V == 2 else ())
    thr = sdf.sdf_threshold
    try:
        if which == "two_views_7x5_all_converged":
            sdf.sdf_threshold = 1e9
        t = image.trace_image(sdf, poses, intr, H=H, W=W)
        torch.cuda.synchronize()
    finally:
        sdf.sdf_threshold = thr
    return {k: (t[k].view(torch.uint8) if t[k].dtype == torch.bool else t[k]) for k in
            ("depth", "sdf_last", "finish", "points", "gradient", "t_end_k", "trips")}


def encode(a, n):
    """one output of a call over n rays or points"""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    e = dict(shape=list(a.shape), dtype=str(a.dtype))
    if n <= WHOLE:
        e["hex"] = a.tobytes().hex()
    else:
        e["sha256"] = hashlib.sha256(a.tobytes()).hexdigest()
    return e


def case_size(key):
    """rays or points of the call an entry belongs to"""
    kind, which = key.split("/")[:2]
    if kind == "trace":
        return int(key.split("/")[2])
    if kind == "image":
        return 1 if which == "one_view_1x1" else 70
    return 125 if which == "volume" else 17


def write_fixture(path, note, entries):
    """the note indented, one line per entry"""
    head = json.dumps(note, indent=1)[:-2]
    lines = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in entries.items())
    with open(path, "w") as f:
        f.write(head + ',\n "entries": {\n' + lines + "\n }\n}\n")


def trace_key(name, n, it):
    return f"trace/{name}/{n}/{it}"


def loop_properties(sdf, fdesc, o_d, out):
    """replay the start end's state from the recorded values (fp32, the loop's own operations) -> which of the loop's quirks this call
    shows: crossed ends, a start end converged before iters_max, a finished start end that kept moving, the background branch"""
    f32 = np.float32
    thr = f32(sdf.sdf_threshold)
    near, far, raw, t_end, track = (out[k].cpu().numpy() for k in ("near", "far", "track_sdf", "t_end", "track"))
    it = raw.shape[1] - 1
    t, step = near.copy(), raw[:, 0].copy()
    unf = np.zeros(len(t), bool)
    crossed = converged = stale = False
    for k in range(it):
        step = np.where(np.abs(step) <= thr, f32(0), step)
        m = np.abs(step) > thr
        unf = m if k == 0 else unf & m
        converged |= bool((~m & (far > 0) & np.isfinite(raw[:, k])).any())
        t = (t + step).astype(f32)
        t = np.where(t > far, far, t)
        stale |= bool((~unf & (track[:, k + 1] != track[:, k]).any(axis=1)).any())
        step = np.where(unf, raw[:, k + 1], step)
        ahead = t < t_end[:, k + 1]
        crossed |= bool((unf & ~ahead).any())
        unf = unf & ahead
    bg = False
    if fdesc.bg_sdf:
        plain = type(fdesc).from_buffer_copy(fdesc)
        plain.bg_sdf = 0
        no_bg = sdf_eval(sdf, plain, out["track"].reshape(-1, 3).contiguous(), False, False)["sdf"].cpu().numpy()
        ok = np.isfinite(no_bg)
        bg = bool((no_bg[ok] != raw.reshape(-1)[ok]).any())
    return dict(crossed=crossed, converged_before_iters_max=converged, moved_on_stale_value=stale, background_selected=bg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    entries, trips, props = {}, {}, {}
    for name, n, it in TRACE_CASES:
        out = run_trace(name, n, it)
        key = trace_key(name, n, it)
        entries.update({f"{key}/{k}": encode(v, n) for k, v in out.items()})
        trips[key] = int(out["trips"].item())
        if it == "default":
            sdf, fdesc = field(name)
            props[key] = loop_properties(sdf, fdesc, None, out)
            print(key, "trips", trips[key], props[key], flush=True)
    for which in POINT_CASES:
        entries.update({f"points/{which}/{k}": encode(v, case_size(f"points/{which}")) for k, v in run_points(which).items()})
    image_trips = {}
    for which in IMAGE_CASES:
        out = run_image(which)
        entries.update({f"image/{which}/{k}": encode(v, case_size(f"image/{which}")) for k, v in out.items()})
        image_trips[which] = out["trips"].cpu().tolist()
    print("image trips", image_trips, flush=True)
    note = dict(what="outputs of ls2fm_sphere_trace, ls2fm_trace_image, ls2fm_sdf_eval, ls2fm_sdf_eval_prepared and ls2fm_sdf_volume, "
                     "recorded on an MI355X from the library built at the commit before csrc/trace_loop.h existed",
                made_by="tests/golden/make_golden_trace_parent.py", device=torch.cuda.get_device_name(0),
                library=os.path.basename(_lib.LIB_PATH), fields=" ".join(field.__doc__.split()), trace_trips=trips,
                trace_properties=props, image_trips=image_trips)
    os.makedirs(args.out, exist_ok=True)
    write_fixture(os.path.join(args.out, "trace_parent.json"), note, entries)
    # the fixture itself
    for p in ("crossed", "converged_before_iters_max", "moved_on_stale_value", "background_selected"):
        assert any(v[p] for v in props.values()), p
    two = image_trips["two_views_7x5"]
    assert two[0] != two[1], two
    assert image_trips["two_views_7x5_all_converged"] == [0, 0], image_trips
    same_sdf = {k.split("/", 2)[2] for k in entries if k.startswith("points/sdf/")}
    assert same_sdf == {f"{n}/sdf" for n in FIELDS}, same_sdf
    print(f"wrote {len(entries)} entries")


if __name__ == "__main__":
    main()
