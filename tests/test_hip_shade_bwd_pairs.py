"""shade_bwd works rays of 64 .. 128 samples in PAIRS, one weight-gradient partial per pair (shade_bwd.hip, header 3.): the
smallest shapes at which pairing can go wrong -- a lone ray, one full pair, an odd tail, a ray's second wave partly or fully
live, the one-ray forms on either side of the switch (63 / 129 samples), pose gradients -- through the public render path,
against the CPU oracle at the bars of test_hip_fused_render.py."""
import pytest
import torch

import losses
from conftest import rel_err
from helpers import named_grads
from ls2fm import fused
from ls2fm.options import make_options
from oracle import fields as OF
from test_hip_fused_render import DEV, GTOL, TOL, _beta_ok, _exact_beta_grad, _oracle_states, _randomized

pytestmark = pytest.mark.gpu

# 16 levels: all 32 encoding channels live (the kernel's FULL variants); 6 levels: the variants with per-channel predicates
GRIDS = {16: dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=12, base_resolution=16),
         6: dict(n_levels=6, n_features_per_level=2, log2_hashmap_size=12, base_resolution=16)}
SCALE = 2.0          # BlendedMVS: the box is [-2, 2]^3

CASES = ([(r, 64, True, False) for r in (1, 2, 3, 5)] + [(r, 64, False, False) for r in (1, 2, 3, 5)] +
         [(r, n, True, False) for n in (65, 127, 128) for r in (2, 3)] +
         [(3, 63, True, False), (3, 129, True, False)] +
         [(3, 96, True, True)])


def _through_rays(n, seed):
    """rays that all cross the box (every ray carries gradient: a lone ray must not be a miss)"""
    gen = torch.Generator().manual_seed(seed)
    c = torch.tensor([0.0, 0.0, -2.5 * SCALE]).repeat(n, 1) + 0.02 * SCALE * torch.randn(n, 3, generator=gen)
    d = torch.tensor([0.0, 0.0, 1.0]).repeat(n, 1) + 0.15 * torch.randn(n, 3, generator=gen)
    return c.view(1, n, 3).to(DEV), d.view(1, n, 3).to(DEV)


def _setup(n_samples, dual):
    levels = 16 if dual else 6
    opt = make_options("BlendedMVS", device=DEV, dual_field=dual, sample_intvs=n_samples, hash_encoding=GRIDS[levels])
    cfg = OF.dataset_config("BlendedMVS", dual_field=dual, sample_intvs=n_samples, n_levels=levels, log2_hashmap_size=12)
    return (opt, cfg) + _randomized(opt, 41)


def _all_grads(sdf, rad):
    return {**{"s." + k: v for k, v in named_grads(sdf).items()}, **{"r." + k: v for k, v in named_grads(rad).items()}}


@pytest.mark.parametrize("n_rays,n_samples,dual,pose", CASES)
def test_paired_rays_vs_oracle_and_repeatable(n_rays, n_samples, dual, pose):
    opt, cfg, sdf, rad, ren = _setup(n_samples, dual)
    center, ray = _through_rays(n_rays, 42)
    tgt = torch.rand(1, n_rays, 3, generator=torch.Generator().manual_seed(43))
    nm = torch.tensor([0.2, -0.4, 0.7])

    def run():
        c, r = center.clone().requires_grad_(pose), ray.clone().requires_grad_(pose)
        sdf.zero_grad(set_to_none=True); rad.zero_grad(set_to_none=True)
        assert fused.can_render(ren, opt, c, r, sdf, rad)
        ret = ren.forward(opt, c, r, sdf, rad)
        losses.render_loss(ret, tgt.to(DEV), nm.to(DEV)).backward()
        torch.cuda.synchronize()
        g = {k: v.clone() for k, v in _all_grads(sdf, rad).items()}
        if pose:
            g["center"], g["ray"] = c.grad.cpu().clone(), r.grad.cpu().clone()
        return ret, g

    ret, g1 = run()
    _, g2 = run()
    for k in g1:
        assert torch.equal(g1[k], g2[k]), f"not repeatable: {k}"

    osd, ord_ = _oracle_states(sdf, rad)
    oc, orr = center.cpu().clone().requires_grad_(pose), ray.cpu().clone().requires_grad_(pose)
    oret = OF.render(cfg, oc, orr, osd, ord_)
    losses.render_loss(oret, tgt, nm).backward()
    for k in ("rgb", "sdfs_volume", "normals", "depth_mlp", "normal_mlp"):
        assert rel_err(ret[k].cpu(), oret[k]) < TOL, k
    checked = 0
    for pre, st in (("s.", osd), ("r.", ord_)):
        for k, ref in st.items():
            if pre + k not in g1:
                continue
            ref = ref.grad if ref.grad is not None else torch.zeros_like(ref)
            got = g1[pre + k]
            print(f"[{n_rays}x{n_samples} dual={dual} pose={pose}] {pre + k}: {rel_err(got, ref):.2e}")
            if k == "beta":
                _beta_ok(got, ref, _exact_beta_grad(cfg, sdf.state_dict(), rad.state_dict(), center, ray, tgt, nm))
            else:
                assert rel_err(got, ref) < GTOL, pre + k
            checked += 1
    assert checked == len(g1) - (2 if pose else 0)          # every parameter gradient was compared
    assert max(float(v.grad.abs().max()) for k, v in osd.items() if k.endswith("mlp.0.weight_v")) > 0
    if pose:
        assert rel_err(g1["center"], oc.grad) < GTOL and rel_err(g1["ray"], orr.grad) < GTOL


@pytest.mark.parametrize("n_samples,dual,pose", [(64, True, False), (64, False, False), (65, True, False), (127, True, False), (128, True, False),
                                                 (63, True, False), (129, True, False), (128, True, True), (96, True, True)])
def test_ray_does_not_depend_on_its_workgroup_mates(n_samples, dual, pose):
    """ray 0 of three, the loss reading ray 0 alone, against the same ray rendered alone: render outputs and table gradients bit
    for bit (a ray's per-sample work does not depend on the ray it shares a workgroup with, nor on the lone third ray).

    At 96 samples a 64-point wave of the table scatter holds the end of ray 0 beside the start of ray 1: the scatter classifies
    its runs of samples ray by ray there (bin_items.h: wave_runs), or ray 0's table gradient would change in its last bits with
    its neighbour (14 entries of the SDF table by one unit in the last place, 4.657e-10, with one decision per wave)."""
    opt, cfg, sdf, rad, ren = _setup(n_samples, dual)
    center, ray = _through_rays(3, 44)
    w_rgb = torch.tensor([0.7, -0.4, 0.9], device=DEV)
    nm = torch.tensor([0.2, -0.4, 0.7], device=DEV)

    def run(c, r):
        c, r = c.clone().requires_grad_(pose), r.clone().requires_grad_(pose)
        sdf.zero_grad(set_to_none=True); rad.zero_grad(set_to_none=True)
        ret = ren.forward(opt, c, r, sdf, rad)
        loss = (ret["rgb"][:, :1] * w_rgb).sum() + ret["depth_mlp"][:, :1].sum() + (ret["normal_mlp"][:, :1] * nm).sum() \
            + (ret["normals"][:, :1].norm(dim=-1) - 1).abs().mean()
        loss.backward()
        torch.cuda.synchronize()
        return ret, _all_grads(sdf, rad)

    ret3, g3 = run(center, ray)
    ret1, g1 = run(center[:, :1], ray[:, :1])
    for k in ("rgb", "sdfs_volume", "normals", "depth_mlp", "normal_mlp"):
        assert torch.equal(ret3[k][:, :1], ret1[k]), k
    tables = [k for k in g3 if k.endswith("embedder_obj.params")]
    assert len(tables) == (2 if dual else 1)
    for k in tables:
        assert g1[k].abs().max() > 0
        print(f"[{n_samples} dual={dual} pose={pose}] {k}: {int((g3[k] != g1[k]).sum())} entries differ, max |diff| {float((g3[k] - g1[k]).abs().max()):.3e}")
        assert torch.equal(g3[k], g1[k]), k
