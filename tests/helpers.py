"""Shared case builders: one seeded synthetic case evaluated by the CPU oracle and by the HIP path."""
from __future__ import annotations

import dataclasses
import math
import re
from dataclasses import dataclass

import numpy as np
import torch

from gstex_amd.charts import build_charts
from gstex_amd.scene import CAM_RADIUS, Scene, make_scene, sphere_view
from oracle import raster as O

TOL_ABS = 1e-5  # forward parity tolerance (fp32), north_star: "within 1e-5 fp32"
TOL_REL = 1e-5
GRAD_RTOL = 1e-5  # gradient tolerance (norm-wise and max-element relative, vs the oracle's fp64 autograd), test_gpu_parity.py


@dataclass
class Case:
    inp: O.RasterInputs
    view: object
    C: int
    nth: torch.Tensor
    flip_mask: torch.Tensor = None  # set by oracle_run: pixels excluded from gradient comparisons


def anisotropic(scene: Scene, ratio, seed, n_texels) -> Scene:
    """The scene with each splat's two in-plane scales pulled apart: s_u *= e^r, s_v *= e^-r, r uniform in
    +-log(ratio) / 2 (s_u / s_v within [1 / ratio, ratio], the product s_u s_v kept), recharted for the new scales
    (non-square h x w blocks) with fresh texels.  Seeded on its own generator (seed + 77).  ratio <= 1: the scene as
    it is."""
    if ratio <= 1.0:
        return scene
    g = torch.Generator().manual_seed(seed + 77)
    r = (torch.rand(scene.n, generator=g) * 2 - 1) * math.log(ratio) / 2
    log_scales = scene.log_scales.clone()
    log_scales[:, 0] += r
    log_scales[:, 1] -= r
    if n_texels and n_texels > 0:
        dims, mappings, ps = build_charts(log_scales, float(n_texels))
        T = int((dims[:, 0] * dims[:, 1]).sum().item())
        texture = torch.rand((T, scene.texture.shape[1]), generator=g)
    else:  # 2DGS mode (make_scene): no blocks, the mappings follow the scales
        dims, texture, ps = scene.texture_dims, scene.texture, scene.pixel_scale
        mappings = torch.stack([1 / (6.0 * torch.exp(log_scales[:, 0])), 1 / (6.0 * torch.exp(log_scales[:, 1]))], -1)
    return dataclasses.replace(scene, log_scales=log_scales, texture_dims=dims, mappings=mappings, texture=texture,
                               pixel_scale=ps)


def make_case(n=300, n_texels=20000, H=64, W=80, seed=0, view=0, opacity=None, C=3,
              settings=(1 << 9) | (1 << 10), bg=None, cube=2.0, glob_scale=1.0, *, aniso=1.0, radius=CAM_RADIUS):
    """aniso > 1: the scene through anisotropic(); radius: the camera's distance from the centre of the +-cube/2 cube
    the splats fill (below ~1.7 the near plane and the camera plane cut into the scene)."""
    sc = anisotropic(make_scene(n, n_texels, channels=C, seed=seed, opacity=opacity, cube=cube), aniso, seed, n_texels)
    v = sphere_view(view, H, W, radius=radius)
    means, scales, quats, opac = sc.activated()
    cam = O.Camera(v.viewmat, v.fx, v.fy, v.cx, v.cy, H, W, 16, v.c2w[:3, 3])
    centers, extents = O.aabb_2d(means, scales, glob_scale, quats, cam)
    _, depths = O.project_points(means, cam)
    nth = O.num_tiles_hit(centers, extents, H, W)
    uv0, umap, vmap = sc.uv_mapping()
    g = torch.Generator().manual_seed(seed + 1000)
    rgbs = torch.rand((n, 3), generator=g)
    inp = O.RasterInputs(sc.texture_dims, centers.detach().clone(), extents, depths, rgbs, opac.detach().clone(),
                         means.detach().clone(), scales.detach().clone(), glob_scale, quats.detach().clone(),
                         uv0.detach().clone(), umap, vmap, sc.texture.clone(), cam, settings,
                         None if bg is None else torch.tensor(bg, dtype=torch.float32))
    return Case(inp, v, C, nth)


DIFF = ["rgbs", "opacities", "means", "scales", "quats", "texture", "centers", "uv0"]


def upstream(H, W, C, seed=5, mask=None, tex_channel_scale=None):
    """Seeded upstream gradients of the six outputs; zero at the pixels of `mask` (H, W bool) if given.
    tex_channel_scale: C factors, one per channel of the tex upstream (the same draws, scaled)."""
    g = torch.Generator().manual_seed(seed)
    up = dict(img=torch.randn(H, W, 3, generator=g), depth=torch.randn(H, W, generator=g),
              reg=torch.randn(H, W, generator=g), alpha=torch.randn(H, W, generator=g),
              tex=torch.randn(H, W, C, generator=g), normal=torch.randn(H, W, 3, generator=g))
    if tex_channel_scale is not None:
        scale = torch.as_tensor(tex_channel_scale, dtype=torch.float32)
        assert scale.shape == (C,)
        up["tex"] = up["tex"] * scale
    if mask is not None and bool(mask.any()):
        for k, v in up.items():
            v[mask] = 0.0
    return up


def _scale_kw(tex_channel_scale):
    """upstream()'s per-channel scale as a keyword, passed only when one is given (a test may put an upstream of the
    five-argument form in this module's place)."""
    return {} if tex_channel_scale is None else {"tex_channel_scale": tex_channel_scale}


def _differentiable(settings, outputs):
    """Outputs that take an upstream gradient: with settings bit 15 the unit normal is a forward-only output."""
    if settings & O.SETTING_EVAL_NORMAL:
        names = outputs if outputs is not None else ("img", "depth", "reg", "alpha", "tex", "normal")
        return tuple(k for k in names if k != "normal")
    return outputs


def oracle_run(case: Case, grads=True, seed=5, grad_dtype=torch.float64, outputs=None, flip_mask=None,
               tex_channel_scale=None):
    """flip_mask: use this mask (e.g. one computed on another machine, whose CPU exp may round differently) instead of
    the one this run's margins give.  tex_channel_scale: see upstream()."""
    inp = case.inp
    leaves = {}
    if grads:
        for k in DIFF:
            t = getattr(inp, k).detach().clone().requires_grad_(True)
            setattr(inp, k, t)
            leaves[k] = t
    o32, o64, aux = O.rasterize(inp, grad_dtype=grad_dtype)
    # pixels with a threshold decision within FLIP_MARGIN (an exp ulp may flip it on the GPU; the forward check
    # accounts for them) take no upstream gradient in either run, so a flipped pair cannot enter the comparison
    case.flip_mask = aux["margin"] < FLIP_MARGIN if flip_mask is None else flip_mask
    out = {}
    outputs = _differentiable(inp.settings, outputs)
    if grads:
        up = upstream(inp.cam.H, inp.cam.W, case.C, seed, case.flip_mask, **_scale_kw(tex_channel_scale))
        loss = sum((o64[k] * up[k].to(grad_dtype)).sum() for k in up if outputs is None or k in outputs)
        loss.backward()
        out = {k: (v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v).detach()).float()
               if v.grad is None else v.grad.detach().clone() for k, v in leaves.items()}
        for k in DIFF:
            setattr(inp, k, getattr(inp, k).detach())
    return o32, o64, aux, out


def gpu_run(case: Case, grads=True, seed=5, device="cuda", outputs=None, tex_channel_scale=None):
    """outputs: names of the outputs that receive an upstream gradient (default all six; the others
    reach the kernel as NULL, as for outputs the loss does not use).  tex_channel_scale: see upstream()."""
    import gstex_cuda

    inp = case.inp
    v = case.view
    dv = lambda t: t.detach().to(device).contiguous()  # noqa: E731
    t = {k: dv(getattr(inp, k)) for k in DIFF}
    if grads:
        for k in t:
            t[k].requires_grad_(True)
    n = inp.means.shape[0]
    outs = gstex_cuda.texture_gaussians(
        (n, 1, case.C), dv(inp.texture_dims), t["centers"], dv(inp.extents), dv(inp.depths), dv(case.nth),
        t["rgbs"], t["opacities"], t["means"], t["scales"], inp.glob_scale, t["quats"], t["uv0"], dv(inp.umap),
        dv(inp.vmap), t["texture"], dv(v.viewmat), dv(v.c2w), v.fx, v.fy, v.cx, v.cy, inp.cam.H, inp.cam.W, 16,
        inp.settings, background=None if inp.background is None else dv(inp.background))
    names = ["img", "depth", "reg", "alpha", "tex", "normal"]
    res = {k: o.detach().cpu() for k, o in zip(names, outs)}
    gr = {}
    outputs = _differentiable(inp.settings, outputs)
    if grads:
        up = upstream(inp.cam.H, inp.cam.W, case.C, seed, case.flip_mask, **_scale_kw(tex_channel_scale))
        sel = [i for i, k in enumerate(names) if outputs is None or k in outputs]
        torch.autograd.backward([outs[i] for i in sel], [up[names[i]].to(device) for i in sel])
        gr = {k: (t[k].grad.detach().cpu() if t[k].grad is not None else torch.zeros_like(t[k]).cpu()) for k in t}
    return res, gr


FLIP_MARGIN = 1e-5  # relative distance from a threshold within which an fp32 decision may flip (exp/rcp ulps)
FLIP_FRACTION = 1e-3  # at most this fraction of the pixels (and at least 4) may carry a flipped decision


# Cases outside the random-init distribution of make_scene (isotropic splats, square charts, a camera 2.7 away from
# the nearest splat, glob_scale 1): anisotropic splats on non-square charts, glob_scale != 1, cameras close to and
# inside the +-1 cube.  Fixed inputs; check_stress asserts, from the oracle's run alone, that each reaches its regime.
# Seeds tried: the ones below only (every condition of check_stress held at the first seed of each row).
STRESS_CASES = {
    "aniso4": dict(n=150, n_texels=6000, H=48, W=48, seed=3, aniso=4),
    "aniso10_glob": dict(n=150, n_texels=6000, H=48, W=48, seed=5, aniso=10, glob_scale=1.4, opacity=None),
    "glob0.6": dict(n=150, n_texels=6000, H=48, W=48, seed=6, glob_scale=0.6),
    "near1.3": dict(n=300, n_texels=8000, H=48, W=48, seed=7, radius=1.3, opacity=None),
    "inside0.5_aniso4": dict(n=300, n_texels=8000, H=48, W=48, seed=8, radius=0.5, aniso=4, opacity=None),
    "2dgs_near": dict(n=300, n_texels=0, H=48, W=48, seed=9, radius=1.0),
}
STRESS_ANISO = ("aniso4", "aniso10_glob", "inside0.5_aniso4")
STRESS_NEAR = ("near1.3", "inside0.5_aniso4", "2dgs_near")


def cull_classes(inp):
    """The oracle's preprocessing classes of every splat (preprocess.hip's branches, from oracle values alone):
    near: Tw.z <= near; crossing: not near, and the 3-sigma disc reaches the camera plane (d >= 0); clipped: centre
    depth <= 0.01 (project_points writes xy = 0)."""
    _, _, Tw = O.splat_homography(inp.means, inp.scales, inp.glob_scale, inp.quats, inp.cam)
    c9 = float(O.K_CUTOFF2)
    d = (c9 * (Tw[:, 0] * Tw[:, 0]) + c9 * (Tw[:, 1] * Tw[:, 1])) - Tw[:, 2] * Tw[:, 2]
    near = Tw[:, 2] <= float(O.K_NEAR)
    return dict(near=near, crossing=~near & (d >= 0), clipped=inp.depths <= float(O.K_PROJ_CLIP))


def check_stress(name, case, aux):
    """The stress case reaches the regime it is named for: facts of the oracle's run, not of the code under test."""
    inp = case.inp
    n = inp.means.shape[0]
    seen = torch.zeros(n, dtype=torch.bool)  # splats on some tile list
    seen[torch.as_tensor(aux["sorted_ids"]).long()] = True
    h, w = inp.texture_dims[:, 0].long(), inp.texture_dims[:, 1].long()
    if name in STRESS_ANISO:
        assert int((h != w).sum()) * 2 >= n, f"{name}: only {int((h != w).sum())} / {n} non-square charts"
        assert bool((seen & ((h > 2 * w) | (w > 2 * h))).any()), f"{name}: no visible chart beyond 2:1"
    if name in STRESS_NEAR:
        cls = cull_classes(inp)
        assert bool(cls["near"].any()), f"{name}: no splat culled by Tw.z <= near"
        assert bool(cls["crossing"].any()), f"{name}: no splat culled by d >= 0"
        assert not bool((seen & (cls["near"] | cls["crossing"])).any())
        skipped = torch.zeros(n, dtype=torch.bool)  # splats with a reached pair skipped for z < near ...
        included = torch.zeros(n, dtype=torch.bool)  # ... and with a pair that contributes
        for d in aux["decisions"]["tiles"].values():
            skipped[d["ids"][d["near_skip"].any(1)]] = True
            included[d["ids"][d["incl"].any(1)]] = True
        assert bool((skipped & included).any()), f"{name}: no splat with one pair skipped for z < near, another kept"
        if name == "inside0.5_aniso4":
            assert bool(cls["clipped"].any()), f"{name}: no centre with z <= 0.01"
    assert float(aux["T_final"].detach().min()) < 0.5, f"{name}: alpha.max() <= 0.5"
    H, W = inp.cam.H, inp.cam.W
    near_flip = int((aux["margin"] < FLIP_MARGIN).sum())
    assert near_flip <= max(4, FLIP_FRACTION * H * W), f"{name}: {near_flip} pixels within FLIP_MARGIN of a threshold"


# Channel counts without an instantiation of their own (every C but 3 and 6 runs the raster kernels' runtime-channel
# build, raster_fwd.hip / raster_bwd.hip: CM = 8 register slots, Cn = the call's C), at C > 1 so that a wrong channel stride moves an address:
# C = 8 (every slot live), a C = 8 case with texel blocks on both sides of the backward's staging size, an odd C on a
# ragged image, C = 2, C = 4 without the AA branch, C = 7 with a background.  Fixed inputs; check_channels asserts, from
# the oracle's run alone, that each reaches its regime.  Seeds tried: the ones below only.
CHANNEL_CASES = {
    "tex8": dict(n=200, n_texels=8000, H=40, W=40, seed=12, C=8),
    "tex8_mixed_blocks": dict(n=80, n_texels=10000, H=40, W=40, seed=13, C=8),
    "tex5_ragged": dict(n=150, n_texels=5000, H=17, W=33, seed=14, C=5),
    "tex2": dict(n=200, n_texels=8000, H=40, W=40, seed=15, C=2),
    "tex4_noaa": dict(n=200, n_texels=8000, H=40, W=40, seed=16, C=4, settings=1 << 10),
    "tex7_bg": dict(n=200, n_texels=8000, H=40, W=40, seed=17, C=7, bg=(0.2, 0.5, 0.9)),
}
CHANNEL_PHOTOMETRIC = ("tex8", "tex8_mixed_blocks", "tex5_ragged", "tex2")
# C = 5 for the deterministic per-pair rows against the float-atomic sums, and for bitwise reproducibility
ROWS_CASES = {"rows_tex5": dict(n=300, n_texels=12000, H=48, W=48, seed=29, C=5)}
# Tile lists of three kSegLen = 256 segments (multi-segment checkpoints, whose field count and plane offsets follow C)
# at C = 8 and C = 5.  Seeds tried: C = 8: n=2500, seed=18 (8 pixels near a threshold, cap 4), then 19 (2 pixels);
# C = 5: 20 (5 pixels), then 21 (2 pixels).
DEEP_CHANNEL_CASES = {
    "deep_tex8": dict(n=1500, n_texels=15000, H=32, W=32, seed=19, C=8, opacity=0.05),
    "deep_tex5": dict(n=1500, n_texels=15000, H=32, W=32, seed=21, C=5, opacity=0.05),
}
TEX_STAGE = 1024  # the backward's texel staging size in entries (raster_bwd.hip: kTexStage, GSTEX_TEX_STAGE's default)
SEG_LEN = 256  # tile-list positions per checkpoint segment (raster_common.h: kSegLen, GSTEX_SEG_LEN's default)


def check_channels(name, case, aux):
    """The generic-channel case reaches the regime it is named for: facts of the oracle's run, not of the code under
    test."""
    inp = case.inp
    C = int(re.search(r"tex(\d)", name).group(1))
    assert case.C == C and inp.texture.shape[1] == C and C not in (1, 3, 6), f"{name}: C = {case.C}"
    n = inp.means.shape[0]
    seen = torch.zeros(n, dtype=torch.bool)  # splats on some tile list
    seen[torch.as_tensor(aux["sorted_ids"]).long()] = True
    entries = (inp.texture_dims[:, 0].long() * inp.texture_dims[:, 1].long() * C)[seen]
    assert entries.numel() > 0 and int(entries.min()) > 0
    # a block of h * w * C <= TEX_STAGE entries is summed in the staging area and flushed, a larger one goes
    # straight to global atomics (raster_bwd_kernel: staged = bsize <= kTexStage)
    staged, unstaged = int((entries <= TEX_STAGE).sum()), int((entries > TEX_STAGE).sum())
    if name == "tex8_mixed_blocks":
        assert staged >= 10 and unstaged >= 10, f"{name}: {staged} staged blocks, {unstaged} above the staging size"
    else:
        assert unstaged == 0, f"{name}: {unstaged} blocks above the staging size"
    H, W = inp.cam.H, inp.cam.W
    near_flip = int((aux["margin"] < FLIP_MARGIN).sum())
    assert near_flip <= max(4, FLIP_FRACTION * H * W), f"{name}: {near_flip} pixels within FLIP_MARGIN of a threshold"
    assert float(aux["T_final"].detach().min()) < 0.5, f"{name}: alpha.max() <= 0.5"
    return dict(staged=staged, unstaged=unstaged, largest=int(entries.max()) // C, near_flip=near_flip)


def check_deep_channels(name, case, aux):
    """The deep generic-channel case has three-segment tile lists with a contributor in the third segment (so the
    backward restarts from two checkpoints and reads the final accumulators from the third slot): oracle facts."""
    inp = case.inp
    C = int(re.search(r"tex(\d)", name).group(1))
    assert case.C == C and inp.texture.shape[1] == C and C not in (1, 3, 6), f"{name}: C = {case.C}"
    tr = np.asarray(aux["tile_ranges"])
    lens = tr[:, 1] - tr[:, 0]
    assert int(lens.min()) > 2 * SEG_LEN, f"{name}: a tile list of {int(lens.min())}"
    last = np.asarray(aux["last"])
    assert int(last.max()) > 2 * SEG_LEN, f"{name}: deepest contributor at {int(last.max())}"
    H, W = inp.cam.H, inp.cam.W
    near_flip = int((aux["margin"] < FLIP_MARGIN).sum())
    assert near_flip <= max(4, FLIP_FRACTION * H * W), f"{name}: {near_flip} pixels within FLIP_MARGIN of a threshold"
    assert float(aux["T_final"].detach().min()) < 0.5, f"{name}: alpha.max() <= 0.5"
    return dict(lists=(int(lens.min()), int(lens.max())), last=int(last.max()), near_flip=near_flip)


def assert_close_fwd(gpu, ref64, names=("img", "depth", "reg", "alpha", "tex", "normal"), margin=None):
    """Every output element within 1e-5 (+1e-5 relative) of the oracle.  With `margin` (the oracle's per-pixel
    decision margins, aux["margin"]): a pixel outside the tolerance passes only if one of its threshold decisions
    lies within FLIP_MARGIN of the threshold (an ulp of exp can flip it on either side), and such pixels are
    rare (FLIP_FRACTION)."""
    flipped = None
    for k in names:
        a = gpu[k].double()
        b = ref64[k].double()
        err = (a - b).abs()
        bound = TOL_ABS + TOL_REL * b.abs()
        bad = err > bound
        if margin is not None and bool(bad.any()):
            pix = bad if bad.dim() == 2 else bad.any(-1)
            unexplained = pix & ~(margin < FLIP_MARGIN)
            assert not bool(unexplained.any()), (
                f"{k}: {int(unexplained.sum())} pixels outside 1e-5 (+1e-5 rel) with no decision near a threshold; "
                f"max err {err.max().item():.3e}")
            flipped = pix if flipped is None else flipped | pix
            continue
        assert not bool(bad.any()), (
            f"{k}: {int(bad.sum())} / {bad.numel()} elements outside 1e-5 (+1e-5 rel); max err {err.max().item():.3e}")
    if flipped is not None:
        n = int(flipped.sum())
        assert n <= max(4, FLIP_FRACTION * flipped.numel()), f"{n} pixels with flipped decisions"
        print(f"[parity] {n} / {flipped.numel()} pixels differ by a decision flipped within {FLIP_MARGIN:g} of its threshold")


def grad_rel_err(g, ref):
    if ref.numel() == 0:
        return 0.0, 0.0
    scale = ref.abs().max().item()
    return (g.double() - ref.double()).abs().max().item() / max(scale, 1e-12), scale


def grad_norm_err(g, ref):
    if ref.numel() == 0:
        return 0.0
    n = ref.double().norm().item()
    return (g.double() - ref.double()).norm().item() / max(n, 1e-30)


_SCENES: dict = {}


def make_window_case(n, n_texels, H, W, win, seed=42, view=0, C=3, settings=(1 << 9) | (1 << 10), opacity=0.1):
    """A win x win window at the centre of the H x W sphere view `view` of the seeded make_scene(n, n_texels)
    (the bench scenes: cfg3 = 200k / 1e7 / 800x800, cfg2 = 50k / 1e6 / 800x800): the camera's principal point
    is shifted by the window origin (the bench's cpu_baseline crop), and only the splats that reach the window
    are kept, their texel blocks repacked contiguously (same texels, offsets re-based) -- the other splats
    contribute nothing to these pixels.  Returns a Case usable by oracle_run / gpu_run."""
    from gstex_amd.scene import View

    key = (n, n_texels, seed, opacity)
    if key not in _SCENES:
        _SCENES.clear()
        _SCENES[key] = make_scene(n, n_texels, channels=C, seed=seed, opacity=opacity)
    sc = _SCENES[key]
    full = sphere_view(view, H, W)
    x0, y0 = W // 2 - win // 2, H // 2 - win // 2
    v = View(full.viewmat, full.c2w, full.fx, full.fy, full.cx - x0, full.cy - y0, win, win)
    means, scales, quats, opac = sc.activated()
    cam = O.Camera(v.viewmat, v.fx, v.fy, v.cx, v.cy, win, win, 16, v.c2w[:3, 3])
    centers, extents = O.aabb_2d(means, scales, 1.0, quats, cam)
    nth = O.num_tiles_hit(centers, extents, win, win)
    keep = torch.nonzero(nth > 0).squeeze(1)
    dims = sc.texture_dims[keep].clone()
    hw = (dims[:, 0].long() * dims[:, 1].long())
    rows = torch.cat([torch.arange(int(o), int(o) + int(s)) for o, s in zip(sc.texture_dims[keep, 2].tolist(),
                                                                            hw.tolist())]) if keep.numel() else \
        torch.zeros(0, dtype=torch.long)
    dims[:, 2] = (torch.cumsum(hw, 0) - hw).to(torch.int32)
    texture = sc.texture[rows].clone() if rows.numel() else torch.zeros((0, C))
    uv0, umap, vmap = sc.uv_mapping()
    means, scales, quats, opac = means[keep], scales[keep], quats[keep], opac[keep]
    _, depths = O.project_points(means, cam)
    g = torch.Generator().manual_seed(seed + 1000)
    rgbs = torch.rand((sc.n, 3), generator=g)[keep]
    inp = O.RasterInputs(dims, centers[keep].detach().clone(), extents[keep], depths, rgbs,
                         opac.detach().clone(), means.detach().clone(), scales.detach().clone(), 1.0,
                         quats.detach().clone(), uv0[keep].detach().clone(), umap[keep], vmap[keep], texture, cam,
                         settings, None)
    return Case(inp, v, C, nth[keep])
