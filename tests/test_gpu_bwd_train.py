"""The raster backward's training build (raster_bwd_kernel<3, false, TRAIN>, gstex_raster_bwd_variant) against the
generic build and the fp64 oracle.  Needs an MI355X.

Each scene runs twice through texture_gaussians' backward with a photometric upstream (img, alpha, tex; the tex
gradient equal to the img gradient, as the loss delivers it): once with ONE tensor for both (the query says TRAIN), once
with v_tex = v_img.clone() (generic).  Every gradient of both runs is held to the parity criterion of tests/helpers.py
(norm-wise relative error <= GRAD_RTOL = 1e-5) against the fp64 oracle, and the TRAIN run to the same criterion against
the generic run.  The scenes are the smallest that reach each branch of the visit loop."""
import math

import pytest
import torch

from gstex_amd.scene import make_scene, sphere_view
from helpers import DIFF, FLIP_MARGIN, GRAD_RTOL, STRESS_CASES, Case, check_stress, grad_norm_err, make_case
from oracle import raster as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
TEX_STAGE_TEXELS = 341  # raster_bwd.hip kTexStage / 3: a larger block's run tails go straight to global memory
DEEP_SCALE = 16.0  # the deep-list scene's splat enlargement (median screen extent 11 px; the other scenes' is 15)


def _partial_tiles():
    return make_case(n=300, n_texels=20000, H=70, W=93, seed=31, bg=(0.2, 0.5, 0.9))


def _deep_list():
    """600 splats piled on the four tiles of a 32 x 32 view (cube 0.3), enlarged to the screen size of the other
    scenes' splats (as piled they are sub-pixel: every pair would take the low-pass branch, whose scale gradient is
    zero), at opacity 0.02 so that the pixels' last contributors lie deep in the lists."""
    H = W = 32
    sc = make_scene(600, 12000, seed=32, opacity=0.02, cube=0.3)
    sc.log_scales = sc.log_scales + math.log(DEEP_SCALE)
    v = sphere_view(0, H, W)
    means, scales, quats, opac = sc.activated()
    cam = O.Camera(v.viewmat, v.fx, v.fy, v.cx, v.cy, H, W, 16, v.c2w[:3, 3])
    centers, extents = O.aabb_2d(means, scales, 1.0, quats, cam)
    _, depths = O.project_points(means, cam)
    uv0, umap, vmap = sc.uv_mapping()
    rgbs = torch.rand((sc.n, 3), generator=torch.Generator().manual_seed(1032))
    d = lambda t: t.detach().clone()  # noqa: E731
    inp = O.RasterInputs(sc.texture_dims, d(centers), extents, depths, rgbs, d(opac), d(means), d(scales), 1.0,
                         d(quats), d(uv0), umap, vmap, sc.texture.clone(), cam, (1 << 9) | (1 << 10), None)
    return Case(inp, v, 3, O.num_tiles_hit(centers, extents, H, W))


def _set_block(case, k, h, w, seed):
    """Give splat k an h x w texel block of its own, appended to the texel store."""
    inp = case.inp
    dims = inp.texture_dims.clone()
    dims[k] = torch.tensor([h, w, inp.texture.shape[0]], dtype=dims.dtype)
    inp.texture_dims = dims
    if h * w:
        g = torch.Generator().manual_seed(seed)
        inp.texture = torch.cat([inp.texture, torch.rand((h * w, inp.texture.shape[1]), generator=g)])


def _widest(case):
    """The visible splat with the largest screen extent."""
    area = case.inp.extents.prod(-1) * (case.nth > 0)
    return int(area.argmax())


def _large_block():
    case = make_case(n=12, n_texels=600, H=48, W=48, seed=33, cube=1.0)
    _set_block(case, _widest(case), 20, 20, 1)
    return case


def _untextured():
    case = make_case(n=40, n_texels=2500, H=40, W=56, seed=34)
    _set_block(case, _widest(case), 0, 0, 0)
    return case


def _near_edge_on():
    return make_case(n=40, n_texels=2500, H=40, W=56, seed=35)


# outside the random-init distribution (helpers.STRESS_CASES): anisotropic splats on non-square charts with glob_scale
# 1.4; a camera at the edge of the splat cube (near-plane culls, per-pair z < near skips)
STRESS = {"aniso": "aniso10_glob", "near": "near1.3"}

SCENES = {"partial_tiles": _partial_tiles, "deep_list": _deep_list, "large_block": _large_block,
          "untextured": _untextured, "near_edge_on": _near_edge_on,
          "aniso": lambda: make_case(**STRESS_CASES[STRESS["aniso"]]),
          "near": lambda: make_case(**STRESS_CASES[STRESS["near"]])}


def _check_scene(name, case, aux):
    """The scene reaches the branch it is named for (facts of the oracle's run, not of the code under test)."""
    inp = case.inp
    hw = inp.texture_dims[:, 0].long() * inp.texture_dims[:, 1].long()
    seen = torch.zeros(inp.means.shape[0], dtype=torch.bool)  # splats on some tile list
    seen[torch.as_tensor(aux["sorted_ids"]).long()] = True
    if name == "partial_tiles":
        assert inp.cam.H % 16 and inp.cam.W % 16 and inp.background is not None
    elif name == "deep_list":
        # a wave's last contributor lies past position 512: three 256-position segments, two checkpoint starts
        assert int(torch.as_tensor(aux["last"]).max()) >= 512
    elif name == "large_block":
        assert bool((seen & (hw > TEX_STAGE_TEXELS)).any())
    elif name == "untextured":
        assert bool((seen & (hw == 0)).any()) and bool((seen & (hw > 0)).any())
    elif name == "near_edge_on":
        assert bool((seen & O._splat_table(inp, torch.float64)["hp"]).any())
    elif name in STRESS:
        check_stress(STRESS[name], case, aux)


_ORACLE: dict = {}


def _oracle(name):
    """(case, upstream (g, g_alpha), fp64 gradients) of a scene, computed once."""
    if name in _ORACLE:
        return _ORACLE[name]
    case = SCENES[name]()
    inp = case.inp
    leaves = {}
    for k in DIFF:
        leaves[k] = getattr(inp, k).detach().clone().requires_grad_(True)
        setattr(inp, k, leaves[k])
    _, o64, aux = O.rasterize(inp)
    _check_scene(name, case, aux)
    H, W = inp.cam.H, inp.cam.W
    gen = torch.Generator().manual_seed(7)
    g, ga = torch.randn(H, W, 3, generator=gen), torch.randn(H, W, generator=gen)
    flip = aux["margin"] < FLIP_MARGIN  # (helpers.oracle_run: no upstream where an fp32 decision may flip)
    g[flip] = 0.0
    ga[flip] = 0.0
    loss = (o64["img"] * g.double()).sum() + (o64["alpha"] * ga.double()).sum() + (o64["tex"] * g.double()).sum()
    loss.backward()
    ref = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().clone() for k, v in leaves.items()}
    for k in DIFF:
        setattr(inp, k, getattr(inp, k).detach())
    _ORACLE[name] = (case, (g, ga), ref)
    return _ORACLE[name]


def _record_variants(monkeypatch):
    """The build every gstex_raster_bwd call of the test selects, by the library's own query."""
    from gstex_amd import _lib, ops

    seen = []
    inner = ops._launch

    def launch(name, *args):
        if name == "gstex_raster_bwd":
            seen.append(_lib.load().gstex_raster_bwd_variant(args[0]))
        return inner(name, *args)
    monkeypatch.setattr(ops, "_launch", launch)
    return seen


def _gpu_grads(case, g, ga, shared):
    import gstex_cuda

    inp, v = case.inp, case.view
    dv = lambda t: t.detach().to(DEV).contiguous()  # noqa: E731
    t = {k: dv(getattr(inp, k)).requires_grad_(True) for k in DIFF}
    n = inp.means.shape[0]
    img, _, _, alpha, tex, _ = gstex_cuda.texture_gaussians(
        (n, 1, 3), dv(inp.texture_dims), t["centers"], dv(inp.extents), dv(inp.depths), dv(case.nth), t["rgbs"],
        t["opacities"], t["means"], t["scales"], inp.glob_scale, t["quats"], t["uv0"], dv(inp.umap), dv(inp.vmap),
        t["texture"], dv(v.viewmat), dv(v.c2w), v.fx, v.fy, v.cx, v.cy, inp.cam.H, inp.cam.W, 16, inp.settings,
        background=None if inp.background is None else dv(inp.background))
    v_img = g.to(DEV)
    v_tex = v_img if shared else v_img.clone()
    torch.autograd.backward([img, alpha, tex], [v_img, ga.to(DEV), v_tex])
    return {k: (torch.zeros_like(x) if x.grad is None else x.grad).detach().cpu() for k, x in t.items()}


@pytest.mark.parametrize("name", list(SCENES))
def test_train_build_matches_generic_and_oracle(name, monkeypatch):
    from gstex_amd import _lib

    case, (g, ga), ref = _oracle(name)
    seen = _record_variants(monkeypatch)
    train = _gpu_grads(case, g, ga, shared=True)
    generic = _gpu_grads(case, g, ga, shared=False)
    assert seen == [_lib.BWD_TRAIN, _lib.BWD_GENERIC]
    errs = {k: (grad_norm_err(train[k], ref[k]), grad_norm_err(generic[k], ref[k]), grad_norm_err(train[k], generic[k]))
            for k in DIFF}
    print(f"[bwd-train] {name} norm-rel (train vs oracle, generic vs oracle, train vs generic): "
          + ", ".join(f"{k}={a:.1e}/{b:.1e}/{c:.1e}" for k, (a, b, c) in errs.items()))
    for k in DIFF:  # no gradient of the scene is degenerate (a zero the runs could only match in rounding noise)
        assert float(ref[k].norm()) > 1e-3, f"{name}: the oracle's {k} gradient is (almost) zero"
    for k, (a, b, c) in errs.items():
        assert a <= GRAD_RTOL, f"{name}: TRAIN grad {k} vs oracle {a:.3e} > {GRAD_RTOL:.0e}"
        assert b <= GRAD_RTOL, f"{name}: generic grad {k} vs oracle {b:.3e} > {GRAD_RTOL:.0e}"
        assert c <= GRAD_RTOL, f"{name}: TRAIN grad {k} vs generic {c:.3e} > {GRAD_RTOL:.0e}"


@pytest.mark.parametrize("dataset", [False, True])
def test_loss_backward_shares_one_gradient_image(dataset):
    """photometric_loss / image_loss at C = 3: img and tex receive one tensor, whose values are bit for bit the two
    tensors of share_grad=False; at C = 4 the gradients stay separate, and the C entry point refuses d_tex == d_img."""
    from gstex_amd import _lib
    from gstex_amd.loss import _cwin, image_loss, photometric_loss

    H, W = 70, 93
    gen = torch.Generator().manual_seed(41)
    img = (torch.rand(H, W, 3, generator=gen) * 1.4 - 0.2).to(DEV)
    alpha, bg = torch.rand(H, W, generator=gen).to(DEV), torch.rand(3, generator=gen).to(DEV)
    gt = torch.rand(H, W, 3, generator=gen).to(DEV)
    target = (gt * 255).to(torch.uint8) if dataset else gt
    mask = (torch.rand(H, W, generator=gen) > 0.2).to(DEV) if dataset else None

    def run(C, share):
        tex = (torch.rand(H, W, C, generator=torch.Generator().manual_seed(C)) * 0.3).to(DEV)
        got = {}

        class Probe(torch.autograd.Function):  # sees the gradients as the raster backward would
            @staticmethod
            def forward(ctx, a, b):
                return a.clone(), b.clone()

            @staticmethod
            def backward(ctx, ga, gb):
                got["img"], got["tex"] = ga, gb
                return ga, gb
        a, b = Probe.apply(img.clone().requires_grad_(True), tex.requires_grad_(True))
        al = alpha.clone().requires_grad_(True)
        loss = (image_loss(a, b, al, bg, target, mask, share_grad=share).loss if dataset
                else photometric_loss(a, b, al, bg, target, share_grad=share)[0])
        loss.backward()
        return got["img"], got["tex"], al.grad

    s_img, s_tex, s_alpha = run(3, True)
    u_img, u_tex, u_alpha = run(3, False)
    assert s_tex.data_ptr() == s_img.data_ptr() and u_tex.data_ptr() != u_img.data_ptr()
    assert torch.equal(s_img, u_img) and torch.equal(s_img, u_tex) and torch.equal(s_alpha, u_alpha)
    assert float(s_img.abs().max()) > 0
    f_img, f_tex, _ = run(4, True)
    assert f_tex.data_ptr() != f_img.data_ptr() and torch.equal(f_tex[..., :3], f_img)
    assert float(f_tex[..., 3].abs().max()) == 0.0
    if not dataset:  # the C entry point: one address for both gradients is a 3-channel call
        tex4 = torch.zeros(H, W, 4, device=DEV)
        ws = torch.empty((int(_lib.load().gstex_loss_workspace_size(H, W)),), device=DEV, dtype=torch.uint8)
        d = torch.empty(H, W, 4, device=DEV)
        one = torch.ones((), device=DEV)
        with pytest.raises(_lib.GstexError, match="d_tex may be d_img only with C == 3"):
            _lib.call("gstex_loss_bwd", H, W, 4, _lib.ptr(img), _lib.ptr(tex4), _lib.ptr(alpha), _lib.ptr(bg),
                      _lib.ptr(gt), _cwin(), 0.2, one.data_ptr(), _lib.ptr(d), _lib.ptr(d), _lib.ptr(alpha.clone()),
                      _lib.ptr(ws), ws.numel(), _lib.stream_of(img.device))


def test_fused_step_selects_train_and_matches_unshared(monkeypatch):
    """One GStexTrainer.forward_backward at 500 splats / 64 x 64 through the fused step: the loss hands the raster
    backward one gradient tensor and the call selects TRAIN; with shared_grad=False it selects the generic build; the
    parameter gradients of the two agree by the parity criterion."""
    from gstex_amd import _lib
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    dev = torch.device("cuda", 0)
    sc = make_scene(500, 10_000, seed=5)
    views = [sphere_view(i, 64, 64).to(dev) for i in range(2)]
    gen = torch.Generator().manual_seed(2)
    gts = [torch.rand((64, 64, 3), generator=gen).to(dev) for _ in range(2)]
    seen = _record_variants(monkeypatch)
    grads = {}
    for shared in (True, False):
        tr = GStexTrainer(sc, dev, start_step=3000, defer_texture=True, fused_step=True, shared_grad=shared)
        tr.zero_grad()
        tr.forward_backward(views[0], gts[0])  # sizes the pair capacity (per-op path)
        tr.optimizer_step()
        tr.wait_texture()
        assert tr._fused_ok(False, None)
        del seen[:]
        tr.zero_grad()
        tr.forward_backward(views[1], gts[1])
        torch.cuda.synchronize()
        assert seen == [_lib.BWD_TRAIN if shared else _lib.BWD_GENERIC]
        grads[shared] = {name: ps[0].grad.detach().double().cpu() for name, ps in tr.param_groups().items()
                         if ps[0].grad is not None}
    assert grads[True].keys() == grads[False].keys() and {"texture_dc", "xyz"} <= grads[True].keys()
    for name, a in grads[True].items():
        err = grad_norm_err(a, grads[False][name])
        assert err <= GRAD_RTOL, f"{name}: shared vs unshared gradient {err:.3e} > {GRAD_RTOL:.0e}"
