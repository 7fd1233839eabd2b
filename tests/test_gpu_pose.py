"""Camera pose gradients on the GPU: gstex_raster_viewmat_bwd (the raster's and get_aabb_2d's view-matrix gradient),
gstex_sh_dirs_bwd (the SH view-direction gradient) and the path from GStexTrainer.forward_backward to
PoseRefiner.pose_adjustment, each against the CPU oracle's fp64 autograd at the project's gradient tolerance
(helpers.GRAD_RTOL = 1e-5, norm-wise and max-element relative).  Needs an MI355X."""
import math

import pytest
import torch

import gstex_cuda
from gstex_amd import ops
from gstex_amd.activations import sh_rest
from gstex_amd.model import GStexTrainer, _gauss_window
from gstex_amd.pose import PoseRefiner, corrected_matrices, exp_so3xr3
from gstex_amd.scene import View, make_scene, sphere_view
from helpers import DIFF, GRAD_RTOL, STRESS_CASES, Case, check_stress, grad_norm_err, grad_rel_err, make_case, \
    oracle_run, upstream
from oracle import raster as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
NAMES = ["img", "depth", "reg", "alpha", "tex", "normal"]
NEW_KERNELS = ("gstex_raster_viewmat_bwd", "gstex_sh_dirs_bwd")
# the gradients the deterministic mode makes bitwise reproducible (test_gpu_parity.test_backward_is_deterministic): the
# per-splat sums' chain; the texel gradient is accumulated with float atomics in either mode
BITWISE = ["rgbs", "opacities", "means", "scales", "quats", "centers"]


def _assert_grad(got, ref, what):
    ne, (re, scale) = grad_norm_err(got, ref), grad_rel_err(got, ref)
    print(f"[pose] {what}: norm err {ne:.3e}, max-element rel err {re:.3e} (scale {scale:.3e})")
    assert ne <= GRAD_RTOL and re <= GRAD_RTOL, f"{what}: norm err {ne:.3e}, element err {re:.3e} > {GRAD_RTOL:.0e}"


class _Launches:
    """Counts ops._launch calls by entry-point name."""

    def __enter__(self):
        self.names, self._orig = [], ops._launch

        def counted(name, *a):
            self.names.append(name)
            return self._orig(name, *a)

        ops._launch = counted
        return self

    def __exit__(self, *exc):
        ops._launch = self._orig


# ------------------------------------------------------------------------------------------------ 1. raster
def _intrinsics_case():
    """fx != fy and an off-centre principal point."""
    case = make_case(n=300, n_texels=20000, H=64, W=80, seed=3)
    v0, inp = case.view, case.inp
    v = View(v0.viewmat, v0.c2w, v0.fx * 0.93, v0.fx * 1.11, v0.cx + 5.3, v0.cy - 3.7, v0.H, v0.W)
    cam = O.Camera(v.viewmat, v.fx, v.fy, v.cx, v.cy, v.H, v.W, 16, v.c2w[:3, 3])
    centers, extents = O.aabb_2d(inp.means, inp.scales, inp.glob_scale, inp.quats, cam)
    _, depths = O.project_points(inp.means, cam)
    inp.cam, inp.centers, inp.extents, inp.depths = cam, centers.detach().clone(), extents, depths
    return Case(inp, v, case.C, O.num_tiles_hit(centers, extents, v.H, v.W))


RASTER_CASES = {
    # name: (case builder, the outputs that take an upstream gradient (None: all six))
    "textured": (lambda: make_case(n=300, n_texels=20000, H=64, W=80), None),
    "2dgs": (lambda: make_case(n=300, n_texels=0, H=64, W=80, seed=1), None),
    "photometric": (lambda: make_case(n=300, n_texels=20000, H=64, W=80, seed=2), ("img", "alpha", "tex")),
    "intrinsics": (_intrinsics_case, None),
    # helpers.STRESS_CASES: anisotropic splats, non-square charts, glob_scale 1.4; a camera at the edge of the splat
    # cube, where the view-matrix gradient is largest relative to the depths it divides by
    "aniso": (lambda: make_case(**STRESS_CASES["aniso10_glob"]), None),
    "near": (lambda: make_case(**STRESS_CASES["near1.3"]), None),
}
STRESS = {"aniso": "aniso10_glob", "near": "near1.3"}
_RASTER_REF: dict = {}
_RASTER_FP32: dict = {}  # the oracle's own fp32-autograd error of each reference (the yardstick, not a bound)


def _raster_ref(name):
    """(case, outputs, the oracle's fp64 dL/d(viewmat): the raster's own part and the part through the centres)."""
    if name not in _RASTER_REF:
        build, outputs = RASTER_CASES[name]
        case = build()
        inp, cam0 = case.inp, case.inp.cam
        V = cam0.viewmat.double().clone().requires_grad_(True)
        inp.cam = O.Camera(V, cam0.fx, cam0.fy, cam0.cx, cam0.cy, cam0.H, cam0.W, cam0.block, cam0.campos)
        _, _, aux, og = oracle_run(case, grads=True, outputs=outputs)  # (sets case.flip_mask)
        if name in STRESS:
            check_stress(STRESS[name], case, aux)
        g_raster = V.grad.detach().clone()
        V.grad = None
        c64, _ = O.aabb_2d(inp.means, inp.scales, inp.glob_scale, inp.quats, inp.cam, dtype=F64)
        (c64 * og["centers"].double()).sum().backward()
        g_centres = V.grad.detach().clone()
        V.grad = None
        oracle_run(case, grads=True, grad_dtype=torch.float32, outputs=outputs)
        _RASTER_FP32[name] = (grad_norm_err(V.grad, g_raster), grad_rel_err(V.grad, g_raster)[0])
        V.grad = None
        inp.cam = cam0
        _RASTER_REF[name] = (case, outputs, g_raster, g_centres)
    return _RASTER_REF[name]


def _gpu_raster(case, outputs, fold, pose, through_aabb=False):
    """texture_gaussians forward + backward -> ({name: gradient}, launch names).  pose: viewmat requires a gradient.
    through_aabb: the centres come from get_aabb_2d on the same viewmat leaf (the reference's call sequence)."""
    inp, v = case.inp, case.view
    dv = lambda t: t.detach().to(DEV).contiguous()  # noqa: E731
    t = {k: dv(getattr(inp, k)).requires_grad_(True) for k in DIFF}
    vm = dv(v.viewmat).requires_grad_(pose)
    centers = t["centers"]
    if through_aabb:
        centers, _ = gstex_cuda.get_aabb_2d(t["means"], t["scales"], inp.glob_scale, t["quats"], vm,
                                            (v.fx, v.fy, v.cx, v.cy))
    n = inp.means.shape[0]
    with _Launches() as rec:
        outs = gstex_cuda.texture_gaussians(
            (n, 1, case.C), dv(inp.texture_dims), centers, dv(inp.extents), dv(inp.depths), dv(case.nth),
            t["rgbs"], t["opacities"], t["means"], t["scales"], inp.glob_scale, t["quats"], t["uv0"], dv(inp.umap),
            dv(inp.vmap), t["texture"], vm, dv(v.c2w), v.fx, v.fy, v.cx, v.cy, inp.cam.H, inp.cam.W, 16,
            inp.settings, background=None if inp.background is None else dv(inp.background), fold_aabb=fold)
        up = upstream(inp.cam.H, inp.cam.W, case.C, 5, case.flip_mask)
        sel = [i for i, k in enumerate(NAMES) if outputs is None or k in outputs]
        torch.autograd.backward([outs[i] for i in sel], [up[NAMES[i]].to(DEV) for i in sel])
    gr = {k: (t[k].grad.detach().cpu() if t[k].grad is not None else None) for k in t}
    gr["viewmat"] = vm.grad.detach().cpu() if vm.grad is not None else None
    gr["c2w"] = None
    return gr, rec.names


def _check_raster(name, det):
    case, outputs, g_raster, g_centres = _raster_ref(name)
    print(f"[pose] {name} viewmat (raster part), the oracle's own fp32 autograd: norm err {_RASTER_FP32[name][0]:.3e}, "
          f"max-element rel err {_RASTER_FP32[name][1]:.3e}")
    for fold in (False, True):
        base, base_names = _gpu_raster(case, outputs, fold, pose=False)
        got, names = _gpu_raster(case, outputs, fold, pose=True)
        assert not any(k in base_names for k in NEW_KERNELS), base_names
        assert names.count("gstex_raster_viewmat_bwd") == 1
        assert base["viewmat"] is None and tuple(got["viewmat"].shape) == (3, 4)
        ref = g_raster + g_centres if fold else g_raster
        _assert_grad(got["viewmat"], ref, f"{name} fold_aabb={fold} det={det} viewmat")
        # asking for the pose gradient leaves every other gradient as it was
        for k in DIFF:
            if base[k] is None or got[k] is None:
                assert base[k] is None and got[k] is None, k  # (centers under fold_aabb)
            elif det and k in BITWISE:
                assert torch.equal(base[k], got[k]), f"{name} fold={fold}: {k} changed bits with the pose gradient"
            else:  # float atomics: the two runs' sums differ in order
                assert grad_norm_err(got[k], base[k]) <= GRAD_RTOL, k
    # the reference's call sequence: centres from get_aabb_2d on the same leaf, no fold -> the same total
    got, names = _gpu_raster(case, outputs, False, pose=True, through_aabb=True)
    assert names.count("gstex_raster_viewmat_bwd") == 2  # the raster's and get_aabb_2d's (centre-only mode)
    _assert_grad(got["viewmat"], g_raster + g_centres, f"{name} through get_aabb_2d det={det} viewmat")


@pytest.mark.parametrize("name", list(RASTER_CASES))
def test_raster_viewmat_gradient(name):
    _check_raster(name, det=False)


@pytest.mark.parametrize("name", list(RASTER_CASES))
def test_raster_viewmat_gradient_deterministic(name, deterministic):
    _check_raster(name, det=True)
    # the reduction has no atomics: a second backward gives the same bits
    case, outputs, _, _ = _raster_ref(name)
    a, _ = _gpu_raster(case, outputs, True, pose=True)
    b, _ = _gpu_raster(case, outputs, True, pose=True)
    assert torch.equal(a["viewmat"], b["viewmat"])


def test_viewmat_4x4_input_gets_a_4x4_gradient():
    case, outputs, g_raster, _ = _raster_ref("textured")
    v = case.view
    vm4 = torch.cat([v.viewmat, torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    case4 = Case(case.inp, View(vm4, v.c2w, v.fx, v.fy, v.cx, v.cy, v.H, v.W), case.C, case.nth, case.flip_mask)
    got, _ = _gpu_raster(case4, outputs, False, pose=True)
    assert tuple(got["viewmat"].shape) == (4, 4) and float(got["viewmat"][3].abs().max()) == 0.0
    _assert_grad(got["viewmat"][:3], g_raster, "4x4 viewmat")


# ------------------------------------------------------------------------------------------------ 2. reduction edges
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_centre_only_viewmat_gradient(n):
    """get_aabb_2d's viewmat gradient (the kernel's centre-only mode): one thread, the 256-splat block boundaries,
    many workspace rows; every 7th splat moved behind the camera (culled: no contribution)."""
    sc = make_scene(n, 0, seed=11)
    v = sphere_view(3, 64, 80)
    means, scales, quats, _ = sc.activated()
    means, scales, quats = means.detach().clone(), scales.detach(), quats.detach()
    behind = torch.arange(n) % 7 == 3
    means[behind] = 1.5 * v.c2w[:3, 3] + 0.1 * means[behind]
    g = torch.Generator().manual_seed(n)
    v_centers = torch.randn((n, 2), generator=g)
    intr = (v.fx, v.fy, v.cx, v.cy)

    V = v.viewmat.double().clone().requires_grad_(True)
    cam = O.Camera(V, v.fx, v.fy, v.cx, v.cy, v.H, v.W, 16, v.c2w[:3, 3])
    c64, e64 = O.aabb_2d(means, scales, 1.0, quats, cam, dtype=F64)
    if n >= 255:
        assert bool(behind.any()) and float(e64[behind].abs().max()) == 0.0  # culled
        assert float(e64[~behind].min()) > 0.0
    (c64 * v_centers.double()).sum().backward()

    def run(vc):
        vm = v.viewmat.to(DEV).requires_grad_(True)
        with _Launches() as rec:
            c, _ = ops.get_aabb_2d(means.to(DEV), scales.to(DEV), 1, quats.to(DEV), vm, intr)
            c.backward(vc.to(DEV))
        assert rec.names.count("gstex_raster_viewmat_bwd") == 1
        return vm.grad.detach().cpu()

    got = run(v_centers)
    _assert_grad(got, V.grad, f"centre-only n={n}")
    assert torch.equal(got, run(v_centers))  # no atomics: identical bits
    # culled splats contribute exactly nothing: other upstream values there change no bit
    vc2 = v_centers.clone()
    vc2[behind] = vc2[behind] * 3.0 + 1.0
    assert torch.equal(got, run(vc2))


def test_project_points_viewmat_gradient():
    """project_points chains an arriving xys / depths gradient to viewmat (never dropped)."""
    sc = make_scene(257, 0, seed=12)
    v = sphere_view(2, 64, 80)
    means = sc.means.detach().clone()
    means[::9] = 1.5 * v.c2w[:3, 3]  # behind the camera: clipped
    g = torch.Generator().manual_seed(3)
    gx, gd = torch.randn((257, 2), generator=g), torch.randn((257,), generator=g)
    V = v.viewmat.double().clone().requires_grad_(True)
    xy, d = O.project_points(means, O.Camera(V, v.fx, v.fy, v.cx, v.cy, v.H, v.W, 16, v.c2w[:3, 3]), dtype=F64)
    ((xy * gx.double()).sum() + (d * gd.double()).sum()).backward()
    vm = v.viewmat.to(DEV).requires_grad_(True)
    xy_g, d_g = ops.project_points(means.to(DEV), vm, (v.fx, v.fy, v.cx, v.cy))
    torch.autograd.backward([xy_g, d_g], [gx.to(DEV), gd.to(DEV)])
    _assert_grad(vm.grad.cpu(), V.grad, "project_points viewmat")


# ------------------------------------------------------------------------------------------------ 3. SH directions
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("layout", ["full", "rest"])
@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_sh_direction_gradient(degree, layout, n):
    g = torch.Generator().manual_seed(100 * degree + n)
    dirs = torch.randn((n, 3), generator=g) * (0.5 + torch.rand((n, 1), generator=g))  # not unit length
    K = 25  # every degree gstex_sh_fwd covers
    coeffs = torch.randn((n, K, 3), generator=g)
    if layout == "rest":
        coeffs[:, 0] = 0.0  # the DC term the rest layout leaves out
    v_out = torch.randn((n, 3), generator=g)

    d64 = dirs.double().clone().requires_grad_(True)
    c64 = coeffs.double().clone().requires_grad_(True)
    (O.spherical_harmonics(degree, d64, c64, dtype=F64) * v_out.double()).sum().backward()
    ref_dirs = d64.grad if d64.grad is not None else torch.zeros_like(d64)

    def run(need_dirs):
        d = dirs.to(DEV).requires_grad_(need_dirs)
        c = (coeffs[:, 1:] if layout == "rest" else coeffs).to(DEV).contiguous().requires_grad_(True)
        with _Launches() as rec:
            out = sh_rest(degree, d, c) if layout == "rest" else ops.spherical_harmonics(degree, d, c)
            out.backward(v_out.to(DEV))
        assert rec.names.count("gstex_sh_dirs_bwd") == (1 if need_dirs else 0)
        return (d.grad.cpu() if need_dirs else None), c.grad.cpu()

    gd, gc = run(True)
    if degree == 0:
        assert float(gd.abs().max()) == 0.0 and float(ref_dirs.abs().max()) == 0.0
    else:
        _assert_grad(gd, ref_dirs, f"sh dirs degree={degree} {layout} n={n}")
    _, gc0 = run(False)
    assert torch.equal(gc, gc0)  # asking for v_viewdirs leaves v_coeffs as it was
    ref_c = c64.grad[:, 1:] if layout == "rest" else c64.grad
    assert grad_norm_err(gc, ref_c) <= GRAD_RTOL


# ------------------------------------------------------------------------------------------------ 4. trainer
def _trainer(fused_step=False, **kw):
    sc = make_scene(300, 20000, seed=21, opacity=None)
    return GStexTrainer(sc, DEV, start_step=3000, fused_step=fused_step, **kw)


def _ssim64(x, y):
    """gstex_amd.model.ssim in fp64 (the same window values), on (H, W, 3) images."""
    win = _gauss_window(11, 1.5, "cpu").double()
    k = win.numel()

    def filt(t):  # (C, H, W): separable valid correlation
        t = torch.stack([(t[..., j:t.shape[-1] - k + 1 + j] * win[j]) for j in range(k)], 0).sum(0)
        return torch.stack([(t[..., j:t.shape[-2] - k + 1 + j, :] * win[j]) for j in range(k)], 0).sum(0)

    x, y = x.permute(2, 0, 1), y.permute(2, 0, 1)
    mu1, mu2 = filt(x), filt(y)
    s11, s22, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s11 + s22 + C2))).mean()


def _oracle_pose_grad(tr, base, tangent, gt):
    """d(0.8 L1 + 0.2 (1 - SSIM)) / d(tangent) of the trainer's render at the corrected view, by the oracle in fp64."""
    from gstex_amd.charts import SH2RGB, get_uv_mapping

    c = lambda t: t.detach().cpu()  # noqa: E731
    means = c(tr.means)
    quats = c(tr.quats) / c(tr.quats).norm(dim=-1, keepdim=True)
    s = torch.exp(c(tr.scales)[:, :-1]).clamp(min=1e-9)
    scales = torch.cat([s, 1e-5 * s.mean(dim=-1, keepdim=True)], dim=-1)
    opac = torch.sigmoid(c(tr.opacities))
    uv0, umap, vmap = get_uv_mapping(quats, c(tr.mappings))
    t = tangent.double().clone().requires_grad_(True)
    vm, c2w = corrected_matrices(base.viewmat.double(), base.c2w.double(), exp_so3xr3(t[None])[0])
    campos = c2w[:3, 3]
    cam = O.Camera(vm, base.fx, base.fy, base.cx, base.cy, base.H, base.W, 16, campos)
    cam32 = O.Camera(vm.detach().float(), base.fx, base.fy, base.cx, base.cy, base.H, base.W, 16,
                     campos.detach().float())
    centers, extents = O.aabb_2d(means, scales, 1.0, quats, cam32)
    _, depths = O.project_points(means, cam32)
    centers = centers.detach().clone().requires_grad_(True)
    viewdirs = means.double() - campos  # the dropped-campos check: the SH colour depends on the camera position
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    rest = c(tr.features_rest)
    coeffs = torch.cat([torch.zeros_like(rest[:, :1, :]), rest], 1)
    rgbs = O.spherical_harmonics(tr.sh_degree_now(), viewdirs, coeffs, dtype=F64)
    inp = O.RasterInputs(c(tr.texture_dims), centers, extents, depths, rgbs, opac, means, scales, 1.0, quats, uv0,
                         umap, vmap, SH2RGB(c(tr.texture_dc)), cam, tr.settings, None)
    _, o64, _ = O.rasterize(inp)
    rgb = torch.clamp(o64["img"] + o64["tex"][:, :, 0:3] + (1 - o64["alpha"][:, :, None]) * c(tr.background).double(),
                      0.0, 1.0)
    loss = 0.8 * torch.abs(gt.double() - rgb).mean() + 0.2 * (1 - _ssim64(gt.double(), rgb))
    loss.backward(retain_graph=True)  # (the corrected matrices' graph is walked again below)
    c64, _ = O.aabb_2d(means, scales, 1.0, quats, cam, dtype=F64)
    (c64 * centers.grad.double()).sum().backward()  # the folded centre chain
    return t.grad.detach(), float(loss.detach())


def test_trainer_pose_gradient_matches_the_oracle():
    base = sphere_view(1, 64, 80).to(DEV)
    tangent = torch.tensor([0.02, -0.015, 0.01, 0.012, -0.02, 0.015])
    gt = torch.rand((64, 80, 3), generator=torch.Generator().manual_seed(4))
    grads, losses = {}, {}
    for fused in (False, True):
        tr = _trainer(fused_step=fused, defer_texture=fused)
        if fused:  # a trainer that takes the fused path for a constant view (a first step sizes the pair capacity)
            tr.zero_grad()
            tr.forward_backward(sphere_view(2, 64, 80).to(DEV), gt.to(DEV))
            assert tr._fused_ok(False, None) and tr._fused_ok(False, None, base)
        r = PoseRefiner(2, DEV, accumulate=1)
        with torch.no_grad():
            r.pose_adjustment[1].copy_(tangent.to(DEV))
        tr.zero_grad()
        pose_view = r.view(1, base)
        assert not tr._fused_ok(False, None, pose_view)
        with _Launches() as rec:
            out = tr.forward_backward(pose_view, gt.to(DEV))
        assert rec.names.count("gstex_raster_viewmat_bwd") == 1 and rec.names.count("gstex_sh_dirs_bwd") == 1
        g = r.pose_adjustment.grad.detach().cpu()
        assert float(g[0].abs().max()) == 0.0  # the other view's adjustment is untouched
        grads[fused], losses[fused] = g[1], float(out.loss)
        if not fused:
            ref, ref_loss = _oracle_pose_grad(tr, sphere_view(1, 64, 80), tangent, gt)
    assert abs(losses[False] - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-6
    _assert_grad(grads[False], ref, "trainer pose_adjustment.grad")
    # fused_step=True declines the fused path for a view that requires a gradient: the per-op value
    _assert_grad(grads[True], ref, "trainer (fused_step=True) pose_adjustment.grad")
    assert grad_norm_err(grads[True], grads[False]) <= GRAD_RTOL


def _se3_log_norm(T):
    """|log(T)| of a rigid 4x4 (fp64): the rotation vector and J^-1 t."""
    R, t = T[:3, :3], T[:3, 3]
    th = math.acos(max(-1.0, min(1.0, (float(R.trace()) - 1.0) / 2.0)))
    vee = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    w = vee * (0.5 if th < 1e-6 else th / (2.0 * math.sin(th)))
    K = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=F64)
    B = 0.5 if th < 1e-6 else (1 - math.cos(th)) / th ** 2
    C = 1.0 / 6.0 if th < 1e-6 else (th - math.sin(th)) / th ** 3
    J = torch.eye(3, dtype=F64) + B * K + C * (K @ K)
    return float(torch.cat([torch.linalg.solve(J, t), w]).norm())


def test_pose_refinement_reduces_loss_and_pose_error():
    """Scene frozen; target: the trainer's own render at the true view (sphere_view(1, 64, 80)).  Start: that view
    perturbed by the tangent (0.03, -0.02, 0.02 | 0.012, -0.01, 0.008) (|log| = 0.045); 40 pose-only Adam steps at the
    default lr 1e-3 with accumulate=1 (Adam can move each parameter by at most 0.04).  Both the photometric loss and the
    pose error |log(T_true^-1 T_est)| must end strictly below their step-0 values."""
    tr = _trainer()
    true_view = sphere_view(1, 64, 80).to(DEV)
    with torch.no_grad():
        gt = tr.render(true_view, composite=True)["rgb"].clone()
    pert = PoseRefiner(1, DEV)
    with torch.no_grad():
        pert.pose_adjustment.copy_(torch.tensor([[0.03, -0.02, 0.02, 0.012, -0.01, 0.008]], device=DEV))
    start = pert.view(0, true_view)
    start = View(start.viewmat.detach(), start.c2w.detach(), start.fx, start.fy, start.cx, start.cy, start.H, start.W)
    r = PoseRefiner(1, DEV, accumulate=1)

    def pose_error():
        est = r.view(0, start).c2w.detach().double().cpu()
        return _se3_log_norm(torch.linalg.inv(true_view.c2w.double().cpu()) @ est)

    err0 = pose_error()
    assert abs(err0 - 0.045) < 0.005
    losses = []
    for _ in range(41):  # 40 updates, then the loss at the last pose
        tr.zero_grad()
        out = tr.forward_backward(r.view(0, start), gt)  # (no regulariser: the photometric loss alone)
        losses.append(out.loss)
        if len(losses) <= 40:
            assert r.step() is True
    losses = torch.stack(losses).cpu()
    err1 = pose_error()
    print(f"[pose] refinement: loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}, pose error {err0:.5f} -> {err1:.5f}")
    assert float(losses[-1]) < float(losses[0])
    assert err1 < err0


def test_fit_with_a_pose_refiner():
    """train.fit(pose_refiner=...): each step renders the refiner's view, adds the regulariser and steps the refiner
    after the optimizer; only the visited views' adjustments move."""
    from gstex_amd.train import fit

    tr = _trainer()
    gen = torch.Generator().manual_seed(8)
    pairs = [(sphere_view(i, 64, 80), torch.rand((64, 80, 3), generator=gen)) for i in range(3)]
    r = PoseRefiner(3, DEV, accumulate=1)
    step0 = tr.step
    with _Launches() as rec:
        res = fit(tr, pairs, 2, build_chart_every=0, pose_refiner=r)
    assert rec.names.count("gstex_raster_viewmat_bwd") == 2 and rec.names.count("gstex_sh_dirs_bwd") == 2
    assert tr.step == step0 + 2 and r.steps == 2 and bool(torch.isfinite(res["loss"]).all())
    moved = r.pose_adjustment.detach().abs().amax(dim=-1).cpu() > 0
    assert sorted(set(res["views"])) == torch.nonzero(moved).squeeze(1).tolist() and len(set(res["views"])) == 2
    # two Adam updates at lr <= 1e-3: each is bounded by lr (1 - b1) / sqrt(1 - b2) = 3.2 lr
    p = r.pose_adjustment.detach().abs().cpu()[moved]
    assert bool(torch.isfinite(p).all()) and float(p.max()) <= 2 * 3.2e-3


# ------------------------------------------------------------------------------------------------ 6. no change without it
def test_constant_viewmat_launches_neither_new_kernel(deterministic):
    case, outputs, _, _ = _raster_ref("textured")
    a, names = _gpu_raster(case, outputs, True, pose=False)
    assert not any(k in names for k in NEW_KERNELS), names
    assert names.count("gstex_raster_setup_bwd") == 1 and names.count("gstex_raster_bwd") == 1
    b, _ = _gpu_raster(case, outputs, True, pose=True)
    for k in BITWISE:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    # and the trainer's step on a constant view takes the same path as before: no pose kernels
    tr = _trainer()
    gt = torch.rand((64, 80, 3), generator=torch.Generator().manual_seed(4)).to(DEV)
    tr.zero_grad()
    with _Launches() as rec:
        tr.forward_backward(sphere_view(1, 64, 80).to(DEV), gt)
    assert not any(k in rec.names for k in NEW_KERNELS), rec.names
