"""The fused loss on dataset targets (gstex_loss_target_fwd / _bwd through gstex_amd.loss.image_loss) on the GPU:
uint8 / RGBA targets and bool / float masks against the eager restatement of the reference (image_loss_eager), the
cases where it must reproduce photometric_loss bit for bit, and the trainer's step on an RGBA uint8 image with a mask
and a random background.

Shapes: 37x45 (partial edge tiles; 3 x 3 tiles x 3 channels = 27 forward workgroups, so the XCD remap has a
remainder) and 11x12 (1 x 2 valid SSIM positions); 300x290 (19 x 19 tiles x 3 channels = 1083 partial records, partial
edge tiles on both axes) in one case each, where the reduction's strided loop takes a second pass with a ragged tail.
Tolerances are those of test_fused_loss_matches_eager_torch; at 300x290 the eager twin's own fp32 terms lie within
2.1e-8 of their fp64 evaluation (on the CPU, this seed), well inside a quarter of the 2e-6 bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(37, 45), (11, 12)]
LARGE = (300, 290)


def _raster_outputs(H, W, C, seed):
    """img reaches outside [0, 1] (the clamp gates gradients); a 5x5 block saturated at 1 (ties with a target of 1)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(H, W, 3, generator=g) * 1.4 - 0.2
    tex = torch.rand(H, W, C, generator=g) * 0.3
    alpha = torch.rand(H, W, generator=g)
    bg = torch.rand(3, generator=g)
    img[:5, :5] = 2.0
    return img, tex, alpha, bg


def _image(H, W, dtype, channels, seed):
    """The target: 1 (255) in the 5x5 tie block; RGBA alpha is a mix of 0, 1 and values between."""
    g = torch.Generator().manual_seed(100 + seed)
    u8 = torch.randint(0, 256, (H, W, channels), generator=g, dtype=torch.uint8)
    if channels == 4:
        pick = torch.rand(H, W, generator=g)
        u8[..., 3][pick < 0.25] = 0
        u8[..., 3][pick > 0.75] = 255
    u8[:5, :5] = 255
    if dtype == "u8":
        return u8
    f = torch.rand(H, W, channels, generator=g)
    if channels == 4:
        f[..., 3] = u8[..., 3].float() / 255.0  # exact 0 and 1 among the alphas
    f[:5, :5] = 1.0
    return f


def _mask(H, W, kind, seed):
    """About 30 % false, plus one fully false tile-aligned 16x16 block where the image holds one."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(200 + seed)
    keep = torch.rand(H, W, generator=g) >= 0.3
    if H >= 32 and W >= 32:
        keep[16:32, 16:32] = False
    if kind == "bool":
        return keep
    return torch.rand(H, W, generator=g) * keep  # float values in [0, 1], exact zeros where not kept


def _eager(leaves, bg, image, mask, upstream=1.7):
    from gstex_amd.loss import image_loss_eager

    img, tex, alpha = leaves
    rgb = torch.clamp(img + tex[:, :, 0:3] + (1 - alpha[:, :, None]) * bg[None, None, :], 0.0, 1.0)
    ref = image_loss_eager(rgb, bg, image, mask)
    ref.loss.backward(torch.tensor(upstream, device=DEV))
    return ref


# the cross product over SHAPES (ids as a stack of parametrize decorators gives them), and LARGE once
_EAGER_CASES = [pytest.param(shape, C, dtype, channels, mask_kind, id=f"shape{i}-{C}-{dtype}-{channels}-{mask_kind}")
                for i, shape in enumerate(SHAPES) for C in (3, 4) for dtype in ("f32", "u8") for channels in (3, 4)
                for mask_kind in ("none", "bool", "f32")]
_EAGER_CASES.append(pytest.param(LARGE, 4, "u8", 4, "bool", id="300x290-4-u8-4-bool"))


@pytest.mark.parametrize("shape,C,dtype,channels,mask_kind", _EAGER_CASES)
def test_image_loss_matches_eager(shape, C, dtype, channels, mask_kind):
    from gstex_amd.loss import image_loss

    H, W = shape
    seed = 7 * H + C
    img, tex, alpha, bg = _raster_outputs(H, W, C, seed)
    image = _image(H, W, dtype, channels, seed).to(DEV)
    mask = _mask(H, W, mask_kind, seed)
    mask = None if mask is None else mask.to(DEV)
    bg = bg.to(DEV)
    leaves = [t.to(DEV).requires_grad_(True) for t in (img, tex, alpha)]
    res = image_loss(leaves[0], leaves[1], leaves[2], bg, image, mask)
    res.loss.backward(torch.tensor(1.7, device=DEV))
    ref_leaves = [t.to(DEV).requires_grad_(True) for t in (img, tex, alpha)]
    ref = _eager(ref_leaves, bg, image, mask)

    assert torch.equal(res.rgb, ref.rgb), "the composite must match the eager expression bit for bit"
    assert torch.equal(res.gt, ref.gt), "the target must match the eager conversion and composite bit for bit"
    got, want = res.terms.tolist(), ref.terms.tolist()
    print("terms", got, want)
    assert float(res.loss) == got[0]
    for name, a, b in zip(("loss", "L1", "SSIM", "MSE"), got, want):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), f"{name}: {a!r} vs {b!r}"
    m = None if mask is None else mask.float()
    for a, b, name in zip(leaves, ref_leaves, ("img", "tex", "alpha")):
        err = float((a.grad - b.grad).abs().max())
        scale = float(b.grad.abs().max())
        print(name, "grad err", err, "scale", scale)
        assert scale > 0.0 and err <= 1e-5 * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"
        if m is not None:  # nothing reaches a pixel the mask removes
            assert float((a.grad.reshape(H, W, -1) * (m == 0)[..., None]).abs().max()) == 0.0, name
    assert float(leaves[1].grad[:, :, 3:].abs().sum()) == 0.0
    if m is not None and H >= 32:
        assert float(leaves[0].grad[16:32, 16:32].abs().max()) == 0.0


_SAME_BITS_CASES = [pytest.param(shape, case, id=f"shape{i}-{case}") for i, shape in enumerate(SHAPES)
                    for case in ("f32", "u8", "u8_rgba_opaque", "all_true_mask")]
_SAME_BITS_CASES.append(pytest.param(LARGE, "f32", id="300x290-f32"))


@pytest.mark.parametrize("shape,case", _SAME_BITS_CASES)
def test_image_loss_reproduces_photometric_loss(shape, case):
    """Where the target policy adds no arithmetic (or only multiplications by 1 and additions of 0), the template's
    instantiations give photometric_loss's bits: rgb, the loss and the three gradients.  (At 300x290 the two- and the
    three-column reductions are compared over more than one pass of their strided loop.)"""
    from gstex_amd.loss import image_loss, photometric_loss

    H, W = shape
    C = 4
    img, tex, alpha, bg = _raster_outputs(H, W, C, 11 * H)
    u8 = _image(H, W, "u8", 3, H)
    # u8.float() / 255 as the CPU data path divides (on the device torch multiplies by the rounded reciprocal of a
    # Python scalar divisor, which is not v / 255 for every byte value)
    as_float = (u8.float() / 255).to(DEV)
    mask = None
    if case == "f32":
        image = as_float
    elif case == "u8":
        image = u8.to(DEV)
    elif case == "u8_rgba_opaque":
        image = torch.cat([u8, torch.full((H, W, 1), 255, dtype=torch.uint8)], -1).to(DEV)
    else:
        image, mask = u8.to(DEV), torch.ones(H, W, dtype=torch.bool, device=DEV)
    bg = bg.to(DEV)
    up = torch.tensor(1.7, device=DEV)
    a = [t.to(DEV).requires_grad_(True) for t in (img, tex, alpha)]
    res = image_loss(a[0], a[1], a[2], bg, image, mask)
    res.loss.backward(up)
    b = [t.to(DEV).requires_grad_(True) for t in (img, tex, alpha)]
    loss, rgb = photometric_loss(b[0], b[1], b[2], bg, as_float)
    loss.backward(up)
    assert torch.equal(res.gt, as_float)
    assert torch.equal(res.rgb, rgb)
    assert torch.equal(res.loss.detach(), loss.detach()), (float(res.loss), float(loss))
    for x, y, name in zip(a, b, ("img", "tex", "alpha")):
        assert torch.equal(x.grad, y.grad), f"{name}: max diff {float((x.grad - y.grad).abs().max()):.3e}"


def test_image_loss_takes_offset_views_and_hw1_masks():
    """An image or mask whose storage offset breaks the pixel load's alignment is copied, not misread."""
    from gstex_amd.loss import image_loss

    H, W = 11, 12
    img, tex, alpha, bg = (t.to(DEV) for t in _raster_outputs(H, W, 3, 5))
    image = _image(H, W, "u8", 4, 5).to(DEV)
    mask = _mask(H, W, "bool", 5).to(DEV)
    want = image_loss(img, tex, alpha, bg, image, mask)
    flat = torch.zeros(H * W * 4 + 3, dtype=torch.uint8, device=DEV)
    flat[3:] = image.reshape(-1)
    got = image_loss(img, tex, alpha, bg, flat[3:].view(H, W, 4), mask[..., None])
    assert torch.equal(got.terms, want.terms) and torch.equal(got.gt, want.gt)


# ---------------------------------------------------------------- trainer
def _grads_match(a, b):
    for (name, pa), pb in zip(a.param_groups().items(), b.param_groups().values()):
        ga, gb = pa[0].grad, pb[0].grad
        if ga is None and gb is None:
            continue
        # the texel gradients are float-atomic sums (order varies run to run); every splat gradient is reproducible
        tol = 1e-5 * float(gb.abs().max()) if name == "texture_dc" else 0.0
        assert float((ga - gb).abs().max()) <= tol, name


def test_trainer_step_on_rgba_uint8_with_mask_and_random_background():
    from gstex_amd.loss import image_loss, photometric_loss
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    H, W = 96, 112
    sc = make_scene(3000, 60_000, seed=9)
    view = sphere_view(1, H, W).to(DEV)
    g = torch.Generator().manual_seed(4)
    rgba = torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8)
    rgba[:20, :, 3] = 0
    rgba[40:, :, 3] = 255
    rgba = rgba.to(DEV)
    mask = (torch.rand(H, W, generator=g) >= 0.3).to(DEV)
    gt_f32 = torch.rand((H, W, 3), generator=g).to(DEV)
    kw = dict(start_step=3000, background="random", background_seed=5)
    auto, manual = GStexTrainer(sc, DEV, **kw), GStexTrainer(sc, DEV, **kw)
    reg = GStexTrainer(sc, DEV, lambda_reg=0.02, **kw)
    plain, parent = GStexTrainer(sc, DEV, start_step=3000), GStexTrainer(sc, DEV, start_step=3000)
    eager = GStexTrainer(sc, DEV, fused_loss=False, **kw)
    torch.use_deterministic_algorithms(True)  # splat gradients bitwise reproducible (row mode)
    try:
        auto.zero_grad()
        res = auto.forward_backward(view, rgba, mask=mask)
        bg1 = auto.background.clone()
        manual.zero_grad()
        manual.refresh_background()
        out = manual.render(view, sh_degree_now=manual.sh_degree_now(), composite=False)
        r = image_loss(out["img"], out["tex"], out["alpha"], manual.background, rgba, mask)
        r.loss.backward()
        # a second step draws another background; the same seed gives the same sequence
        auto.zero_grad()
        res2 = auto.forward_backward(view, rgba, mask=mask)
        bg2 = auto.background.clone()
        # the 2DGS regulariser on top (unmasked, eager, gstex.py:1316-1317)
        reg.zero_grad()
        res_reg = reg.forward_backward(view, rgba, mask=mask)
        # fused_loss=False: the eager twin on the render's own composite
        eager.zero_grad()
        res_eager = eager.forward_backward(view, rgba, mask=mask)
        # a float32 three-channel target without a mask is the parent's step
        plain.zero_grad()
        res_plain = plain.forward_backward(view, gt_f32)
        parent.zero_grad()
        pout = parent.render(view, sh_degree_now=parent.sh_degree_now(), composite=False)
        ploss, _ = photometric_loss(pout["img"], pout["tex"], pout["alpha"], parent.background, gt_f32.contiguous())
        ploss.backward()
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(manual.background, bg1)
    assert torch.isfinite(res.loss) and abs(float(res.loss) - float(r.loss)) <= 1e-6 * max(1.0, abs(float(r.loss)))
    assert torch.equal(res.rgb, r.rgb) and torch.equal(res.terms, r.terms)
    assert auto.step == manual.step
    assert not torch.equal(bg1, bg2) and bool(((bg2 >= 0) & (bg2 < 1)).all())
    assert torch.equal(manual.refresh_background(), bg2)
    assert float(res2.loss) != float(res.loss)
    # (auto's gradients are now those of its second step: compare the first step through a fresh pair instead)
    first = GStexTrainer(sc, DEV, **kw)
    torch.use_deterministic_algorithms(True)
    try:
        first.zero_grad()
        first.forward_backward(view, rgba, mask=mask)
    finally:
        torch.use_deterministic_algorithms(False)
    _grads_match(first, manual)
    # a fully transparent target pixel is the step's background
    assert torch.equal(r.gt[:20], bg1.expand(20, W, 3))
    psnr = -10.0 * torch.log10(res.terms[3])
    assert torch.isfinite(psnr) and float(psnr) > 0.0
    assert float(res.terms[0]) == float(res.loss)
    assert torch.isfinite(res_reg.loss) and float(res_reg.loss) != float(res.loss)
    for got, want in zip(res_eager.terms.tolist(), res.terms.tolist()):
        assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (res_eager.terms, res.terms)
    assert torch.equal(res_eager.rgb, res.rgb)
    assert res_plain.terms is None
    assert torch.equal(res_plain.loss, ploss.detach())
    _grads_match(plain, parent)


def test_eval_render_under_random_background_uses_the_viewer_colour():
    from gstex_amd.model import VIEWER_BACKGROUND, GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    sc = make_scene(500, 10_000, seed=2)
    view = sphere_view(0, 48, 56).to(DEV)
    tr = GStexTrainer(sc, DEV, background="random")
    tr.refresh_background()
    fixed = GStexTrainer(sc, DEV, background=VIEWER_BACKGROUND)
    assert torch.equal(tr.eval_render(view)["rgb"], fixed.eval_render(view)["rgb"])
    assert torch.equal(GStexTrainer(sc, DEV, background="black").background, torch.zeros(3, device=DEV))
    assert torch.equal(GStexTrainer(sc, DEV, background="white").background, torch.ones(3, device=DEV))
