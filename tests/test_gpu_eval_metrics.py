"""The evaluation metrics on the GPU: gstex_eval_metrics (through gstex_amd.loss.image_metrics) against the eager
restatement of the reference's protocol (image_metrics_eager), and GStexTrainer.evaluate / evaluate_split.

Shapes: 37x45 (partial edge tiles; 3 x 3 tiles x 3 channels = 27 forward workgroups, so the XCD remap has a
remainder) and 11x12 (1 x 2 valid SSIM positions); 300x290 (19 x 19 tiles x 3 channels = 1083 partial records, partial
edge tiles on both axes) in one case, where the reduction's strided loop takes a second pass with a ragged tail: there
the eager twin's own fp32 metrics lie within 2e-8 (PSNR: 3.3e-7) of their fp64 evaluation (on the CPU, this seed),
well inside a quarter of the bounds below.  SSIM and the MSEs carry the loss terms' tolerance of
test_image_loss_matches_eager (2e-6 * max(1, |want|)); PSNR = -10 log10(MSE) carries that bound propagated:
10 / ln 10 = 4.343 times the MSE's relative tolerance, plus 2 fp32 ulps of the PSNR for log10f and the rounding."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(37, 45), (11, 12)]
LARGE = (300, 290)
TOL = 2e-6


def _levels(n):
    """n byte levels k for a render of exactly k / 255: first those whose fp32 product 255 * (k / 255) rounds below k
    (the truncation then gives k - 1), then the rest."""
    k = np.arange(256, dtype=np.float32)
    low = (np.float32(255.0) * (k / np.float32(255.0))).astype(np.uint8) != k.astype(np.uint8)
    order = np.concatenate([np.nonzero(low)[0], np.nonzero(~low)[0][::7]])
    return torch.from_numpy(order[np.arange(n) % len(order)].astype(np.float32))


def _raster_outputs(H, W, C, seed):
    """As test_gpu_image_loss: img reaches outside [0, 1], a 5x5 block saturated at 1; plus a strip (row 6) whose
    composite is exactly k / 255 (alpha = 1 and a zero texture: (k / 255 + 0) + 0 * bg)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(H, W, 3, generator=g) * 1.4 - 0.2
    tex = torch.rand(H, W, C, generator=g) * 0.3
    alpha = torch.rand(H, W, generator=g)
    bg = torch.rand(3, generator=g)
    img[:5, :5] = 2.0
    img[6] = (_levels(W) / 255.0)[:, None]
    tex[6] = 0.0
    alpha[6] = 1.0
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


def _composite(img, tex, alpha, bg):
    return torch.clamp(img + tex[:, :, 0:3] + (1 - alpha[:, :, None]) * bg[None, None, :], 0.0, 1.0)


def _check_metrics(got, want):
    """got, want: [PSNR, SSIM, MSE, MSE_raw] as Python floats."""
    print("metrics", got, want)
    for name, a, b in zip(("SSIM", "MSE", "MSE_raw"), got[1:], want[1:]):
        assert abs(a - b) <= TOL * max(1.0, abs(b)), f"{name}: {a!r} vs {b!r}"
    mse_tol = TOL * max(1.0, abs(want[2]))
    psnr_tol = 4.343 * (mse_tol / want[2]) + 2.0 * float(np.spacing(np.float32(abs(want[0]))))
    print("PSNR tolerance", psnr_tol)
    assert abs(got[0] - want[0]) <= psnr_tol, f"PSNR: {got[0]!r} vs {want[0]!r} (tolerance {psnr_tol:.3e})"


# the cross product over SHAPES (ids as a stack of parametrize decorators gives them), and LARGE once
_EAGER_CASES = [pytest.param(shape, C, dtype, channels, id=f"shape{i}-{C}-{dtype}-{channels}")
                for i, shape in enumerate(SHAPES) for C in (3, 4) for dtype in ("f32", "u8") for channels in (3, 4)]
_EAGER_CASES.append(pytest.param(LARGE, 4, "u8", 4, id="300x290-4-u8-4"))


@pytest.mark.parametrize("shape,C,dtype,channels", _EAGER_CASES)
def test_image_metrics_matches_eager(shape, C, dtype, channels):
    from gstex_amd.loss import image_loss, image_metrics, image_metrics_eager

    H, W = shape
    seed = 7 * H + C
    img, tex, alpha, bg = (t.to(DEV) for t in _raster_outputs(H, W, C, seed))
    image = _image(H, W, dtype, channels, seed).to(DEV)
    res = image_metrics(img, tex, alpha, bg, image)
    ref = image_metrics_eager(_composite(img, tex, alpha, bg), bg, image)

    assert res.rgb_u8.dtype == torch.uint8 and tuple(res.rgb_u8.shape) == (H, W, 3)
    assert torch.equal(res.rgb, ref.rgb), "the composite must match the eager expression bit for bit"
    assert torch.equal(res.gt, ref.gt), "the target must match the eager conversion and composite bit for bit"
    assert torch.equal(res.rgb_u8, ref.rgb_u8), "the quantised bytes must match (255.0 * rgb).to(uint8)"
    # the strip holds its levels: k, or k - 1 where 255 * (k / 255) rounds below k
    k = _levels(W)
    want_q = (np.float32(255.0) * (k.numpy() / np.float32(255.0))).astype(np.uint8)
    assert np.array_equal(res.rgb_u8[6, :, 0].cpu().numpy(), want_q)
    assert bool((res.rgb_u8[:5, :5] == 255).all())
    _check_metrics(res.metrics.tolist(), ref.metrics.tolist())
    for prop, j in (("psnr", 0), ("ssim", 1), ("mse", 2), ("mse_raw", 3)):
        v = getattr(res, prop)
        assert v.is_cuda and v.dim() == 0 and float(v) == float(res.metrics[j])
    # the unquantised MSE is the training step's (image_loss terms[3], no mask)
    terms = image_loss(img, tex, alpha, bg, image).terms.tolist()
    assert abs(float(res.mse_raw) - terms[3]) <= TOL * max(1.0, abs(terms[3]))


def test_image_metrics_out_row_and_offset_view():
    from gstex_amd.loss import image_metrics

    H, W = 11, 12
    img, tex, alpha, bg = (t.to(DEV) for t in _raster_outputs(H, W, 3, 5))
    image = _image(H, W, "u8", 4, 5).to(DEV)
    want = image_metrics(img, tex, alpha, bg, image)
    table = torch.full((3, 4), -7.0, device=DEV)
    got = image_metrics(img, tex, alpha, bg, image, out=table[1])
    assert got.metrics.data_ptr() == table[1].data_ptr()
    assert torch.equal(table[1], want.metrics)
    assert bool((table[0] == -7.0).all()) and bool((table[2] == -7.0).all())
    # an image whose storage offset breaks the pixel load's alignment is copied, not misread
    flat = torch.zeros(H * W * 4 + 3, dtype=torch.uint8, device=DEV)
    flat[3:] = image.reshape(-1)
    off = image_metrics(img, tex, alpha, bg, flat[3:].view(H, W, 4))
    assert torch.equal(off.metrics, want.metrics) and torch.equal(off.gt, want.gt)
    assert torch.equal(off.rgb_u8, want.rgb_u8)


# ---------------------------------------------------------------- trainer
H, W = 48, 56


@pytest.fixture(scope="module")
def scene():
    from gstex_amd.scene import make_scene

    return make_scene(500, 10_000, seed=2)


def _rgba(seed, h=H, w=W):
    g = torch.Generator().manual_seed(seed)
    rgba = torch.randint(0, 256, (h, w, 4), generator=g, dtype=torch.uint8)
    rgba[:10, :, 3] = 0
    rgba[30:, :, 3] = 255
    return rgba


def test_evaluate_is_eval_renders_image_scored_by_the_protocol(scene):
    from gstex_amd.loss import image_metrics_eager
    from gstex_amd.model import VIEWER_BACKGROUND, GStexTrainer
    from gstex_amd.scene import sphere_view

    view = sphere_view(0, H, W).to(DEV)
    image = _rgba(4).to(DEV)
    kw = dict(background="random", background_seed=5, start_step=3000)
    tr = GStexTrainer(scene, DEV, **kw)
    tr.refresh_background()  # the step's colour is not the evaluation's
    res = tr.evaluate(view, image)
    assert torch.equal(res.rgb, tr.eval_render(view)["rgb"])
    viewer = torch.tensor(VIEWER_BACKGROUND, device=DEV)
    assert torch.equal(res.gt[:10], viewer.expand(10, W, 3))  # a transparent target pixel is the viewer colour
    ref = image_metrics_eager(res.rgb, viewer, image)
    assert torch.equal(res.gt, ref.gt) and torch.equal(res.rgb_u8, ref.rgb_u8)
    _check_metrics(res.metrics.tolist(), ref.metrics.tolist())
    eager = GStexTrainer(scene, DEV, fused_loss=False, **kw)
    table = torch.zeros(2, 4, device=DEV)
    res_eager = eager.evaluate(view, image, out=table[1])
    assert torch.equal(res_eager.rgb_u8, res.rgb_u8) and torch.equal(res_eager.rgb, res.rgb)
    assert torch.equal(table[1], ref.metrics) and res_eager.metrics.data_ptr() == table[1].data_ptr()
    assert bool((table[0] == 0).all())


def test_evaluate_leaves_the_training_state_alone(scene):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import sphere_view

    view = sphere_view(1, H, W).to(DEV)
    image = _rgba(6).to(DEV)
    tr = GStexTrainer(scene, DEV, background="random", background_seed=5, start_step=3000)
    for _ in range(2):  # (the second step takes the fused render: the pair capacity is known by then)
        tr.zero_grad()
        tr.forward_backward(view, image)
        params = tr.parameters()
        grads = [p.grad for p in params]
        before = dict(step=tr.step, params=[p.detach().clone() for p in params],
                      grads=[None if g is None else g.clone() for g in grads], background=tr.background.clone(),
                      gen=tr._background_gen.get_state().clone(), texel_grad=tr.texel_grad.state(),
                      skipped=list(tr.skipped_steps),
                      capacity=None if tr.pairs is None else tr.pairs.capacity, control=tr.step_control.clone())
        res = tr.evaluate(view, image)
        assert torch.isfinite(res.metrics).all()
        assert tr.step == before["step"]
        assert all(a is b for a, b in zip(tr.parameters(), params))
        assert all(p.grad is g for p, g in zip(params, grads))
        assert all(torch.equal(p.detach(), q) for p, q in zip(params, before["params"]))
        assert all((g is None and q is None) or torch.equal(g, q) for g, q in zip(grads, before["grads"]))
        assert any(g is not None and float(g.abs().max()) > 0 for g in grads)
        assert torch.equal(tr.background, before["background"])
        assert torch.equal(tr._background_gen.get_state(), before["gen"])
        assert tr.texel_grad.state() == before["texel_grad"]
        assert tr.skipped_steps == before["skipped"]
        assert (None if tr.pairs is None else tr.pairs.capacity) == before["capacity"]
        assert torch.equal(tr.step_control, before["control"])
        tr.optimizer_step()
        assert tr.step == before["step"] + 1
    assert tr.skipped_steps == []


def test_evaluate_runs_a_pending_texel_update(scene):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import sphere_view

    view = sphere_view(1, H, W).to(DEV)
    image = _rgba(6).to(DEV)
    tr = GStexTrainer(scene, DEV, defer_texture=True, start_step=3000)
    assert tr.defer_texture
    tr.zero_grad()
    tr.forward_backward(view, image)
    tr.optimizer_step()
    assert tr._pending_tex is not None
    stale = tr.texture_dc.detach().clone()  # (read directly: texels() would run the update)
    step = tr.step
    first = tr.evaluate(view, image)
    assert tr._pending_tex is None and tr.step == step
    assert not torch.equal(tr.texture_dc.detach(), stale)  # the update ran before the render
    tr.wait_texture()
    again = tr.evaluate(view, image)
    assert torch.equal(first.rgb, again.rgb) and torch.equal(first.metrics, again.metrics)


def test_evaluate_split(scene, tmp_path):
    from PIL import Image

    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import sphere_view

    g = torch.Generator().manual_seed(8)
    pairs = [(sphere_view(0, H, W), _rgba(1)),  # on the CPU, as load_blender yields them
             (sphere_view(1, H, W), torch.rand(H, W, 3, generator=g)),
             (sphere_view(2, H, W), _rgba(2)[..., :3].contiguous())]
    tr = GStexTrainer(scene, DEV, background="random", start_step=3000)
    got = tr.evaluate_split(pairs, output_dir=tmp_path)
    assert "lpips" not in got
    per = got["per_image"]
    assert not per.is_cuda and tuple(per.shape) == (3, 4) and bool(torch.isfinite(per).all())
    singles = [tr.evaluate(v.to(DEV), im.to(DEV)) for v, im in pairs]
    for i, res in enumerate(singles):
        assert torch.equal(per[i], res.metrics.cpu()), i
        png = np.asarray(Image.open(tmp_path / f"{i:06d}-img.png"))
        want = torch.cat([(res.gt * 255).byte(), res.rgb_u8], dim=1).cpu().numpy()
        assert png.shape == (H, 2 * W, 3) and np.array_equal(png, want), i
    for j, key in enumerate(("psnr", "ssim", "mse", "mse_raw")):
        assert got[key] == float(per[:, j].double().mean())
    assert got["gaussian_count"] == float(tr.means.shape[0]) and got["texel_count"] == float(tr.n_texels)
    assert tr.evaluate_split(pairs)["per_image"].equal(per)  # without output_dir: the same table
