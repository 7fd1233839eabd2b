"""The evaluation metrics without a GPU: the C ABI additions (gstex_eval_metrics*) are declared, exported, bound and
reject invalid arguments before any launch; image_metrics refuses bad inputs in Python; image_metrics_eager gives its
known answers on the CPU; evaluate_split averages per image as the reference does."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from gstex_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gstex_hip.h")
NEW = ("gstex_eval_metrics_workspace_size", "gstex_eval_metrics")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------- C ABI
def test_new_symbols_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} is not declared in gstex_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19  # additive


def test_metrics_workspace_size(lib):
    assert lib.gstex_eval_metrics_workspace_size(10, 64) == 0 and lib.gstex_eval_metrics_workspace_size(64, 10) == 0
    # three floats per forward workgroup (4 x 4 tiles x 3 channels) and nothing else: no gmap planes
    assert lib.gstex_eval_metrics_workspace_size(64, 64) == 4 * 4 * 3 * 3 * 4
    assert lib.gstex_eval_metrics_workspace_size(37, 45) == 3 * 3 * 3 * 3 * 4  # partial edge tiles count
    assert lib.gstex_eval_metrics_workspace_size(64, 64) < lib.gstex_loss_target_workspace_size(64, 64)


# host memory standing in for device pointers: compared with NULL and checked for alignment only, every call below is
# rejected before any launch
_BUF = (ctypes.c_float * 8)()


def _target(**kw):
    fake = ctypes.addressof(_BUF)
    base = dict(gt=fake, mask=None, gt_dtype=_lib.GT_U8, gt_channels=4, mask_dtype=_lib.MASK_F32, reserved=0)
    base.update(kw)
    return _lib.GstexLossTarget(**base)


def _metrics(lib, target, H=64, W=64, C=3, ptrs=None, window=True, out=None, ws=None, ws_bytes=0):
    win = (ctypes.c_float * 11)() if window else None
    rc = lib.gstex_eval_metrics(H, W, C, ptrs, ptrs, ptrs, ptrs, ctypes.byref(target) if target else None, win,
                                None, None, None, out, ws, ws_bytes, None)
    return rc, _lib.last_error()


def test_eval_metrics_rejects_invalid_arguments(lib):
    fake = ctypes.addressof(_BUF)
    need = lib.gstex_eval_metrics_workspace_size(64, 64)
    good = dict(ptrs=fake, out=fake, ws=fake, ws_bytes=need)
    cases = [
        (dict(target=None), "null target"),
        (dict(target=_target(gt=None)), "null target gt"),
        (dict(target=_target(gt_dtype=2)), "gt_dtype"),
        (dict(target=_target(gt_dtype=-1)), "gt_dtype"),
        (dict(target=_target(gt_channels=5)), "gt_channels"),
        (dict(target=_target(gt_channels=2)), "gt_channels"),
        (dict(target=_target(gt=fake + 2)), "aligned"),  # an RGBA uint8 pixel is one 32-bit load
        (dict(target=_target(gt=fake + 4, gt_dtype=_lib.GT_F32)), "aligned"),  # an RGBA fp32 pixel is one float4
        (dict(target=_target(mask=fake), **good), "mask"),  # the evaluation applies no mask
        (dict(target=_target(mask=fake, mask_dtype=_lib.MASK_BOOL), **good), "mask"),
        (dict(target=_target(reserved=1), **good), "reserved"),
        (dict(target=_target(), H=10), "window"),
        (dict(target=_target(), W=8), "window"),
        (dict(target=_target(), C=2), "channels"),
        (dict(target=_target(), C=9), "channels"),
        (dict(target=_target()), "null pointer"),  # null images and output
        (dict(target=_target(), **dict(good, out=None)), "null pointer"),  # images given, metrics_out null
        (dict(target=_target(), **dict(good, window=False)), "null pointer"),
        (dict(target=_target(), **dict(good, ws_bytes=need - 1)), "workspace too small"),
        (dict(target=_target(), **dict(good, ws=None, ws_bytes=1 << 20)), "workspace too small"),
    ]
    for kw, word in cases:
        kw = dict(kw)
        rc, msg = _metrics(lib, kw.pop("target"), **kw)
        assert rc == 1 and word in msg and msg.startswith("gstex_eval_metrics:"), (kw, rc, msg)


# ---------------------------------------------------------------- image_metrics refusals (no device is touched)
def _raster_outputs(H=16, W=20, C=3):
    g = torch.Generator().manual_seed(0)
    return (torch.rand(H, W, 3, generator=g), torch.rand(H, W, C, generator=g), torch.rand(H, W, generator=g),
            torch.rand(3, generator=g))


def test_image_metrics_refuses_bad_inputs():
    from gstex_amd.loss import image_metrics

    H, W = 16, 20
    img, tex, alpha, bg = _raster_outputs(H, W)
    u8 = torch.zeros(H, W, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="image_metrics: img must be a CUDA tensor"):
        image_metrics(img, tex, alpha, bg, u8)  # CPU tensors
    with pytest.raises(ValueError, match="image_metrics: img must be a CUDA fp32 tensor of shape"):
        image_metrics(img.double(), tex, alpha, bg, u8)
    with pytest.raises(ValueError, match="image_metrics: background must be a CUDA fp32 tensor of shape"):
        image_metrics(img, tex, alpha, torch.zeros(4), u8)
    with pytest.raises(ValueError, match="image_metrics: alpha must be"):
        image_metrics(img, tex, alpha[..., None], bg, u8)
    with pytest.raises(ValueError, match="image_metrics: tex must be CUDA fp32"):
        image_metrics(img, torch.zeros(H, W, 2), alpha, bg, u8)
    with pytest.raises(ValueError, match="image_metrics: image must be float32 or uint8"):
        image_metrics(img, tex, alpha, bg, torch.zeros(H, W, 3, dtype=torch.int16))
    with pytest.raises(ValueError, match="image_metrics: image must have shape"):
        image_metrics(img, tex, alpha, bg, torch.zeros(H, W, 5))
    with pytest.raises(ValueError, match="image_metrics: image must have shape"):
        image_metrics(img, tex, alpha, bg, torch.zeros(H, W + 1, 3))
    for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 2)[:, 0], [0.0] * 4):
        with pytest.raises(ValueError, match="image_metrics: out must be a contiguous CUDA fp32 tensor of 4"):
            image_metrics(img, tex, alpha, bg, u8, out=bad)
    small = _raster_outputs(10, W)
    with pytest.raises(ValueError, match="image_metrics: the image must be larger than the 11-tap"):
        image_metrics(*small, torch.zeros(10, W, 3, dtype=torch.uint8))


# ---------------------------------------------------------------- image_metrics_eager known answers (CPU)
def test_eager_constant_half_against_128():
    from gstex_amd.loss import image_metrics_eager

    H = W = 16
    rgb = torch.full((H, W, 3), 0.5)
    image = torch.full((H, W, 3), 128, dtype=torch.uint8)
    res = image_metrics_eager(rgb, torch.zeros(3), image)
    assert res.rgb_u8.dtype == torch.uint8 and tuple(res.rgb_u8.shape) == (H, W, 3)
    assert bool((res.rgb_u8 == 127).all())  # 255 * 0.5 = 127.5, truncated
    assert torch.equal(res.rgb, rgb) and torch.equal(res.gt, image.float() / 255.0)
    assert tuple(res.metrics.shape) == (4,) and res.metrics.dtype == torch.float32
    for p in (res.psnr, res.ssim, res.mse, res.mse_raw):
        assert isinstance(p, torch.Tensor) and p.dim() == 0
    # 128/255 and 127/255 are each rounded to fp32 (half an ulp: 3.0e-8 above 0.5, 1.5e-8 below), so their difference
    # is 1/255 to 4.5e-8, 1.15e-5 of it, and its square to twice that; PSNR moves by 10 / ln 10 times the MSE's share
    assert float(res.mse) == pytest.approx((1.0 / 255.0) ** 2, rel=3e-5)
    assert float(res.psnr) == pytest.approx(20.0 * math.log10(255.0), abs=4.343 * 3e-5 + 1e-5)  # 48.1308 dB
    a, b, c1 = 128.0 / 255.0, 127.0 / 255.0, 0.01 ** 2  # two constant images: no variance, cs = C2 / C2 = 1
    # in fp32 the variances E[x^2] - mu^2 of a constant image are rounding noise, not 0: each filtered map is two
    # passes of 11-term sums of values near 0.25 (2 * 11 * 2^-24 relative, 3.3e-7 absolute), so a variance or the
    # covariance is off by up to 6.6e-7 and cs = (2 s12 + C2) / (s11 + s22 + C2) by (2 + 2) * 6.6e-7 / C2 = 2.9e-3
    assert float(res.ssim) == pytest.approx((2 * a * b + c1) / (a * a + b * b + c1), abs=4 * 6.6e-7 / 0.03 ** 2)
    assert float(res.mse_raw) == pytest.approx((0.5 - 128.0 / 255.0) ** 2, rel=1e-4)
    assert torch.equal(res.metrics, torch.stack([res.psnr, res.ssim, res.mse, res.mse_raw]))


def test_eager_every_level_truncates_as_float32():
    from gstex_amd.loss import image_metrics_eager

    k = np.arange(256, dtype=np.float32)
    level = k / np.float32(255.0)  # the float32 nearest k / 255
    want = (np.float32(255.0) * level).astype(np.uint8)  # k, or k - 1 where the product rounds below k
    low = want != k.astype(np.uint8)
    assert np.array_equal(want[low], k.astype(np.uint8)[low] - 1)
    rgb = torch.from_numpy(level).reshape(16, 16, 1).repeat(1, 1, 3)
    image = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1).repeat(1, 1, 3)
    res = image_metrics_eager(rgb, torch.zeros(3), image)
    assert np.array_equal(res.rgb_u8[..., 0].reshape(-1).numpy(), want)
    assert torch.equal(res.rgb_u8[..., 0], res.rgb_u8[..., 1]) and torch.equal(res.rgb_u8[..., 0], res.rgb_u8[..., 2])
    # every byte off by one contributes (1 / 255)^2 to the sum
    assert float(res.mse) == pytest.approx(float(low.sum()) / 256.0 * (1.0 / 255.0) ** 2, rel=1e-4, abs=1e-12)
    if low.any():
        assert math.isfinite(float(res.psnr))
    # the levels whose bytes agree alone (the others replaced by level 0): every byte equals its target, PSNR is inf
    keep = torch.from_numpy(~low).reshape(16, 16, 1)
    res = image_metrics_eager(rgb * keep, torch.zeros(3), image * keep)
    assert torch.equal(res.rgb_u8, image * keep)
    assert float(res.mse) == 0.0 and float(res.psnr) == math.inf


def test_eager_transparent_rgba_is_the_background():
    from gstex_amd.loss import image_metrics_eager

    g = torch.Generator().manual_seed(3)
    rgb, bg = torch.rand(16, 16, 3, generator=g), torch.rand(3, generator=g)
    rgba = torch.randint(0, 256, (16, 16, 4), generator=g, dtype=torch.uint8)
    rgba[..., 3] = 0
    for image in (rgba, rgba.float() / 255.0):
        res = image_metrics_eager(rgb, bg, image)
        assert torch.equal(res.gt, bg[None, None, :].expand(16, 16, 3))
        assert torch.equal(res.mse_raw, ((rgb - res.gt) ** 2).mean())


# ---------------------------------------------------------------- evaluate_split's averaging
def test_evaluate_split_averages_per_image():
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import sphere_view

    mses = [1e-2, 1e-4, 1e-3]
    rows = [[-10.0 * math.log10(m), 0.5 + 0.1 * i, m, 2.0 * m] for i, m in enumerate(mses)]
    calls = []

    def evaluate(view, image, out=None):
        i = len(calls)
        calls.append((view, image))
        out.copy_(torch.tensor(rows[i]))

    stub = types.SimpleNamespace(device=torch.device("cpu"), means=torch.zeros(5, 3), n_texels=7, evaluate=evaluate)
    pairs = [(sphere_view(i, 16, 16), torch.full((16, 16, 3), i, dtype=torch.uint8)) for i in range(3)]
    got = GStexTrainer.evaluate_split(stub, iter(pairs))
    assert len(calls) == 3 and all(int(im[0, 0, 0]) == i for i, (_, im) in enumerate(calls))
    assert "lpips" not in got
    assert set(got) == {"psnr", "ssim", "mse", "mse_raw", "gaussian_count", "texel_count", "per_image"}
    per = got["per_image"]
    assert not per.is_cuda and tuple(per.shape) == (3, 4)
    assert torch.equal(per, torch.tensor(rows))
    mean_of_psnrs = float(per[:, 0].double().mean())
    psnr_of_mean = -10.0 * math.log10(float(per[:, 2].double().mean()))
    assert mean_of_psnrs == pytest.approx(30.0, abs=1e-5) and abs(mean_of_psnrs - psnr_of_mean) > 1.0
    assert got["psnr"] == mean_of_psnrs
    for j, key in enumerate(("psnr", "ssim", "mse", "mse_raw")):
        assert isinstance(got[key], float) and got[key] == float(per[:, j].double().mean())
    assert got["gaussian_count"] == 5.0 and got["texel_count"] == 7.0
    with pytest.raises(ValueError, match="no \\(view, image\\) pairs"):
        GStexTrainer.evaluate_split(stub, [])
