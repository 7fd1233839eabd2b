"""Fused GStex photometric loss (``gstex_loss_fwd`` / ``gstex_loss_bwd``).

``photometric_loss(img, tex, alpha, background, gt)`` is the reference's training loss on the raw
rasterizer outputs: the background composite and clamp (gstex.py:1204-1205) followed by
``0.8 * L1 + 0.2 * (1 - SSIM)`` (gstex.py:1301-1322, pytorch_msssim SSIM, 11-tap sigma-1.5 window,
valid filtering).  One forward launch (+ a one-workgroup reduction) and one backward launch replace
the ~40 elementwise kernels and four GEMMs the same expression costs in eager PyTorch.

``image_loss(img, tex, alpha, background, image, mask=None)`` is the same loss on the image a dataset delivers
(``gstex_loss_target_fwd`` / ``_bwd``): a uint8 or float32 target with 3 or 4 channels, an optional mask, and the
step's MSE (for PSNR) from the same launch; ``image_loss_eager`` restates it with torch ops.

``image_metrics(img, tex, alpha, background, image)`` is one view's evaluation by the reference's protocol
(``gstex_eval_metrics``): PSNR and SSIM of the uint8-quantised render against the composited target, forward only;
``image_metrics_eager`` restates it with torch ops.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import call, ptr

_WINDOWS: dict = {}
_CWIN = None


def _cwin():
    """The 11-tap window as the C array the loss kernels take (built once: no per-step tensor-to-list work)."""
    global _CWIN
    if _CWIN is None:
        _CWIN = (ctypes.c_float * 11)(*(float(x) for x in gaussian_window().numpy()))
    return _CWIN


def gaussian_window(size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """pytorch_msssim._fspecial_gauss_1d, evaluated in fp32 on the CPU."""
    key = (size, sigma)
    w = _WINDOWS.get(key)
    if w is None:
        coords = torch.arange(size, dtype=torch.float32) - size // 2
        g = torch.exp(-(coords**2) / (2 * sigma**2))
        w = (g / g.sum()).contiguous()
        _WINDOWS[key] = w
    return w


def _check_args(fn, img, tex, alpha, background, image, mask=None, gt=False):
    """The arguments of photometric_loss, image_loss and image_metrics.  Shapes and dtypes first, then the window, then
    the device: each refusal names what is wrong with the call.  gt: `image` is photometric_loss's gt, float32
    (H, W, 3) like the render.  Returns the mask as (H, W) (or None)."""
    if alpha.dim() != 2:
        raise ValueError(f"{fn}: alpha must be a CUDA fp32 tensor of shape (H, W)")
    H, W = alpha.shape
    fp32 = [("img", img, (H, W, 3)), ("alpha", alpha, (H, W)), ("background", background, (3,))]
    if gt:
        fp32.insert(2, ("gt", image, (H, W, 3)))
    for name, t, shape in fp32:
        if tuple(t.shape) != shape or t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} must be a CUDA fp32 tensor of shape {shape}")
    if tex.dim() != 3 or tuple(tex.shape[:2]) != (H, W) or not 3 <= tex.shape[2] <= 8 or tex.dtype != torch.float32:
        raise ValueError(f"{fn}: tex must be CUDA fp32 (H, W, C) with 3 <= C <= 8")
    if not gt:
        mask = _check_target(fn, alpha, image, mask)
    if H <= 10 or W <= 10:
        raise ValueError(f"{fn}: the image must be larger than the 11-tap SSIM window")
    for name, t in (("img", img), ("tex", tex), ("alpha", alpha), ("background", background),
                    ("gt" if gt else "image", image), ("mask", mask)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{fn}: {name} must be a CUDA tensor")
    return mask


def _aligned(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    """t, or a fresh copy when its storage offset breaks the kernels' pixel load (an RGBA pixel is one load)."""
    return t if t.data_ptr() % nbytes == 0 else t.clone()


def _prepare(ws_size, img, tex, alpha, background, image, mask=None, image_align=16):
    """What the kernels read: the tensors detached and contiguous, the image and the mask aligned to their loads; and
    the workspace of the size the library's function `ws_size` gives."""
    img, tex, alpha, background = (t.detach().contiguous() for t in (img, tex, alpha, background))
    image = _aligned(image.detach().contiguous(), image_align)
    if mask is not None:
        mask = _aligned(mask.detach().contiguous(), 4)
    H, W = alpha.shape
    ws = torch.empty((int(getattr(_lib.load(), ws_size)(H, W)),), device=img.device, dtype=torch.uint8)
    return img, tex, alpha, background, image, mask, ws


def _loss_target(image, mask) -> _lib.GstexLossTarget:
    return _lib.GstexLossTarget(
        ptr(image), ptr(mask), _lib.GT_U8 if image.dtype == torch.uint8 else _lib.GT_F32, int(image.shape[2]),
        _lib.MASK_BOOL if mask is not None and mask.dtype == torch.bool else _lib.MASK_F32, 0)


def _backward(ctx, g_loss, n_inputs):
    """The backward of both autograd functions: forward saved (img, tex, alpha, background, target, ws[, mask]) and
    set ctx.ssim_lambda and ctx.dataset_target (gstex_loss_target_bwd takes the target as a descriptor)."""
    if g_loss is None:
        return (None,) * n_inputs
    img, tex, alpha, background, image, ws, *rest = ctx.saved_tensors
    H, W = alpha.shape
    C = tex.shape[2]
    d_img = torch.empty_like(img)
    # at C = 3 both gradients are the same image (d_tex[0..2] = d_img): one tensor, written once, which the raster
    # backward recognises by its address (gstex_raster_bwd_variant); ctx.share_grad = False keeps two tensors
    d_tex = d_img if C == 3 and ctx.share_grad else torch.empty_like(tex)
    d_alpha = torch.empty_like(alpha)
    g = g_loss.detach().to(torch.float32).contiguous()
    if ctx.dataset_target:
        target = _loss_target(image, rest[0] if rest else None)
        symbol, gt = "gstex_loss_target_bwd", ctypes.byref(target)
    else:
        symbol, gt = "gstex_loss_bwd", ptr(image)
    call(symbol, H, W, C, ptr(img), ptr(tex), ptr(alpha), ptr(background), gt, _cwin(), ctx.ssim_lambda, g.data_ptr(),
         ptr(d_img), ptr(d_tex), ptr(d_alpha), ptr(ws), ws.numel(), _lib.stream_of(img.device))
    return (d_img, d_tex, d_alpha) + (None,) * (n_inputs - 3)


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, tex, alpha, background, gt, ssim_lambda, share_grad=True):
        _check_args("photometric_loss", img, tex, alpha, background, gt, gt=True)
        img, tex, alpha, background, gt, _, ws = _prepare("gstex_loss_workspace_size", img, tex, alpha, background, gt,
                                                          image_align=4)
        H, W = alpha.shape
        C = tex.shape[2]
        out = torch.empty((3,), device=img.device, dtype=torch.float32)
        rgb = torch.empty((H, W, 3), device=img.device, dtype=torch.float32)
        call("gstex_loss_fwd", H, W, C, ptr(img), ptr(tex), ptr(alpha), ptr(background), ptr(gt), _cwin(),
             float(ssim_lambda), ptr(rgb), ptr(out), ptr(ws), ws.numel(), _lib.stream_of(img.device))
        ctx.save_for_backward(img, tex, alpha, background, gt, ws)
        ctx.ssim_lambda = float(ssim_lambda)
        ctx.share_grad = bool(share_grad)
        ctx.dataset_target = False
        ctx.mark_non_differentiable(rgb)
        ctx.set_materialize_grads(False)  # rgb's (always unused) gradient stays None, no zero image
        return out[0], rgb  # out[1:] = (L1, SSIM) stay readable through the base tensor

    @staticmethod
    def backward(ctx, g_loss, g_rgb):
        return _backward(ctx, g_loss, 7)


def photometric_loss(img, tex, alpha, background, gt, ssim_lambda: float = 0.2, share_grad: bool = True):
    """Returns (loss, rgb): loss is the differentiable 0-dim training loss, rgb the composited image.  share_grad: with
    a 3-channel tex, img and tex receive ONE gradient tensor (the same image; the raster backward then reads it once
    and takes its training build); False gives each its own."""
    return _PhotometricLoss.apply(img, tex, alpha, background, gt, ssim_lambda, share_grad)


# ---------------------------------------------------------------------------------------------------------------
# the loss on the image a dataset delivers: uint8 / RGBA targets and masks (gstex.py:1238-1260, 1277-1303)
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class ImageLoss:
    """What image_loss / image_loss_eager return.  loss: the differentiable 0-dim training loss; rgb: the composited
    (unmasked) render, outputs["rgb"]; gt: the composited unmasked target (H, W, 3); terms: four floats
    [loss, L1, SSIM, MSE] on the device (PSNR = -10 log10(MSE), get_metrics_dict)."""
    loss: torch.Tensor
    rgb: torch.Tensor
    gt: torch.Tensor
    terms: torch.Tensor

    def psnr(self) -> torch.Tensor:
        return -10.0 * torch.log10(self.terms[3])


def _check_target(name, alpha, image, mask):
    """The dataset image and mask (dtypes and shapes), refused in words before any HIP call.  Returns the mask as
    (H, W) (or None)."""
    H, W = alpha.shape
    if image.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name}: image must be float32 or uint8 (got {image.dtype})")
    if image.dim() != 3 or tuple(image.shape[:2]) != (H, W) or image.shape[2] not in (3, 4):
        raise ValueError(f"{name}: image must have shape ({H}, {W}, 3) or ({H}, {W}, 4) (got {tuple(image.shape)})")
    if mask is not None:
        if mask.dtype == torch.uint8:
            raise ValueError(f"{name}: a uint8 mask is ambiguous (0/1 or 0/255?): pass bool or float32")
        if mask.dtype not in (torch.bool, torch.float32):
            raise ValueError(f"{name}: mask must be bool or float32 (got {mask.dtype})")
        if tuple(mask.shape) not in ((H, W), (H, W, 1)):
            raise ValueError(f"{name}: mask must have shape ({H}, {W}) or ({H}, {W}, 1) (got {tuple(mask.shape)})")
        mask = mask.reshape(H, W)
    return mask


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, tex, alpha, background, image, mask, ssim_lambda, share_grad=True):
        mask = _check_args("image_loss", img, tex, alpha, background, image, mask)
        img, tex, alpha, background, image, mask, ws = _prepare("gstex_loss_target_workspace_size", img, tex, alpha,
                                                                background, image, mask)
        H, W = alpha.shape
        C = tex.shape[2]
        dev = img.device
        terms = torch.empty((4,), device=dev, dtype=torch.float32)
        rgb = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
        gt = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
        target = _loss_target(image, mask)
        call("gstex_loss_target_fwd", H, W, C, ptr(img), ptr(tex), ptr(alpha), ptr(background), ctypes.byref(target),
             _cwin(), float(ssim_lambda), ptr(rgb), ptr(gt), ptr(terms), ptr(ws), ws.numel(), _lib.stream_of(dev))
        saved = (img, tex, alpha, background, image, ws) + ((mask,) if mask is not None else ())
        ctx.save_for_backward(*saved)
        ctx.ssim_lambda = float(ssim_lambda)
        ctx.share_grad = bool(share_grad)
        ctx.dataset_target = True
        ctx.mark_non_differentiable(rgb, gt, terms)
        ctx.set_materialize_grads(False)
        return terms[0], rgb, gt, terms

    @staticmethod
    def backward(ctx, g_loss, g_rgb, g_gt, g_terms):
        return _backward(ctx, g_loss, 8)


def image_loss(img, tex, alpha, background, image, mask=None, ssim_lambda: float = 0.2,
               share_grad: bool = True) -> ImageLoss:
    """The training loss of get_loss_dict on the raw rasterizer outputs and the image a dataset delivers, in one
    forward and one backward launch: `image` is float32 or uint8 (v / 255, get_gt_img), (H, W, 3) or (H, W, 4)
    (straight alpha, composited on `background` as composite_with_background does); `mask` is bool or float32,
    (H, W) or (H, W, 1): L1 and SSIM see gt * mask and rgb * mask (gstex.py:1294-1299), the MSE does not.
    `background` is read on the device by the kernels (no host synchronisation).  share_grad: as photometric_loss."""
    loss, rgb, gt, terms = _ImageLoss.apply(img, tex, alpha, background, image, mask, ssim_lambda, share_grad)
    return ImageLoss(loss, rgb, gt, terms)


def _target_eager(image, background):
    """The (H, W, 3) float32 target of a dataset image with torch ops: get_gt_img's v / 255 and
    composite_with_background (gstex.py:1244-1245, 1256-1258)."""
    if image.dtype == torch.uint8:
        # get_gt_img divides on the CPU, a true division.  A tensor divisor gives that on every device: by a Python
        # scalar torch's device kernel multiplies by the rounded reciprocal instead, which is not the division the CPU
        # data path (and the fused kernels) perform
        image = image.float() / torch.full((), 255.0, device=image.device)
    if image.shape[2] == 4:
        a = image[..., -1].unsqueeze(-1).repeat((1, 1, 3))
        return a * image[..., :3] + (1 - a) * background
    return image


def image_loss_eager(rgb, background, image, mask=None, ssim_lambda: float = 0.2) -> ImageLoss:
    """image_loss with torch ops on the composited render `rgb`, restating gstex.py:1244-1245, 1256-1258 and
    1294-1303 (runs on any device; the trainer's fused_loss=False path and the tests' reference)."""
    from .model import ssim  # (model imports this module)

    if rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("image_loss_eager: rgb must have shape (H, W, 3)")
    mask = _check_target("image_loss_eager", rgb[..., 0], image, mask)
    gt = _target_eager(image, background)
    mse = torch.mean((rgb.detach() - gt) ** 2)
    x, y = gt, rgb
    if mask is not None:
        m = mask[..., None]
        x = x * m
        y = y * m
    l1 = torch.abs(x - y).mean()
    sim = ssim(x.permute(2, 0, 1)[None, ...], y.permute(2, 0, 1)[None, ...])
    loss = (1 - ssim_lambda) * l1 + ssim_lambda * (1 - sim)
    terms = torch.stack([loss.detach(), l1.detach(), sim.detach(), mse])
    return ImageLoss(loss, rgb.detach(), gt, terms)


# ---------------------------------------------------------------------------------------------------------------
# one view's evaluation metrics by the reference's protocol (gstex.py:1337-1403): PSNR / SSIM on the uint8 render
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class ImageMetrics:
    """What image_metrics / image_metrics_eager return.  rgb: the composited render, outputs["rgb"] (H, W, 3) float32;
    rgb_u8: its quantisation (255.0 * rgb).to(uint8) (H, W, 3), the bytes the reference writes to its PNGs; gt: the
    composited target (H, W, 3) float32; metrics: four floats [PSNR, SSIM, MSE, MSE_raw] on the device -- PSNR, SSIM
    and MSE of the quantised render (get_image_metrics_and_images), MSE_raw of the unquantised one (get_metrics_dict).
    The properties are 0-dim views of `metrics`: nothing is read back to the host."""
    rgb: torch.Tensor
    rgb_u8: torch.Tensor
    gt: torch.Tensor
    metrics: torch.Tensor

    @property
    def psnr(self) -> torch.Tensor:
        return self.metrics[0]

    @property
    def ssim(self) -> torch.Tensor:
        return self.metrics[1]

    @property
    def mse(self) -> torch.Tensor:
        return self.metrics[2]

    @property
    def mse_raw(self) -> torch.Tensor:
        return self.metrics[3]


def _check_out(fn, out):
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.numel() != 4
                            or not out.is_contiguous()):
        raise ValueError(f"{fn}: out must be a contiguous CUDA fp32 tensor of 4 elements")


@torch.no_grad()
def image_metrics(img, tex, alpha, background, image, out=None) -> ImageMetrics:
    """PSNR, SSIM and MSE of one view as get_image_metrics_and_images takes them (gstex.py:1337-1403), on the raw
    rasterizer outputs and the image a dataset delivers, in one launch pair (gstex_eval_metrics): the composite and
    clamp, the uint8 quantisation of the render (255.0 * rgb).to(uint8).float() / 255.0, the target's conversion and
    alpha composite on `background` (as image_loss; no mask: the reference's evaluation applies none), and the
    reduction to [PSNR, SSIM, MSE, MSE_raw] on the device.  Not differentiable.  `out`: a contiguous CUDA float32
    tensor of 4 elements the metrics are written into (one row of a per-image table)."""
    fn = "image_metrics"
    _check_out(fn, out)
    _check_args(fn, img, tex, alpha, background, image)
    if out is not None and (not out.is_cuda or out.device != img.device):
        raise ValueError(f"{fn}: out must be a contiguous CUDA fp32 tensor of 4 elements on the images' device")
    img, tex, alpha, background, image, _, ws = _prepare("gstex_eval_metrics_workspace_size", img, tex, alpha,
                                                         background, image)
    H, W = alpha.shape
    C = tex.shape[2]
    dev = img.device
    metrics = out if out is not None else torch.empty((4,), device=dev, dtype=torch.float32)
    rgb = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    rgb_u8 = torch.empty((H, W, 3), device=dev, dtype=torch.uint8)
    gt = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    target = _loss_target(image, None)
    call("gstex_eval_metrics", H, W, C, ptr(img), ptr(tex), ptr(alpha), ptr(background), ctypes.byref(target),
         _cwin(), ptr(rgb), ptr(rgb_u8), ptr(gt), ptr(metrics), ptr(ws), ws.numel(), _lib.stream_of(dev))
    return ImageMetrics(rgb, rgb_u8, gt, metrics)


@torch.no_grad()
def image_metrics_eager(rgb, background, image) -> ImageMetrics:
    """image_metrics with torch ops on the composited render `rgb`: the reference's own expressions (get_gt_img and
    composite_with_background, gstex.py:1244-1245, 1256-1258; the quantisation and the metrics, :1375-1384, with
    PeakSignalNoiseRatio(data_range=1) = -10 log10(MSE) and this project's restatement of pytorch_msssim's SSIM).
    Runs on any device; the trainer's fused_loss=False path and the tests' reference."""
    from .model import ssim  # (model imports this module)

    if rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("image_metrics_eager: rgb must have shape (H, W, 3)")
    _check_target("image_metrics_eager", rgb[..., 0], image, None)
    rgb = rgb.detach()
    gt = _target_eager(image, background)
    gt_r = torch.moveaxis(gt, -1, 0)[None, ...]
    pred = torch.moveaxis(rgb, -1, 0)[None, ...]
    q = (255.0 * pred).to(dtype=torch.uint8)
    pred = q.to(dtype=torch.float32) / 255.0
    mse = torch.mean((pred - gt_r) ** 2)
    psnr = -10.0 * torch.log10(mse)
    sim = ssim(gt_r, pred)
    mse_raw = torch.mean((rgb - gt) ** 2)
    metrics = torch.stack([psnr, sim, mse, mse_raw]).to(torch.float32)
    return ImageMetrics(rgb, torch.moveaxis(q[0], 0, -1).contiguous(), gt, metrics)


# ---------------------------------------------------------------------------------------------------------------
# geometry regularisers of get_loss_dict (gstex.py:1313-1317), for a trainer with depth / normal renders
# ---------------------------------------------------------------------------------------------------------------
def depths_to_points(depth: torch.Tensor, viewmat: torch.Tensor, c2w: torch.Tensor, fx: float, fy: float, cx: float,
                     cy: float) -> torch.Tensor:
    """World-space points (H, W, 3) of a rendered depth map, as the reference's depths_to_points
    (gstex.py:122-149): pixel (i, j) looks along the unit world ray of camera direction ((j - cx + 0.5) / fx,
    (i - cy + 0.5) / fy, 1); the depth is view-space z ("don't use view depth", :145-146), so the distance along
    the ray is depth / (the ray's view-space z component)."""
    H, W = depth.shape[0], depth.shape[1]
    dev, f = depth.device, torch.float32
    rows = torch.arange(H, device=dev, dtype=f)[:, None].expand(H, W)
    cols = torch.arange(W, device=dev, dtype=f)[None, :].expand(H, W)
    cam_dir = torch.stack([(cols - cx + 0.5) / fx, (rows - cy + 0.5) / fy, torch.ones_like(rows)], dim=-1)
    world_dir = cam_dir @ c2w[:3, :3].to(f).T
    world_dir = world_dir / (world_dir.norm(dim=-1, keepdim=True) + 1e-9)
    view_z = world_dir @ viewmat[2, :3].to(f)
    dist = depth.reshape(H, W) / view_z
    return c2w[:3, 3].to(f) + dist[..., None] * world_dir


def depth_to_normal(depth: torch.Tensor, viewmat: torch.Tensor, c2w: torch.Tensor, fx: float, fy: float, cx: float,
                    cy: float) -> torch.Tensor:
    """Normals (H, W, 3) estimated from a depth map, as the reference's depth_to_normal (gstex.py:151-161): the unit
    cross product of the central differences of depths_to_points down the rows and along the columns; the one-pixel
    border is zero."""
    p = depths_to_points(depth, viewmat, c2w, fx, fy, cx, cy)
    d_rows = p[2:, 1:-1] - p[:-2, 1:-1]
    d_cols = p[1:-1, 2:] - p[1:-1, :-2]
    out = torch.zeros_like(p)
    out[1:-1, 1:-1] = torch.nn.functional.normalize(torch.linalg.cross(d_rows, d_cols, dim=-1), dim=-1)
    return out


def scheduled(value, step: int) -> float:
    """A loss weight as get_loss_dict reads it (gstex.py:1304-1311): a number, or [before, after, switch_step]."""
    if isinstance(value, (int, float)):
        return float(value)
    return float(value[1] if step >= value[2] else value[0])


def geometry_loss(alpha: torch.Tensor, normal: torch.Tensor, estimated_normal: torch.Tensor, reg: torch.Tensor,
                  lambda_normal: float, lambda_reg: float) -> torch.Tensor:
    """normal_loss + reg_loss of get_loss_dict (gstex.py:1316-1317): lambda_normal * mean(alpha - <n, n_est>) +
    lambda_reg * mean(reg)."""
    loss = alpha.new_zeros(())
    if lambda_normal != 0.0:
        loss = loss + lambda_normal * torch.mean(alpha.reshape(alpha.shape[0], alpha.shape[1])
                                                 - torch.sum(normal * estimated_normal, dim=-1))
    if lambda_reg != 0.0:
        loss = loss + lambda_reg * torch.mean(reg)
    return loss
