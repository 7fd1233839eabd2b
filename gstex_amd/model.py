"""GStex train-step harness around the HIP rasterizer.

Reproduces the parts of the reference's GStexModel that sit either side of the hot path, so the
"train-step ms" metric is measured on the same work the reference does per step:
  * parameter activations            gstex.py:1059-1066
  * UV frames (detached)             gstex.py:975-990
  * preprocessing                    gstex.py:1077-1080   (project_points / get_aabb_2d / tiles)
  * SH colour with the DC zeroed     gstex.py:1099-1114
  * texture = SH2RGB(texture_dc)     gstex.py:1093-1094,1119
  * texture_gaussians                gstex.py:1133-1162
  * background composite             gstex.py:1204-1205
  * loss 0.8 L1 + 0.2 (1 - SSIM)     gstex.py:1301-1322 (pytorch_msssim SSIM semantics; fused HIP
                                     kernels in gstex_amd.loss, eager torch path kept for reference)
  * the batch image as delivered     gstex.py:1238-1260, 1294-1299 (uint8 / RGBA targets on the step's background,
                                     masks, the step's MSE: inside the same loss kernels, gstex_amd.loss.image_loss)
  * background_color                 gstex.py:178, 1012-1020 ("random": a fresh colour per step, drawn on the device)
  * per-group Adam, eps 1e-15        gstex_configs.py:207-244, engine/optimizers.py:158-171
                                     (one fused HIP launch, gstex_amd.optim.FusedAdam)
The rechart every 100 steps (gstex.py:890-914) is provided by `recharge()`.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch

from . import ops
from .activations import activate, sh_rest
from .loss import (ImageMetrics, depth_to_normal, gaussian_window, geometry_loss, image_loss, image_loss_eager,
                   image_metrics, image_metrics_eager, photometric_loss, scheduled)
from .optim import FusedAdam
from .charts import RGB2SH, SH2RGB, SH_C0, build_charts, get_uv_mapping, texture_dims_to_query
from .scene import Scene, View
from .texel_grad import TexelGrad

# gstex-blender-nvs optimizer settings (gstex_configs.py:207-244)
LRS = {
    "xyz": 5 * 1.6e-5,
    "features_dc": 0.0025,
    "features_rest": 0.0025 / 20,
    "opacity": 0.05,
    "scaling": 0.005,
    "rotation": 0.001,
    "texture_dc": 1e-3,
}
DEFAULT_SETTINGS = (1 << 9) | (1 << 10)
BACKGROUNDS = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}  # background_color names (gstex.py:1012-1020)
# the fixed colour a background="random" model renders on outside training (gstex.py:355-358)
VIEWER_BACKGROUND = (0.1490, 0.1647, 0.2157)


def _gauss_window(size=11, sigma=1.5, device=None):
    return gaussian_window(size, sigma).to(device)  # the same fp32 weights the fused kernels use


def _composite(img, tex, alpha, bg):
    """The render on the background `bg` (3,): clamp(img + tex[..., :3] + (1 - alpha) * bg) (gstex.py:1204-1205)."""
    return torch.clamp(img + tex[..., 0:3] + (1 - alpha[..., None]) * bg[None, None, :], 0.0, 1.0)


_BANDS: dict = {}


def _band(n: int, win: torch.Tensor) -> torch.Tensor:
    """(n, n-k+1) banded matrix M with M[i+j, i] = win[j]: x @ M is the valid 1-D correlation."""
    key = (n, win.numel(), win.device, float(win[0]))
    m = _BANDS.get(key)
    if m is None:
        k = win.numel()
        out = n - k + 1
        m = torch.zeros(n, out, device=win.device, dtype=win.dtype)
        idx = torch.arange(out, device=win.device)
        for j in range(k):
            m[idx + j, idx] = win[j]
        _BANDS[key] = m
    return m


def ssim(x: torch.Tensor, y: torch.Tensor, data_range=1.0, win_size=11, sigma=1.5, K=(0.01, 0.03)) -> torch.Tensor:
    """pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3) on (1,C,H,W): separable
    gaussian window, valid convolution, mean over the map (gstex.py:351,1303).

    The separable valid filter runs as two banded GEMMs (hipBLASLt): MIOpen serves this depthwise
    11-tap convolution with its naive kernels, which cost more than the whole rasterizer."""
    H, W = x.shape[-2:]
    g = _gauss_window(win_size, sigma, x.device)
    bw = _band(W, g)
    bh = _band(H, g)

    def filt(t):  # (..., H, W) -> (..., H-k+1, W-k+1)
        return torch.matmul(bh.t(), torch.matmul(t, bw))

    C1 = (K[0] * data_range) ** 2
    C2 = (K[1] * data_range) ** 2
    maps = filt(torch.stack([x, y, x * x, y * y, x * y], 0))
    mu1, mu2 = maps[0], maps[1]
    s11 = maps[2] - mu1 * mu1
    s22 = maps[3] - mu2 * mu2
    s12 = maps[4] - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    sm = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    return sm.mean()


@dataclass
class StepOutput:
    loss: torch.Tensor
    rgb: torch.Tensor
    terms: torch.Tensor | None = None  # [main loss, L1, SSIM, MSE] of a step through image_loss (else None)


class GStexTrainer:
    """Holds the GStex parameters on one device and runs forward/backward/Adam steps."""

    def __init__(self, scene: Scene, device, sh_degree: int = 3, settings: int = DEFAULT_SETTINGS,
                 pixel_num: float | None = None, background=(1.0, 1.0, 1.0), fused_adam: bool = True,
                 fused_loss: bool = True, fused_activations: bool = True, geometry_outputs: bool = False,
                 sh_degree_interval: int = 1000, fix_init: bool = False, start_step: int = 0,
                 defer_texture: bool = False, lambda_normal=0.0, lambda_reg=0.0, use_normal_loss: bool = False,
                 pair_capacity: bool | None = None, fused_step: bool | None = None, background_seed: int = 0,
                 shared_grad: bool | None = None, lrs: dict | None = None):
        self.device = torch.device(device)
        d = self.device
        P = lambda t: torch.nn.Parameter(t.detach().to(d).contiguous())  # noqa: E731
        # the geometry parameters (what decides which (pixel, splat) pairs exist) share one allocation, each segment
        # 16-B aligned (the fused Adam's float4 path): `geometry_flat` snapshots / restores all four in one copy
        geo = [scene.means, scene.log_scales, scene.quats, scene.opacity_logits]
        sizes = [int(t.numel()) for t in geo]
        self.geometry_flat = torch.zeros(sum((n + 3) // 4 * 4 for n in sizes), device=d, dtype=torch.float32)
        views, off = [], 0
        for t, n in zip(geo, sizes):
            v = self.geometry_flat[off:off + n].view(t.shape)
            v.copy_(t.detach().to(d))
            views.append(torch.nn.Parameter(v))
            off += (n + 3) // 4 * 4
        self.means, self.scales, self.quats, self.opacities = views
        self.features_dc = P(scene.features_dc)
        self.features_rest = P(scene.features_rest)
        # the texel parameter stores the SH-DC value; the raster reads SH2RGB of it (gstex.py:1119).  Like the
        # reference's JaggedTexture (jagged_texture.py:36-64) it is a capacity store: rows [0, n_texels) are the
        # texels of the current charts, the store only grows at a rechart, and the raster takes the whole store
        # (texture_dims never index past n_texels), so its gradient needs no slice-backward copy
        tex_dc = RGB2SH(scene.texture[:, :3])
        self.texture_dc = P(tex_dc)
        self.n_texels = int(tex_dc.shape[0])
        self.texture_dims = scene.texture_dims.to(d).contiguous()
        self.mappings = scene.mappings.to(d).contiguous()
        self.sh_degree = sh_degree
        self.settings = settings
        # lrs: the per-group learning rates of a preset (gstex_amd.train.PRESETS); default LRS (gstex-blender-nvs)
        self.lrs = dict(LRS if lrs is None else lrs)
        if set(self.lrs) != set(LRS):
            raise ValueError(f"lrs must have exactly the groups {sorted(LRS)} (got {sorted(self.lrs)})")
        self.pixel_num = pixel_num if pixel_num is not None else float(scene.texture.shape[0])
        # background: a colour, "white", "black", or "random" (gstex.py:178, 1012-1020): a fresh uniform colour per
        # training step, drawn on the device into this same tensor (refresh_background), which feeds the render's
        # composite, the loss and an RGBA target's composite alike.  background_seed (not in the reference, which
        # draws from the global generator) seeds the trainer's own device generator.
        self.random_background = isinstance(background, str) and background == "random"
        if isinstance(background, str):
            if not self.random_background and background not in BACKGROUNDS:
                raise ValueError(f'background must be a colour, "white", "black" or "random" (got {background!r})')
            background = BACKGROUNDS.get(background, VIEWER_BACKGROUND)
        self.background = torch.tensor(background, dtype=torch.float32, device=d)
        self._eval_background = self.background.clone() if self.random_background else self.background
        self._background_gen = None
        if self.random_background:
            self._background_gen = torch.Generator(device=d)
            self._background_gen.manual_seed(int(background_seed))
        # the raster's own background is zero (the composite adds the real one, gstex.py:1204): one cached tensor
        self._bg_zero = torch.zeros_like(self.background)
        self._one = torch.ones((), dtype=torch.float32, device=d)
        self.step = start_step
        self.sh_degree_interval = sh_degree_interval  # gstex.py:182
        self.fix_init = fix_init  # gstex.py:209 (DTU configs): SH view directions (x, -z, y), gstex.py:1104-1108
        self.fused_adam = fused_adam
        self.fused_loss = fused_loss
        self.fused_activations = fused_activations
        # depth / distortion / normal renders: only for losses or views that read them (the reference's normal
        # and distortion weights default to 0, gstex.py:198-201, so its training loss uses none of them)
        self.geometry_outputs = geometry_outputs
        # the 2DGS regularisers of get_loss_dict (gstex.py:198-201, 207, 1218-1220, 1313-1317): weights as numbers or
        # [before, after, switch_step] schedules; a non-zero weight renders depth / distortion / normal for the step
        self.lambda_normal = lambda_normal
        self.lambda_reg = lambda_reg
        self.use_normal_loss = use_normal_loss
        self.test_colors = None  # eval-render test colours (gstex.py:309)
        # paint(): the (n_texels, 5) stroke accumulator (zero between calls: the blend kernel re-zeroes what the
        # scatter touched) and the per-splat scratch of its depth render
        self._paint_acc = None
        self._paint_scratch = {}
        # last_visibility: (num_tiles_hit, extents) of the last differentiable render, on either render path -- what
        # the density controller's per-step statistics read (gstex_amd.density).  Kept as the tensors themselves (per-op
        # render) or as (arena, two byte offsets, n) (fused render: the views are made when somebody asks)
        self._last_vis = None
        # defer_texture (not in the reference; fused Adam on a HIP device): the texel parameter's Adam update of step k
        # (73 % of the parameters at cfg3) runs in step k+1, before the raster forward, from a persistent gradient
        # buffer the raster grids zero (DESIGN.md "The texel gradient's life cycle"; the slots: _pending_slots).
        # Readers of texture_dc outside the step go through wait_texture() / texels(), which run a pending update.
        self.defer_texture = bool(defer_texture) and fused_adam and self.device.type == "cuda"
        self._pending_tex = None
        self._pending_collective = False  # the pending update first waits for a GradSync collective
        # pair_capacity (not in the reference; fused Adam on a HIP device): the training renders size their pair
        # buffers from an ops.PairCapacity instead of reading the pair total back to the host (gstex.py:1045-1052,
        # 1127), so a step has no host synchronisation.  Each step's renders write an overflow flag into
        # step_control[step % 8] (a device fp32 ring; gstex_amd.dist.GradSync replaces it by a slice of its flat
        # buffer, all-reduced with the gradients) that every Adam launch of the step reads (skip on overflow).
        # GSTEX_SYNC_PAIRS=1 restores the read-back.
        if pair_capacity is None:
            pair_capacity = os.environ.get("GSTEX_SYNC_PAIRS", "0") == "0"
        self.pairs = ops.PairCapacity(d) if (pair_capacity and fused_adam and self.device.type == "cuda") else None
        self.step_control = torch.zeros(8, device=d, dtype=torch.float32)
        self.skipped_steps = []  # steps whose update the pair-capacity guard skipped (found by _poll_pairs)
        # fused_step (not in the reference): the photometric training render as one C prologue call and one autograd
        # node (gstex_amd.fused) -- the same launches with ~0.23 ms less host time before the raster forward (the
        # device idles through that after a synchronisation); GSTEX_FUSED_STEP=0 restores the per-op render
        if fused_step is None:
            fused_step = os.environ.get("GSTEX_FUSED_STEP", "1") != "0"
        self.fused_step = bool(fused_step)
        # shared_grad (not in the reference): the fused loss hands the raster backward ONE upstream gradient for the
        # colour and the texture image (at 3 channels they are the same image), which selects the backward's training
        # build (gstex_raster_bwd_variant); GSTEX_SHARED_GRAD=0 keeps two tensors and the generic build
        if shared_grad is None:
            shared_grad = os.environ.get("GSTEX_SHARED_GRAD", "1") != "0"
        self.shared_grad = bool(shared_grad)
        self.texel_grad = TexelGrad()  # its buffers, zero flags and routing (as above)
        if self.defer_texture:
            self.texel_grad.own(self.texture_dc, self.fused_step)
        self._build_optimizer()

    @property
    def last_visibility(self):
        """(num_tiles_hit (n,) int32, extents (n, 2)) of the last differentiable render since zero_grad(), or None."""
        v = self._last_vis
        if v is None or len(v) == 2:
            return v
        arena, o_nth, o_ext, n = v
        return (arena[o_nth:o_nth + 4 * n].view(torch.int32),
                arena[o_ext:o_ext + 8 * n].view(torch.float32).view(n, 2))

    @property
    def texture_grad_sink(self):
        """The buffer the raster backward accumulates the texel gradient into (None: autograd owns it)."""
        return self.texel_grad.sink

    def _step_texels(self, buf, only, skip_flag):
        """The deferred texel update reading `buf` (the gradient buffer of the step it belongs to)."""
        keep = self.texture_dc.grad
        self.texture_dc.grad = buf
        try:
            self.optimizer.step(only=only, skip_flag=skip_flag)
        finally:
            self.texture_dc.grad = keep

    def reset_texture_grad(self):
        """Discard the texel-gradient sink's content lazily (zero_grad(); a skipped step's gradient): the
        next differentiable render is the step's first again, whose raster forward zeroes the sink."""
        self.texel_grad.reset()

    def _skip_flag(self):
        """The current step's guard flag (1-element view of step_control) for its Adam launches, or None."""
        if self.pairs is None:
            return None
        k = self.step % 8
        return self.step_control[k:k + 1]

    def _poll_pairs(self):
        """Pair totals of finished renders (non-blocking): grows the capacity, records skipped steps."""
        if self.pairs is not None and self.pairs.poll():
            import warnings

            new = self.pairs.overflows[len(self.skipped_steps):]
            self.skipped_steps.extend(new)
            warnings.warn(f"GStexTrainer: the pair total of step(s) {new} exceeded the pair capacity; their updates "
                          f"were skipped on the device and the capacity grew to {self.pairs.capacity}")

    def _run_pending_texture(self):
        fn, self._pending_tex = self._pending_tex, None
        if fn is not None:
            fn()

    def _pending_slots(self):
        """Where a render runs the pending texel update: -> (before_pair_wait, texture_ready) callbacks.  Without a
        pair-count read-back (pairs) it runs here, at the render's start: ~90 us of streaming work the device starts
        on while the host enqueues the preprocessing and binning, instead of idling after a synchronisation.  With
        one, while the host waits for the count.  An update that first waits for its collective (GradSync) runs
        right before the raster forward, the first reader of the texels, so the binning does not queue behind it."""
        if self._pending_tex is None:
            return None, None
        if self._pending_collective:
            return None, self._run_pending_texture
        if self.pairs is None:
            return self._run_pending_texture, None
        self._run_pending_texture()
        return None, None

    def wait_texture(self):
        """Order the current stream after the pending texel update (defer_texture): it is enqueued now."""
        self._run_pending_texture()

    def texels(self) -> torch.Tensor:
        """The texel store (SH-DC values) for readers outside the step (export, average_colors, viewers): runs a
        pending deferred update first (defer_texture), so no reader depends on remembering wait_texture()."""
        self.wait_texture()
        return self.texture_dc.detach()

    # ------------------------------------------------------------------ parameters
    def param_groups(self):
        return {
            "xyz": [self.means],
            "features_dc": [self.features_dc],
            "features_rest": [self.features_rest],
            "opacity": [self.opacities],
            "scaling": [self.scales],
            "rotation": [self.quats],
            "texture_dc": [self.texture_dc],
        }

    def parameters(self):
        return [p for ps in self.param_groups().values() for p in ps]

    def _build_optimizer(self):
        groups = [{"params": ps, "lr": self.lrs[name], "name": name} for name, ps in self.param_groups().items()]
        if self.fused_adam:
            self.optimizer = FusedAdam(groups, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(groups, eps=1e-15, foreach=True)

    # ------------------------------------------------------------------ forward
    def render(self, view: View, sh_degree_now: int | None = None, composite: bool = True, geometry: bool | None = None):
        """get_outputs (gstex.py:992-1236), training branch.  geometry: render depth / distortion / normal (default:
        the trainer's geometry_outputs).  sh_degree_now: default min(step // sh_degree_interval, sh_degree), as
        get_outputs evaluates it in training and eval alike (gstex.py:1103)."""
        means = self.means
        deg = self.sh_degree_now() if sh_degree_now is None else sh_degree_now
        before_pair_wait, texture_ready = self._pending_slots()
        if self._fused_ok(composite, geometry, view):
            return self._render_fused(view, deg, texture_ready)
        if self.fused_activations:  # one HIP launch each way (gstex_amd.activations)
            quats, scales, opacities, uv0, umap, vmap, viewdirs = activate(
                means, self.quats, self.scales, self.opacities, self.mappings, view.campos)
            if view.c2w.requires_grad and torch.is_grad_enabled():
                # camera pose refinement (gstex_amd.pose): the kernel's view directions carry no gradient; the torch
                # expression of the branch below does, to the camera position c2w[:3, 3]
                viewdirs = means.detach() - view.c2w[:3, 3]
                viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        else:
            quats = self.quats / self.quats.norm(dim=-1, keepdim=True)
            s = torch.exp(self.scales[:, :-1]).clamp(min=1e-9)
            scales = torch.cat([s, 1e-5 * s.mean(dim=-1, keepdim=True).detach()], dim=-1)
            opacities = torch.sigmoid(self.opacities)
            uv0, umap, vmap = get_uv_mapping(quats, self.mappings)
            viewdirs = means.detach() - view.c2w[:3, 3]
            viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        viewdirs = self._sh_viewdirs(viewdirs)
        intr = (view.fx, view.fy, view.cx, view.cy)
        # project_points / get_aabb_2d / get_num_tiles_hit_2d (gstex.py:1077-1080) in one launch; the centre
        # gradient is chained inside the raster backward (fold_aabb below), the depths only order the tile lists
        depths, centers, extents, nth = ops.preprocess(means, scales, 1, quats, view.viewmat, intr, view.H, view.W)
        n = self.means.shape[0]
        if self.sh_degree > 0:
            if self.fused_activations:  # the zeroed DC term (gstex.py:1100) without the cat
                rgbs = sh_rest(deg, viewdirs, self.features_rest)
            else:
                colors = torch.cat([torch.zeros_like(self.features_dc[:, None, :]), self.features_rest], dim=1)
                rgbs = ops.spherical_harmonics(deg, viewdirs, colors)
        else:
            rgbs = torch.sigmoid(self.features_dc)
        # SH2RGB(texture_dc) (gstex.py:1119) applied by the raster on read instead of materialised
        texture = self.texture_dc
        sink, zero_sink, first, on_grad, _ = self.texel_grad.target(fused=False)
        guard = None
        if self.pairs is not None and torch.is_grad_enabled():
            self._poll_pairs()
            guard = (self.pairs, self._skip_flag(), first, self.step)
        img, depth, reg, alpha, tex, normal = ops.texture_gaussians(
            (n, 1, 3), self.texture_dims, centers, extents, depths, nth, rgbs, opacities, means, scales, 1, quats,
            uv0, umap, vmap, texture, view.viewmat, view.c2w, view.fx, view.fy, view.cx, view.cy, view.H, view.W,
            ops.BLOCK_WIDTH, self.settings, background=self._bg_zero,
            texture_transform=(SH_C0, 0.5), fold_aabb=True,  # centers come from get_aabb_2d just above
            geometry_outputs=self.geometry_outputs if geometry is None else geometry,
            texture_grad_sink=sink, zero_texture_grad_sink=zero_sink, on_texture_grad=on_grad,
            texture_ready=texture_ready, before_pair_wait=before_pair_wait, pair_guard=guard)
        if torch.is_grad_enabled():
            self.texel_grad.rendered()
            self._last_vis = (nth, extents)
        out = dict(img=img, tex=tex, depth=depth, reg=reg, alpha=alpha, normal=normal)
        if composite:
            out["rgb"] = _composite(img, tex, alpha, self.background)
        return out

    def _sh_viewdirs(self, viewdirs):
        """fix_init (gstex.py:209, the DTU configs): the SH basis is evaluated at (x, -z, y) (gstex.py:1104-1108)."""
        swap = self.fix_init and self.sh_degree > 0
        return torch.stack([viewdirs[:, 0], -viewdirs[:, 2], viewdirs[:, 1]], -1) if swap else viewdirs

    def _fused_ok(self, composite: bool, geometry, view: View | None = None) -> bool:
        """Whether render() takes gstex_amd.fused's path (see its docstring for why each condition is there).  A view
        whose viewmat / c2w require a gradient (camera pose refinement) declines it: that path has no pose chain."""
        if view is not None and (view.viewmat.requires_grad or view.c2w.requires_grad):
            return False
        return (self.fused_step and not composite and not (self.geometry_outputs if geometry is None else geometry)
                and self.fused_activations and self.sh_degree > 0 and not self.fix_init
                and self.pairs is not None and self.pairs.capacity > 0 and self.texture_grad_sink is not None
                and torch.is_grad_enabled() and not torch.are_deterministic_algorithms_enabled()
                and not torch.cuda.is_current_stream_capturing())

    def _render_fused(self, view: View, deg: int, texture_ready=None):
        from . import fused

        self._poll_pairs()
        img, alpha, tex = fused.train_render(self, view, deg, self.texel_grad.target(fused=True), texture_ready)
        self.texel_grad.rendered()
        depth, reg, normal = ops._zero_views(self.device, int(view.H), int(view.W))  # not rendered, as the per-op path
        return dict(img=img, tex=tex, depth=depth, reg=reg, alpha=alpha, normal=normal)

    @torch.no_grad()
    def eval_render(self, view: View, edit_texture: torch.Tensor | None = None):
        """The reference's eval render (get_outputs with extra_stuff, gstex.py:1086-1203): a 6-channel texture
        [SH2RGB(texture_dc), 0, 0, 0] and three raster calls -- the image, the test-colour render with
        thresholded opacities (test_img / uv_im) and the settings | 1 << 15 render (edit_img, clean normals).
        Same outputs (tests/test_gpu_eval.py checks them against those three 6-channel calls), computed with one
        binning and the 3-channel raster (below)."""
        self.wait_texture()
        means = self.means
        quats, scales, opacities, uv0, umap, vmap, viewdirs = activate(
            means, self.quats, self.scales, self.opacities, self.mappings, view.campos)
        viewdirs = self._sh_viewdirs(viewdirs)
        intr = (view.fx, view.fy, view.cx, view.cy)
        _, depths = ops.project_points(means, view.viewmat, intr)
        centers, extents = ops.get_aabb_2d(means, scales, 1, quats, view.viewmat, intr)
        nth = ops.get_num_tiles_hit_2d(centers, extents, view.H, view.W, ops.BLOCK_WIDTH)
        n = means.shape[0]
        rgbs = (sh_rest(self.sh_degree_now(), viewdirs, self.features_rest) if self.sh_degree > 0
                else torch.sigmoid(self.features_dc))
        if self.test_colors is None or self.test_colors.shape[0] != n:
            g = torch.Generator(device="cpu").manual_seed(0)
            self.test_colors = torch.rand((n, 3), generator=g).to(means.device)  # gstex.py:309
        bgz = self._bg_zero
        # the three calls share one geometry: binned and sorted once.  The reference's 6-channel texture is
        # [SH2RGB(texture_dc), 0, 0, 0] for the first call and [edit_texture or 0, 0, 0, 0] for the other two; a
        # zero texel contributes exactly 0, so each call runs the 3-channel raster (SH2RGB as texture_transform,
        # the all-zero texture as transform (0, 0)) and channels 3..5 of its texture output are zeros -- the same
        # outputs without materialising two 6-channel copies of the texel store
        bins = ops.bin_gaussians(centers, extents, depths, nth, view.H, view.W)

        def tg(cr, tex, transform, co, st):
            return ops.texture_gaussians(
                (n, 1, 3), self.texture_dims, centers, extents, depths, nth, cr, co, means, scales, 1, quats, uv0,
                umap, vmap, tex, view.viewmat, view.c2w, view.fx, view.fy, view.cx, view.cy, view.H, view.W,
                ops.BLOCK_WIDTH, st, background=bgz, texture_transform=transform, binning=bins)

        img, depth, reg, alpha, tex, normal = tg(rgbs, self.texture_dc, (SH_C0, 0.5), opacities, self.settings)
        upd, upd_tf = (edit_texture, None) if edit_texture is not None else (self.texture_dc, (0.0, 0.0))
        test_op = opacities.clone()
        test_op[test_op <= 0.5] = 0.0
        test_op[test_op > 0.2] = 1.0
        t_out = tg(self.test_colors, upd, upd_tf, test_op, self.settings)
        if edit_texture is not None:
            n_edit, n_unit = tg(self.test_colors, upd, upd_tf, opacities, self.settings | (1 << 15))[4:6]
        else:
            # the settings | 1 << 15 call has the first call's geometry and weights: its texture output is the zero
            # texture's (0) and its normal is the first call's accumulated normal as a unit vector (0 where none),
            # the same fp32 operations as the kernel's bit-15 epilogue -- no third raster pass
            n2 = (normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2]
            inv = torch.where(n2 > 0, 1.0 / torch.sqrt(n2), torch.zeros_like(n2))
            n_edit, n_unit = None, normal * inv[..., None]
        zeros3 = torch.zeros_like(img)  # texture channels 3..5 of every call
        bg = self._eval_background[None, None, :]  # (the trainer's background; the viewer colour under "random")
        edit_tex_img = n_edit[..., :3] if n_edit is not None else zeros3
        return dict(rgb=_composite(img, tex, alpha, self._eval_background), depth=depth, alpha=alpha, normal=normal,
                    test_img=t_out[0] + (1 - t_out[3][..., None]) * bg,
                    uv_im=torch.clamp(zeros3 + (1 - t_out[3][..., None]) * bg, 0.0, 1.0),
                    edit_img=_composite(img, edit_tex_img, alpha, self._eval_background),
                    clean_normal_img=torch.clamp(0.5 * (n_unit + 1) + (1 - alpha[..., None]) * bg, 0.0, 1.0))

    @torch.no_grad()
    def evaluate(self, view: View, image: torch.Tensor, out: torch.Tensor | None = None) -> ImageMetrics:
        """One view scored by the reference's protocol (get_image_metrics_and_images, gstex.py:1337-1403): one plain
        render (the per-op path, no geometry outputs: none of eval_render's viewer images) at the current SH degree on
        the evaluation background (the viewer colour under background="random", gstex.py:1021-1025), then PSNR and
        SSIM of the uint8-quantised render against `image` as the dataset delivers it (gstex_amd.loss.image_metrics;
        image_metrics_eager on the composited render with fused_loss=False).  out: a 4-element device fp32 tensor the
        metrics are written into.  The training state is left alone: a pending deferred texel update is run (it
        would run before the next render anyway), nothing else is touched."""
        self.wait_texture()
        r = self.render(view, composite=False, geometry=False)
        bg = self._eval_background
        if self.fused_loss:
            return image_metrics(r["img"], r["tex"], r["alpha"], bg, image, out=out)
        res = image_metrics_eager(_composite(r["img"], r["tex"], r["alpha"], bg), bg, image)
        if out is not None:
            out.copy_(res.metrics)
            res.metrics = out
        return res

    def evaluate_split(self, pairs, output_dir=None) -> dict:
        """A test split scored as get_average_eval_image_metrics does (pipelines/base_pipeline.py:347-410): every
        (View, image) of `pairs` (as gstex_amd.data.load_blender yields them) through evaluate(), image i's metrics
        in row i of one (n, 4) device table that is read back once, after the loop.  Returns psnr, ssim, mse and
        mse_raw, each the float64 mean of the per-image values (the mean of the PSNRs, not the PSNR of the mean MSE),
        gaussian_count, texel_count and per_image (the table on the CPU, columns [PSNR, SSIM, MSE, MSE_raw]).
        There is no lpips key: the LPIPS network's weights are not part of this project, and a made-up 0 would be
        worse than an absent key.  output_dir: also write "{i:06d}-img.png", the reference's `img` (the target's
        (gt * 255).byte() and the render's bytes side by side, base_pipeline.py:383-387)."""
        pairs = list(pairs)
        if not pairs:
            raise ValueError("evaluate_split: no (view, image) pairs")
        table = torch.zeros((len(pairs), 4), device=self.device, dtype=torch.float32)
        for i, (view, image) in enumerate(pairs):
            res = self.evaluate(view.to(self.device), image.to(self.device), out=table[i])
            if output_dir is not None:
                from PIL import Image  # (lazily, as gstex_amd.data)

                both = torch.cat([(res.gt * 255).byte(), res.rgb_u8], dim=1)
                Image.fromarray(both.cpu().numpy()).save(os.path.join(str(output_dir), f"{i:06d}-img.png"))
        per_image = table.cpu()
        mean = per_image.double().mean(dim=0)
        return dict(psnr=float(mean[0]), ssim=float(mean[1]), mse=float(mean[2]), mse_raw=float(mean[3]),
                    gaussian_count=float(self.means.shape[0]), texel_count=float(self.n_texels),
                    per_image=per_image)

    # ------------------------------------------------------------------ mesh extraction
    @torch.no_grad()
    def extract_mesh(self, views, voxel_size: float | None = None, mesh_res: int = 256,
                     sdf_trunc: float | None = None, bounds=None, alpha_min: float = 0.5, depth_trunc: float = 0.0,
                     color: bool = True, keep_largest: int | None = None):
        """The lineage's mesh of a trained model (gstex_amd.mesh, DESIGN.md "Mesh extraction"): every view rendered (the
        per-op path with the geometry outputs, composited on the evaluation background), the depth maps fused into a
        TSDF volume 8 views per launch, and the zero surface extracted by marching tetrahedra, all on the device.
        -> (vertices (V, 3) f32, colors (V, 3) f32 or None, faces (F, 3) int32).

        bounds: (lo, hi) of the surface's box; default the AABB of the means.  The grid is that box padded on every
        side by sdf_trunc + voxel_size.  voxel_size: default the longest PADDED side over mesh_res; the pad depends on
        it, so the two are solved together: with L the box's longest side and the default sdf_trunc = 5 voxel_size
        (the lineage's ratio), voxel_size = L / (mesh_res - 12); with sdf_trunc given, voxel_size =
        (L + 2 sdf_trunc) / (mesh_res - 2) (gstex_amd.mesh.mesh_grid).  near_z is the raster's near plane, 0.2.
        keep_largest: keep that many connected components with the most faces (the lineage's floater removal; a host
        pass).  The training state is left alone: a pending deferred texel update is run (it would run before the next
        render anyway), nothing else is touched."""
        from .mesh import TSDFVolume, largest_components, mesh_grid

        views = [v.to(self.device) for v in views]
        if not views:
            raise ValueError("extract_mesh: no views")
        self.wait_texture()
        if bounds is None:
            m = self.means.detach()
            lo, hi = m.min(dim=0).values.cpu().numpy(), m.max(dim=0).values.cpu().numpy()
        else:
            lo, hi = bounds
        origin, h, dims, trunc, _ = mesh_grid(lo, hi, voxel_size, mesh_res, sdf_trunc)
        vol = TSDFVolume(self.device, origin, h, dims, trunc, color=color)
        for i in range(0, len(views), 8):  # a launch's renders are alive together, no more
            batch = views[i:i + 8]
            vol.integrate(batch, [self._mesh_render(v, color) for v in batch], alpha_min=alpha_min,
                          depth_trunc=depth_trunc, near_z=0.2)
        vertices, colors, faces = vol.extract()
        if keep_largest is not None:
            f, kept = largest_components(faces.cpu().numpy(), vertices.shape[0], int(keep_largest))
            kept = torch.from_numpy(kept).to(self.device)
            vertices = vertices[kept]
            colors = None if colors is None else colors[kept]
            faces = torch.from_numpy(f).to(self.device)
        return vertices, colors, faces

    @torch.no_grad()
    def score_mesh(self, views, reference, *, spacing: float, max_dist: float | None = None, thresholds=(),
                   score_bounds=None, **extract_kw) -> dict:
        """extract_mesh(views, **extract_kw) scored against a reference point cloud (R, 3) by gstex_amd.mesh.score_mesh
        (accuracy, completeness, chamfer and per threshold precision, recall, fscore), all on the device.  spacing: the
        surface sampler's; score_bounds: score_mesh's `bounds`, the observation box (extract_mesh's own `bounds` goes in
        extract_kw).  The dict also holds the mesh as vertices, colors and faces.  Like extract_mesh it leaves the
        training state alone."""
        from .mesh import score_mesh

        extract_kw.setdefault("color", False)
        vertices, colors, faces = self.extract_mesh(views, **extract_kw)
        ref = torch.as_tensor(reference, dtype=torch.float32).to(self.device)
        out = score_mesh(vertices, faces, ref, spacing=spacing, max_dist=max_dist, thresholds=thresholds,
                         bounds=score_bounds)
        out.update(vertices=vertices, colors=colors, faces=faces)
        return out

    # ------------------------------------------------------------------ clustering
    @torch.no_grad()
    def activated_splats(self):
        """The step's activation of the geometry (gstex.py:1059-1066) in torch: -> (means, in-plane scales (n, 2) =
        clamp(exp(log-scales), 1e-9), unit quats), detached."""
        quats = self.quats.detach() / self.quats.detach().norm(dim=-1, keepdim=True)
        scales = torch.exp(self.scales.detach()[:, :2]).clamp(min=1e-9)
        return self.means.detach(), scales, quats

    @torch.no_grad()
    def cluster(self, eps: float, min_pts: int, cell_size: float | None = None):
        """DBSCAN of the trainer's splats under the squared 2-Wasserstein distance (gstex_amd.cluster.dbscan on
        activated_splats(), DESIGN.md "Clustering the splats"): -> ClusterResult(labels, degree, core, n_clusters) on
        the device.  eps bounds the SQUARED distance.  Like extract_mesh it leaves the training state alone (a
        pending deferred texel update is run first)."""
        from .cluster import dbscan

        self.wait_texture()
        return dbscan(*self.activated_splats(), eps, min_pts, cell_size=cell_size)

    def _mesh_render(self, view: View, color: bool) -> dict:
        """One view's inputs of TSDFVolume.integrate: the un-normalised depth, alpha and the composited colour."""
        r = self.render(view, composite=False, geometry=True)
        out = dict(depth=r["depth"].contiguous(), alpha=r["alpha"].contiguous())
        if color:
            out["rgb"] = _composite(r["img"], r["tex"], r["alpha"], self._eval_background).contiguous()
        return out

    # ------------------------------------------------------------------ appearance editing
    @torch.no_grad()
    def paint(self, view: View, stroke: torch.Tensor, texture: torch.Tensor | None = None, depth_eps: float = 1e-2,
              depth: torch.Tensor | None = None) -> torch.Tensor:
        """draw_from_view (gstex.py:489-606): back-project a screen-space RGBA stroke -- (H, W, 4), float32 in [0, 1]
        or uint8 (read as v / 255), straight alpha -- onto the texels of the surface the view sees.

        One preprocess, one binning and one raster setup; one depth render (the trainer's settings, glob_scale 1);
        then every pair whose hit depth lies within depth_eps of the rendered depth adds the stroke to its four
        texels (ops.paint_scatter, settings 1 << 13 alone as gstex.py:599), and the sums are blended into the texels
        (ops.paint_blend, gstex.py:603-605).  texture: a raster-space (n_texels, 3) float32 tensor on the trainer's
        device, edited in place and returned; None: a fresh SH2RGB(texture_dc[:n_texels]).  depth: an (H, W) map used
        instead of the depth render.  With no texels (2DGS mode) or a view that hits no tile the texture is returned
        as it is.  No training state is touched (a pending deferred texel update is run first, as any reader of the
        texels does): the result shows in eval_render(view, edit_texture=...), bake_edits() makes it permanent."""
        return self._paint(view, stroke, texture, (1.0, 0.0), depth_eps, depth)

    def _paint(self, view, stroke, texture, transform, depth_eps, depth):
        self.wait_texture()
        T, d = self.n_texels, self.means.device
        if texture is None:
            texture = SH2RGB(self.texture_dc.detach()[:T])
        ops._check(isinstance(texture, torch.Tensor) and texture.dtype == torch.float32 and texture.device == d
                   and texture.dim() == 2 and texture.shape[1] == 3 and texture.shape[0] >= T
                   and texture.is_contiguous(),
                   f"texture must be a contiguous float32 (>= {T}, 3) tensor on {d}")
        H, W = int(view.H), int(view.W)
        ops._check(isinstance(stroke, torch.Tensor) and stroke.dtype in (torch.float32, torch.uint8)
                   and tuple(stroke.shape) == (H, W, 4) and stroke.device == d,
                   f"stroke must be a float32 or uint8 ({H}, {W}, 4) tensor on {d}")
        if depth is not None:
            ops._check(depth.dtype == torch.float32 and tuple(depth.shape) == (H, W) and depth.device == d,
                       f"depth must be a float32 ({H}, {W}) tensor on {d}")
        if T == 0:
            return texture
        quats, scales, opacities, uv0, umap, vmap, _ = activate(
            self.means, self.quats, self.scales, self.opacities, self.mappings, view.campos)
        intr = (view.fx, view.fy, view.cx, view.cy)
        depths, centers, extents, nth = ops.preprocess(self.means, scales, 1, quats, view.viewmat, intr, H, W)
        bins = ops.bin_gaussians(centers, extents, depths, nth, H, W)
        if bins.sorted_ids.shape[0] == 0:  # no splat reaches a tile
            return texture
        cam = (view.viewmat, view.c2w, view.fx, view.fy, view.cx, view.cy, H, W)
        records, rendered = ops.depth_render(self.texture_dims, centers, nth, opacities, self.means.detach(), scales, 1,
                                             quats, uv0, umap, vmap, *cam, self.settings, bins,
                                             scratch=self._paint_scratch, render=depth is None)
        acc = self._paint_acc
        if acc is None or acc.shape[0] != T:  # (re-made when a rechart changes n_texels; zero from here on: the
            acc = self._paint_acc = torch.zeros((T, 5), device=d, dtype=torch.float32)  # blend re-zeroes its rows)
        ops.paint_scatter(acc, stroke, rendered if depth is None else depth, records, bins.tile_ranges, bins.order,
                          bins.sorted_ids, *cam, T, settings=1 << 13, eps=depth_eps)
        ops.paint_blend(acc, texture, T, transform)
        return texture

    @staticmethod
    def _edit_pair(e):
        return (e.view, e.canvas) if hasattr(e, "canvas") else (e[0], e[1])

    @torch.no_grad()
    def edit_texture(self, edits) -> torch.Tensor:
        """update_edit_texture (gstex.py:427-437): a fresh SH2RGB(texture_dc[:n_texels]) with every edit of the list
        -- gstex_amd.edit.Edit entries or (view, canvas) pairs -- painted on it in order; the tensor to hand to
        eval_render(view, edit_texture=...).  Undo (handle_undo) is the replay of edits[:-1]."""
        self.wait_texture()
        texture = SH2RGB(self.texture_dc.detach()[:self.n_texels])
        for e in edits:
            view, canvas = self._edit_pair(e)
            self.paint(view.to(self.device), canvas.to(self.device), texture)
        return texture

    @torch.no_grad()
    def bake_edits(self, edits) -> None:
        """The same replay written into the model: each edit is blended directly into texture_dc[:n_texels], the
        SH-DC store (the blend reads SH2RGB of a texel and writes RGB2SH of the result, ops.paint_blend's transform),
        so texels no stroke reaches keep their bits -- which a SH2RGB -> RGB2SH round trip of the whole store would
        not.  The Adam moments of texture_dc are left alone (a painted texel's next update still carries its old
        momentum), as are every other parameter, the gradients and the step counter."""
        self.wait_texture()
        store = self.texture_dc.detach()
        for e in edits:
            view, canvas = self._edit_pair(e)
            self._paint(view.to(self.device), canvas.to(self.device), store, (SH_C0, 0.5), 1e-2, None)

    def loss(self, rgb: torch.Tensor, gt: torch.Tensor, ssim_lambda: float = 0.2) -> torch.Tensor:
        l1 = torch.abs(gt - rgb).mean()
        sim = 1 - ssim(gt.permute(2, 0, 1)[None], rgb.permute(2, 0, 1)[None])
        return (1 - ssim_lambda) * l1 + ssim_lambda * sim

    def sh_degree_now(self) -> int:
        """The SH degree ramp of the reference: min(step // sh_degree_interval, sh_degree) (gstex.py:1103)."""
        return min(self.step // self.sh_degree_interval, self.sh_degree)

    def refresh_background(self) -> torch.Tensor:
        """The step's background: under background="random" a fresh uniform colour written into self.background on the
        device (no host read-back); forward_backward calls it once per step, before the render."""
        if self.random_background:
            self.background.uniform_(0.0, 1.0, generator=self._background_gen)
        return self.background

    def forward_backward(self, view: View, gt: torch.Tensor, mask: torch.Tensor | None = None,
                         extra_loss: torch.Tensor | None = None) -> StepOutput:
        """One training step's loss and gradients.  gt: the target as the dataset delivers it -- float32 or uint8,
        (H, W, 3), or (H, W, 4) with straight alpha (composited on the step's background); mask: bool or float32,
        (H, W) or (H, W, 1), applied to both images before L1 and SSIM (gstex.py:1294-1299).

        view: its viewmat / c2w may require a gradient (gstex_amd.pose.PoseRefiner.view): the per-op path then also
        produces the pose gradient (the fused step declines such a view).  extra_loss: a scalar added to the loss
        before the backward (the pose regulariser)."""
        lam_n, lam_r = scheduled(self.lambda_normal, self.step), scheduled(self.lambda_reg, self.step)
        geo = lam_n != 0.0 or lam_r != 0.0
        self.refresh_background()
        out = self.render(view, sh_degree_now=self.sh_degree_now(), composite=not self.fused_loss,
                          geometry=True if geo else None)
        terms = None
        if mask is not None or gt.dtype != torch.float32 or gt.shape[-1] != 3:
            # a dataset target: conversion, alpha composite and mask inside the loss kernels (gstex_amd.loss)
            if self.fused_loss:
                res = image_loss(out["img"], out["tex"], out["alpha"], self.background, gt, mask,
                                 share_grad=self.shared_grad)
            else:
                res = image_loss_eager(out["rgb"], self.background, gt, mask)
            loss, rgb, terms = res.loss, res.rgb, res.terms
        elif self.fused_loss:  # composite + clamp + L1/SSIM in one HIP launch pair (gstex_amd.loss)
            loss, rgb = photometric_loss(out["img"], out["tex"], out["alpha"], self.background, gt.contiguous(),
                                         share_grad=self.shared_grad)
        else:
            rgb = out["rgb"]
            loss = self.loss(rgb, gt)
        if geo:
            # gstex.py:1218-1222: the depth-derived normal (detached) when use_normal_loss, else the rendered normal
            est = (depth_to_normal(out["depth"], view.viewmat, view.c2w, view.fx, view.fy, view.cx, view.cy).detach()
                   if self.use_normal_loss else out["normal"])
            loss = loss + geometry_loss(out["alpha"], out["normal"], est, out["reg"], lam_n, lam_r)
        if extra_loss is not None:
            loss = loss + extra_loss
        loss.backward(self._one)  # (a cached seed: no per-step fill launch for the implicit ones_like)
        return StepOutput(loss.detach(), rgb.detach(), terms)

    def optimizer_step(self, sync=None):
        """The Adam step.  With a gstex_amd.dist.GradSync `sync` (data-parallel training) the gradient exchange is part
        of the step: the texel group is updated as soon as its collective lands, overlapping the head's collective,
        and the 1 / world averaging rides in the fused update (GradSync.all_reduce_and_step); otherwise call
        sync.all_reduce() before this."""
        sf = self._skip_flag()  # this step's pair-capacity guard (None without pair_capacity)
        opt, tex, defer = self.optimizer, {id(self.texture_dc)}, self.defer_texture
        self._run_pending_texture()  # (two steps without a render in between)
        buf = self.texel_grad.stepped()  # the gradient this step's texel update reads (the next step's may differ)
        if not self.fused_adam:  # (torch's Adam: no skip_flag, which needs the fused one)
            if sync is not None:
                sync.all_reduce()
            opt.step()
        elif sync is not None:
            # the texel update in pieces, each as soon as its piece of the collective has landed (GradSync)
            rng = (lambda s, lo, hi, first: opt.step_range(self.texture_dc, lo, hi, first, grad_scale=s,
                                                           skip_flag=sf)) if defer else None
            self._pending_tex = sync.all_reduce_and_step(
                lambda s: opt.step(only=tex, grad_scale=s, skip_flag=sf),
                lambda s: opt.step(skip=tex, grad_scale=s, skip_flag=sf), defer_tail=defer, step_tail_range=rng)
            self._pending_collective = defer
        elif defer:
            opt.step(skip=tex, skip_flag=sf)
            self._pending_tex = lambda: self._step_texels(buf, tex, sf)
            self._pending_collective = False
        else:
            opt.step(skip_flag=sf)
        self.step += 1

    def zero_grad(self, set_to_none: bool = True):
        """Optimizers.zero_grad_all (engine/optimizers.py): torch's default set_to_none=True, so backward
        writes fresh gradients instead of accumulating into zero-filled ones.  Keep set_to_none=False
        when .grad tensors are views of a flat buffer (gstex_amd.dist.GradSync zeroes that instead).  With
        defer_texture the texel gradient buffer is kept (the raster forward zeroes it), and the previous step's deferred
        texel update is enqueued here, first: it reads that buffer (which set_to_none=False would otherwise zero under
        it), and a step that starts on an idle device -- after a synchronisation -- gets its first long kernel without
        waiting for the host to reach the render (the launch order on the stream is the same as from render())."""
        if self._pending_tex is not None and not self._pending_collective:
            self._run_pending_texture()
        self.reset_texture_grad()
        self._last_vis = None  # (it holds the last fused render's arena: released before the next one is made)
        if self.defer_texture:
            keep = self.texture_dc.grad
            self.optimizer.zero_grad(set_to_none=set_to_none)
            self.texture_dc.grad = keep
            return
        self.optimizer.zero_grad(set_to_none=set_to_none)

    # ------------------------------------------------------------------ rechart
    @torch.no_grad()
    def recharge(self):
        """retexture_after (gstex.py:890-895): rebuild the charts from the current scales, resample the texels
        onto the new grid (texture_sample, JaggedTexture.init_from_dims, jagged_texture.py:116-143) and reset the
        texture Adam moments (reshape_in_optim, gstex.py:799-826: exp_avg / exp_avg_sq zeroed, step kept).

        The texel store is reused in place while the new charts fit its capacity (jagged_texture.py:45-64:
        adjust_texture_size only ever grows it), so the Parameter, its optimizer entry and any flat gradient
        buffer built over it (gstex_amd.dist.GradSync) stay valid; only a growth replaces the Parameter."""
        self.wait_texture()
        new_dims, mappings, _ = build_charts(self.scales.detach(), self.pixel_num)
        n_new = int((new_dims[:, 0].long() * new_dims[:, 1].long()).sum())
        ids, uv = texture_dims_to_query(new_dims)
        query = self.texture_dims[ids].contiguous()
        new_tex = ops.texture_sample((1, 1, 3), query, self.texture_dc.detach(), uv.contiguous())
        old = self.texture_dc
        cap = old.shape[0]
        if n_new > cap:  # adjust_texture_size: grow with zero rows (jagged_texture.py:53-64)
            store = torch.cat([old.detach(), old.new_zeros((n_new - cap, old.shape[1]))], 0)
            self.texture_dc = torch.nn.Parameter(store)
            for g in self.optimizer.param_groups:
                if g["name"] == "texture_dc":
                    g["params"] = [self.texture_dc]
            st = self.optimizer.state.pop(old, None)
            if st:
                self.optimizer.state[self.texture_dc] = {
                    "step": st.get("step", 0),
                    "exp_avg": torch.zeros_like(self.texture_dc),
                    "exp_avg_sq": torch.zeros_like(self.texture_dc),
                }
            if self.defer_texture:  # a fresh persistent gradient buffer (GradSync replaces it)
                self.texel_grad.own(self.texture_dc, self.fused_step)
        else:
            st = self.optimizer.state.get(old)
            if st:
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        self.texture_dc.data[:n_new] = new_tex
        self.texture_dims = new_dims.contiguous()
        self.n_texels = n_new
        self.mappings.copy_(mappings)
        return new_dims

    # ------------------------------------------------------------------ density control
    @torch.no_grad()
    def apply_density(self, grad_sum, count, max_extent, noise, thresholds: dict, size_prune: bool,
                      max_splats: int | None = None):
        """One density-control event (gstex_amd.density; DESIGN.md "Density control"): plan from the statistics
        (three (n,) fp32 arrays) and `thresholds` (density_thresholds), scan, one read-back, then every per-splat
        parameter and the Adam moments the optimizer holds scattered into fresh tensors of n_new rows in source order
        (kept rows keep their moments, clone rows and split children start at zero; each parameter's step count is
        kept, as in recharge()).  noise: (n, 2, 2), the split children's offsets in units of the activated scales.
        Defined on one-texel charts only (ValueError otherwise); a trainer under GradSync raises.  Rebuilt for n_new:
        geometry_flat and its four views, features_dc / features_rest / texture_dc, texture_dims, n_texels, mappings,
        the optimizer's groups and state, the texel gradient's buffers; the paint accumulator and scratch are dropped.
        An event that would leave no splat raises RuntimeError and an all-keep event returns, both with the trainer
        untouched.  On a CPU trainer the eager twins run instead of the kernels.  -> the DensityPlan."""
        from . import density as dn

        n, d = self.means.shape[0], self.device
        if self.texel_grad.routed:
            raise RuntimeError("apply_density: multi-GPU density control (a trainer under GradSync) is not supported")
        one_texel = ("density control is defined on one-texel charts only (n_texels == n, texture_dims rows "
                     "(1, 1, i)): run it before the first rechart onto a texel budget")
        if self.n_texels != n or tuple(self.texture_dims.shape) != (n, 3) or self.texture_dc.shape[0] < n:
            raise ValueError(f"apply_density: {one_texel} (n = {n}, n_texels = {self.n_texels})")
        for name, t in (("grad_sum", grad_sum), ("count", count), ("max_extent", max_extent)):
            if tuple(t.shape) != (n,) or t.dtype != torch.float32 or t.device != self.means.device:
                raise ValueError(f"apply_density: {name} must be a float32 ({n},) tensor on {self.means.device}")
        if tuple(noise.shape) != (n, 2, 2) or noise.dtype != torch.float32 or noise.device != self.means.device:
            raise ValueError(f"apply_density: noise must be a float32 ({n}, 2, 2) tensor on {self.means.device}")

        def one_texel_dims(rows):
            dims = torch.ones((rows, 3), device=d, dtype=torch.int32)
            dims[:, 2] = torch.arange(rows, device=d, dtype=torch.int32)
            return dims

        bad = (self.texture_dims != one_texel_dims(n)).any()  # (read back with the plan's counts)
        plan = dn.plan_event(self.scales, self.opacities, grad_sum, count, max_extent, thresholds, size_prune,
                             max_splats, check=bad)
        if plan.flagged:
            raise ValueError(f"apply_density: {one_texel}")
        if plan.n_new == 0:
            raise RuntimeError("apply_density: the event would prune every splat")
        if plan.kept == n:
            return plan
        self.wait_texture()
        if d.type == "cuda":
            quats_n, scales = activate(self.means.detach(), self.quats.detach(), self.scales.detach(),
                                       self.opacities.detach(), self.mappings, torch.zeros(3, device=d))[:2]
        else:
            quats_n = self.quats / self.quats.norm(dim=-1, keepdim=True)
            s = torch.exp(self.scales[:, :-1]).clamp(min=1e-9)
            scales = torch.cat([s, 1e-5 * s.mean(dim=-1, keepdim=True)], dim=-1)
        opt, before = self.optimizer, self.param_groups()
        attrs = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest",
                 "opacity": "opacities", "scaling": "scales", "rotation": "quats", "texture_dc": "texture_dc"}
        roles = {"xyz": dn.ROLE_MEANS, "scaling": dn.ROLE_LOG_SCALES}
        named = {}
        for group, (p,) in before.items():
            named[group] = (p.detach()[:n], roles.get(group, dn.ROLE_COPY))  # ([:n]: the texel store has a capacity)
            st = opt.state.get(p)
            if st and "exp_avg" in st:
                named[group + ".exp_avg"] = (st["exp_avg"][:n], dn.ROLE_MOMENT)
                named[group + ".exp_avg_sq"] = (st["exp_avg_sq"][:n], dn.ROLE_MOMENT)
        # the geometry parameters' shared allocation, segments 16-B aligned (as __init__)
        m = plan.n_new
        geo = [("xyz", 3), ("scaling", 3), ("rotation", 4), ("opacity", 1)]
        flat = torch.zeros(sum((m * w + 3) // 4 * 4 for _, w in geo), device=d, dtype=torch.float32)
        views, off = {}, 0
        for group, w in geo:
            views[group] = flat[off:off + m * w].view(m, w)
            off += (m * w + 3) // 4 * 4

        def alloc(name, shape):
            v = views.get(name)
            return v if v is not None else torch.empty(shape, device=d, dtype=torch.float32)

        new = dn.apply_event(plan, named, scales, quats_n, noise, thresholds["log_split"], alloc)
        self.geometry_flat = flat
        for group, attr in attrs.items():
            setattr(self, attr, torch.nn.Parameter(new[group]))
        after = self.param_groups()
        for g in opt.param_groups:
            old, p = before[g["name"]][0], after[g["name"]][0]
            g["params"] = [p]
            st = opt.state.pop(old, None)
            if st:
                st = dict(st)  # (the step count is kept)
                if "exp_avg" in st:
                    st["exp_avg"], st["exp_avg_sq"] = new[g["name"] + ".exp_avg"], new[g["name"] + ".exp_avg_sq"]
                opt.state[p] = st
        self.texture_dims = one_texel_dims(m)
        self.n_texels = m
        self.mappings = (1.0 / (2.0 * 3.0 * torch.exp(self.scales.detach()[:, :2]))).contiguous()
        if self.defer_texture:  # fresh persistent gradient buffers for the new texel store
            self.texel_grad.own(self.texture_dc, self.fused_step)
        self.texel_grad.reset()
        self._paint_acc, self._paint_scratch, self.test_colors, self._last_vis = None, {}, None, None
        return plan

    # ------------------------------------------------------------------ selection
    @torch.no_grad()
    def select(self, keep):
        """Keep the splats with keep[i] (a bool (n,) tensor on the trainer's device or the CPU), whatever their charts'
        sizes (gstex_amd.select; DESIGN.md "Selecting splats"): plan, two scans, one read-back, then every per-splat
        parameter's rows gathered and the texel store's kept blocks compacted into fresh tensors, with the Adam moments
        the optimizer holds (kept rows and kept texels keep exp_avg and exp_avg_sq: no value changes, unlike
        recharge(); every step count is kept).  Rebuilt for n_after splats and T_new texels: geometry_flat and its four
        views, features_dc / features_rest, mappings (rows gathered, not recomputed: after a rechart they reflect the
        scales at rechart time and the render must not change), texture_dims, n_texels, texture_dc (exactly T_new rows,
        without spare capacity; one zero row when T_new == 0, since an empty store has no address to hand the raster),
        the optimizer's groups and state and the texel gradient's buffers; the paint accumulator and scratch, the test
        colours and the last visibility are dropped; the pair capacity, step_control and pixel_num stay.  ValueError on a
        keep of the wrong shape or dtype or a malformed texture_dims row, RuntimeError under GradSync or when no splat
        would remain, all with the trainer untouched; an all-true mask returns with the trainer untouched.  A
        DensityController built for the old n must be rebuilt by the caller.  On a CPU trainer the eager twins run
        instead of the kernels.  -> Selection(n_before, n_after, texels_before, texels_after)."""
        from . import select as sel

        n, d = self.means.shape[0], self.device
        if self.texel_grad.routed:
            raise RuntimeError("select: selection on a trainer under GradSync is not supported")
        if not (isinstance(keep, torch.Tensor) and keep.dtype == torch.bool and tuple(keep.shape) == (n,)):
            raise ValueError(f"select: keep must be a bool ({n},) tensor")
        self.wait_texture()
        dims, t_old = self.texture_dims, self.n_texels
        plan = sel.plan_selection(dims, t_old, keep.to(dims.device))
        if plan.flagged:
            raise ValueError(f"select: {sel._MALFORMED} (n_texels = {t_old})")
        if plan.n_new == 0:
            raise RuntimeError("select: the mask would drop every splat")
        if plan.n_new == n:
            return sel.Selection(n, n, t_old, t_old)
        opt, before = self.optimizer, self.param_groups()
        attrs = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest",
                 "opacity": "opacities", "scaling": "scales", "rotation": "quats", "texture_dc": "texture_dc"}

        def moments(p):  # the two Adam moments the optimizer holds for p, or none
            st = opt.state.get(p) or {}
            return [st["exp_avg"], st["exp_avg_sq"]] if "exp_avg" in st else []

        named = {"mappings": self.mappings}
        for group, (p,) in before.items():
            if group == "texture_dc":
                continue
            named[group] = p.detach()
            for k, m in zip(("exp_avg", "exp_avg_sq"), moments(p)):
                named[f"{group}.{k}"] = m
        # the geometry parameters' shared allocation, segments 16-B aligned (as __init__)
        m = plan.n_new
        geo = [("xyz", 3), ("scaling", 3), ("rotation", 4), ("opacity", 1)]
        flat = torch.zeros(sum((m * w + 3) // 4 * 4 for _, w in geo), device=d, dtype=torch.float32)
        views, off = {}, 0
        for group, w in geo:
            views[group] = flat[off:off + m * w].view(m, w)
            off += (m * w + 3) // 4 * 4

        def alloc(name, shape):
            v = views.get(name)
            return v if v is not None else torch.empty(shape, device=d, dtype=torch.float32)

        new = sel.select_rows(plan, named, alloc)
        t_new = plan.n_texels_new
        tex = self.texture_dc
        srcs = [tex.detach()] + moments(tex)
        if t_new == 0:  # only zero-texel charts are left: one zero row stands in for the empty store
            new_dims, _ = sel.select_dims(dims, plan)
            stores = [s.new_zeros((1,) + tuple(s.shape[1:])) for s in srcs]
        else:
            new_dims, stores = sel.apply_selection(dims, t_old, plan, srcs)
        new["texture_dc"] = stores[0]
        if len(stores) == 3:
            new["texture_dc.exp_avg"], new["texture_dc.exp_avg_sq"] = stores[1], stores[2]
        self.geometry_flat = flat
        for group, attr in attrs.items():
            setattr(self, attr, torch.nn.Parameter(new[group]))
        after = self.param_groups()
        for g in opt.param_groups:
            old, p = before[g["name"]][0], after[g["name"]][0]
            g["params"] = [p]
            st = opt.state.pop(old, None)
            if st:
                st = dict(st)  # (the step count is kept)
                if "exp_avg" in st:
                    st["exp_avg"], st["exp_avg_sq"] = new[g["name"] + ".exp_avg"], new[g["name"] + ".exp_avg_sq"]
                opt.state[p] = st
        self.mappings = new["mappings"]
        self.texture_dims = new_dims
        self.n_texels = t_new
        if self.defer_texture:  # fresh persistent gradient buffers for the new texel store
            self.texel_grad.own(self.texture_dc, self.fused_step)
        self.texel_grad.reset()
        self._paint_acc, self._paint_scratch, self.test_colors, self._last_vis = None, {}, None, None
        return sel.Selection(n, m, t_old, t_new)

    @torch.no_grad()
    def reset_opacity(self, value: float = 0.01):
        """The lineage's periodic opacity reset: every opacity logit capped at logit(value), the opacity parameter's
        two Adam moments zeroed (its step count kept).  Plain torch: it runs once per 3,000 steps."""
        import math

        self.opacities.data.clamp_(max=math.log(value / (1.0 - value)))
        st = self.optimizer.state.get(self.opacities)
        if st and "exp_avg" in st:
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
