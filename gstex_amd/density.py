"""Adaptive density control: clone, split and prune one-texel splats while training (not in the reference, whose
pipeline disables culling and densification; the rules are the published method's, 3DGS section 5.2 as 2DGS uses it).

* DensityController   the per-step statistics, the event schedule and the opacity reset around a GStexTrainer
* density_accum / density_plan / density_apply   the HIP entry points (gstex_amd/csrc/density.hip)
* density_*_eager     their eager torch twins, operation for operation, usable on CPU tensors: every kernel operation is
                      one correctly rounded fp32 + - * / sqrt in a fixed order and every decision compares against a
                      threshold formed here on the host, so kernel and twin agree bit for bit (DESIGN.md "Density control")
* scene_extent        the lineage's cameras_extent
* GEOMETRY_STAGE      the lineage's settings of the stage that trains a point cloud into a 2DGS checkpoint

One event: plan (rows[i] in {0, 1, 2}, kind[i]) -> the exclusive scan of rows (the binning's scan) -> ONE read-back
(the new splat count with the event's tallies) -> apply (every per-splat tensor and Adam moment scattered to its rows in
source order).  When the first plan would exceed `max_splats` the event is planned again as prune-only, which costs a
second read-back.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import (DENSITY_CLONE as CLONE, DENSITY_KEEP as KEEP, DENSITY_PRUNE as PRUNE, DENSITY_ROLE_COPY as ROLE_COPY,
                   DENSITY_ROLE_LOG_SCALES as ROLE_LOG_SCALES, DENSITY_ROLE_MEANS as ROLE_MEANS,
                   DENSITY_ROLE_MOMENT as ROLE_MOMENT, DENSITY_SPLIT as SPLIT, ptr)

# the lineage's geometry stage (2DGS arguments/__init__.py: OptimizationParams, ModelParams).  The means' rates are per
# unit of scene_extent: lrs["xyz"] = xyz_lr * extent, decayed to xyz_lr_final * extent over xyz_max_steps.
GEOMETRY_STAGE = dict(
    max_steps=30000, xyz_lr=1.6e-4, xyz_lr_final=1.6e-6, xyz_max_steps=30000,
    lrs={"features_dc": 0.0025, "features_rest": 0.0025 / 20, "opacity": 0.05, "scaling": 0.005, "rotation": 0.001,
         "texture_dc": 1e-3},  # gstex_amd.train._COMMON_LRS
    lambda_normal=[0.0, 0.05, 7000], sh_degree=3, sh_degree_interval=1000,
    density=dict(grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_screen_px=20.0, start=500, stop=15000,
                 every=100, reset_every=3000))


def geometry_stage_lrs(extent: float) -> dict:
    """The seven groups' learning rates of GEOMETRY_STAGE for a scene of this extent (GStexTrainer(lrs=...))."""
    return {"xyz": GEOMETRY_STAGE["xyz_lr"] * float(extent), **GEOMETRY_STAGE["lrs"]}


def scene_extent(views) -> float:
    """1.1 x the largest distance of a camera centre from the centres' mean (the lineage's cameras_extent)."""
    centres = torch.stack([v.c2w[:3, 3].detach().double().cpu() for v in views])
    if centres.shape[0] == 0:
        raise ValueError("scene_extent: no views")
    return 1.1 * float((centres - centres.mean(dim=0, keepdim=True)).norm(dim=1).max())


def _f32(x: float) -> float:
    return float(np.float32(x))


def density_thresholds(extent: float, *, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005,
                       max_screen_px=20.0) -> dict:
    """The fp32 thresholds gstex_density_plan compares against, formed once in double and rounded once: the plan works
    in the log / logit domain, so it has no transcendental and no decision can differ by an ulp of exp."""
    if not (extent > 0 and math.isfinite(extent)):
        raise ValueError(f"extent must be finite and > 0 (got {extent})")
    if not 0.0 < min_opacity < 1.0:
        raise ValueError(f"min_opacity must be in (0, 1) (got {min_opacity})")
    if not (grad_threshold >= 0 and percent_dense > 0 and math.isfinite(max_screen_px)):
        raise ValueError("grad_threshold must be >= 0, percent_dense > 0 and max_screen_px finite")
    return dict(grad_threshold=_f32(grad_threshold), log_big=_f32(math.log(percent_dense * extent)),
                logit_faint=_f32(math.log(min_opacity / (1.0 - min_opacity))), max_screen_px=_f32(max_screen_px),
                log_world=_f32(math.log(0.1 * extent)), log_split=_f32(math.log(1.6)))


# ---------------------------------------------------------------------------------------- eager twins
def _s(v, like: torch.Tensor) -> torch.Tensor:
    """A python number as a 0-dim fp32 tensor (rounded once, as the C call rounds its float arguments)."""
    return torch.tensor(float(v), dtype=torch.float32, device=like.device)


def _sqrt32(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root, as the kernels compute it.  torch's CPU sqrt goes through a vector
    library that is not correctly rounded on every build; the fp64 root rounded once is (53 >= 2 * 24 + 2 bits, so the
    double rounding is innocuous)."""
    return torch.sqrt(x.double()).float()


def density_accum_eager(means, v_means, viewmat, fx, fy, H, W, num_tiles_hit, extents, grad_sum, count, max_extent,
                        skip=None):
    """gstex_density_accum restated: -> the new (grad_sum, count, max_extent).  skip: the guard flag (non-zero: the
    statistics come back unchanged)."""
    if skip is not None and float(torch.as_tensor(skip).reshape(-1)[0]) != 0.0:
        return grad_sum.clone(), count.clone(), max_extent.clone()
    V = viewmat.detach().to(torch.float32)
    x, y, zw = means[:, 0], means[:, 1], means[:, 2]
    gx, gy, gz = v_means[:, 0], v_means[:, 1], v_means[:, 2]
    hw, hh = _s(0.5, means) * _s(W, means), _s(0.5, means) * _s(H, means)
    z = ((V[2, 0] * x + V[2, 1] * y) + V[2, 2] * zw) + V[2, 3]
    gcx = (V[0, 0] * gx + V[0, 1] * gy) + V[0, 2] * gz
    gcy = (V[1, 0] * gx + V[1, 1] * gy) + V[1, 2] * gz
    ax = ((gcx * z) / _s(fx, means)) * hw
    ay = ((gcy * z) / _s(fy, means)) * hh
    norm = _sqrt32(ax * ax + ay * ay)
    seen = num_tiles_hit > 0
    return (torch.where(seen, grad_sum + norm, grad_sum), torch.where(seen, count + 1.0, count),
            torch.where(seen, torch.maximum(max_extent, torch.maximum(extents[:, 0], extents[:, 1])), max_extent))


_ROWS_OF_KIND = (1, 2, 2, 0)  # KEEP, CLONE, SPLIT, PRUNE


def density_plan_eager(log_scales, opac_logits, grad_sum, count, max_extent, thresholds: dict, size_prune: bool,
                       prune_only: bool = False):
    """gstex_density_plan and the scan restated: -> (rows (n,) int32, kind (n,) int32, offsets (n + 1,) int32)."""
    t = {k: _s(v, log_scales) for k, v in thresholds.items()}
    m = torch.maximum(log_scales[:, 0], log_scales[:, 1])
    hot = (count > 0) & (grad_sum >= t["grad_threshold"] * count)
    if prune_only:
        hot = torch.zeros_like(hot)
    big = m > t["log_big"]
    faint = opac_logits.reshape(-1) < t["logit_faint"]
    no = torch.zeros_like(hot)
    child_too_big = ((m - t["log_split"]) > t["log_world"]) if size_prune else no
    size = ((max_extent > t["max_screen_px"]) | (m > t["log_world"])) if size_prune else no
    kind = torch.full_like(m, KEEP, dtype=torch.int32)
    pick = lambda c, v, k: torch.where(c, torch.full_like(k, v), k)  # noqa: E731  (later picks take precedence)
    kind = pick(hot, CLONE, kind)
    kind = pick(size, PRUNE, kind)
    kind = pick(hot & big & ~child_too_big, SPLIT, kind)
    kind = pick(hot & big & child_too_big, PRUNE, kind)
    kind = pick(faint, PRUNE, kind)
    rows = torch.tensor(_ROWS_OF_KIND, dtype=torch.int32, device=kind.device)[kind.long()]
    offsets = torch.cat([rows.new_zeros(1), torch.cumsum(rows, 0, dtype=torch.int32)])
    return rows, kind, offsets


def _frame_columns(quats_n):
    """gstex_common.h quat_frame on the normalised quaternions: -> R[:, :, 0], R[:, :, 1] as (n, 3) each."""
    w, x, y, z = quats_n[:, 0], quats_n[:, 1], quats_n[:, 2], quats_n[:, 3]
    nrm = _sqrt32(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    r00 = 1.0 - 2.0 * (y * y + z * z)
    r01 = 2.0 * (x * y - w * z)
    r10 = 2.0 * (x * y + w * z)
    r11 = 1.0 - 2.0 * (x * x + z * z)
    r20 = 2.0 * (x * z - w * y)
    r21 = 2.0 * (y * z + w * x)
    return torch.stack([r00, r10, r20], -1), torch.stack([r01, r11, r21], -1)


def density_apply_eager(rows, kind, offsets, named: dict, scales, quats_n, noise, log_split: float) -> dict:
    """gstex_density_apply restated.  named: {name: (tensor (n, ...), role)} -> {name: tensor (n_new, ...)}: splat i's
    rows at offsets[i], in source order (keep then clone, or child 0 then child 1)."""
    n = rows.shape[0]
    src = torch.repeat_interleave(torch.arange(n, device=rows.device), rows.long())  # the source splat of each new row
    r = torch.arange(src.shape[0], device=rows.device) - offsets.long()[src]  # 0: keep / child 0; 1: clone / child 1
    split = kind[src] == SPLIT
    out = {}
    for name, (t, role) in named.items():
        flat = t.detach().reshape(n, t.numel() // n if n else 0)
        new = flat[src]
        if role == ROLE_MOMENT:
            new = torch.where(((r == 0) & ~split)[:, None], new, torch.zeros_like(new))
        elif role == ROLE_MEANS:
            c0, c1 = _frame_columns(quats_n)
            a = scales[src, 0] * noise[src, r, 0]
            b = scales[src, 1] * noise[src, r, 1]
            child = new + ((c0[src] * a[:, None]) + (c1[src] * b[:, None]))
            new = torch.where(split[:, None], child, new)
        elif role == ROLE_LOG_SCALES:
            shrunk = new - _s(log_split, new)
            cols = torch.arange(new.shape[1], device=new.device) < 2
            new = torch.where(split[:, None] & cols[None, :], shrunk, new)
        out[name] = new.reshape((src.shape[0],) + tuple(t.shape[1:])).contiguous()
    return out


# ---------------------------------------------------------------------------------------- HIP entry points
def _dev_f32(t, name, shape):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)
            and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous HIP float32 tensor of shape {tuple(shape)}")
    return t


def density_accum(means, v_means, view, num_tiles_hit, extents, skip, grad_sum, count, max_extent) -> None:
    """gstex_density_accum: the statistics updated in place from one step's means gradient and visibility.  One
    launch, no read-back, no allocation.  skip: the step's guard flag (a 1-element device tensor) or None."""
    n = means.shape[0]
    _dev_f32(means.detach(), "means", (n, 3))
    _dev_f32(v_means, "v_means", (n, 3))
    _dev_f32(extents, "extents", (n, 2))
    for name, t in (("grad_sum", grad_sum), ("count", count), ("max_extent", max_extent)):
        _dev_f32(t, name, (n,))
    if not (num_tiles_hit.is_cuda and num_tiles_hit.dtype == torch.int32 and tuple(num_tiles_hit.shape) == (n,)
            and num_tiles_hit.is_contiguous()):
        raise ValueError(f"num_tiles_hit: expected a contiguous HIP int32 tensor of shape ({n},)")
    vm = view.viewmat.detach()
    vm = vm if (vm.dtype == torch.float32 and vm.is_contiguous()) else vm.float().contiguous()
    cam = _lib.make_camera(vm, None, view.fx, view.fy, view.cx, view.cy, view.H, view.W, 16)
    _lib.call("gstex_density_accum", n, ptr(means), ptr(v_means), ctypes.byref(cam), ptr(num_tiles_hit), ptr(extents),
              ptr(skip), ptr(grad_sum), ptr(count), ptr(max_extent), _lib.stream_of(means.device))


def density_plan(log_scales, opac_logits, grad_sum, count, max_extent, thresholds: dict, size_prune: bool,
                 prune_only: bool = False):
    """gstex_density_plan, then the binning's scan over rows: -> (rows, kind, offsets), all on the device."""
    from .ops import _scan_offsets

    n = log_scales.shape[0]
    _dev_f32(log_scales.detach(), "log_scales", (n, 3))
    _dev_f32(opac_logits.detach().reshape(-1), "opac_logits", (n,))
    for name, t in (("grad_sum", grad_sum), ("count", count), ("max_extent", max_extent)):
        _dev_f32(t, name, (n,))
    rows = torch.empty((n,), device=log_scales.device, dtype=torch.int32)
    kind = torch.empty((n,), device=log_scales.device, dtype=torch.int32)
    a = _lib.GstexDensityPlanArgs(
        n=n, size_prune=int(bool(size_prune)), prune_only=int(bool(prune_only)), log_scales=ptr(log_scales),
        opac_logits=ptr(opac_logits), grad_sum=ptr(grad_sum), count=ptr(count), max_extent=ptr(max_extent),
        rows=ptr(rows), kind=ptr(kind), **thresholds)
    _lib.call("gstex_density_plan", ctypes.byref(a), _lib.stream_of(log_scales.device))
    return rows, kind, _scan_offsets(rows)


def density_apply(rows, kind, offsets, n_new: int, named: dict, scales, quats_n, noise, log_split: float,
                  alloc=None) -> dict:
    """gstex_density_apply: named {name: (tensor (n, ...), role)} -> {name: a fresh tensor (n_new, ...)}, one launch
    per GSTEX_DENSITY_MAX_TENSORS tensors.  alloc(name, shape): where a result goes (default: torch.empty)."""
    n = rows.shape[0]
    dev = rows.device
    _dev_f32(scales, "scales", (n, 3))
    _dev_f32(quats_n, "quats_n", (n, 4))
    _dev_f32(noise, "noise", (n, 2, 2))
    out, descs = {}, []
    for name, (t, role) in named.items():
        src = t.detach()
        if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.shape[0] == n):
            raise ValueError(f"{name}: expected a contiguous HIP float32 tensor of {n} rows")
        shape = (n_new,) + tuple(src.shape[1:])
        dst = alloc(name, shape) if alloc is not None else torch.empty(shape, device=dev, dtype=torch.float32)
        if not (dst.is_contiguous() and tuple(dst.shape) == shape and dst.dtype == torch.float32 and dst.device == dev):
            raise ValueError(f"{name}: the destination must be a contiguous float32 {shape} tensor on {dev}")
        out[name] = dst
        width = src.numel() // n if n else 0
        descs.append(_lib.GstexDensityTensor(ptr(src), ptr(dst), width, int(role)))
    for i in range(0, len(descs), _lib.DENSITY_MAX_TENSORS):
        chunk = descs[i:i + _lib.DENSITY_MAX_TENSORS]
        arr = (_lib.GstexDensityTensor * len(chunk))(*chunk)
        a = _lib.GstexDensityApplyArgs(
            n=n, n_tensors=len(chunk), n_new=int(n_new), log_split=float(log_split), rows=ptr(rows), kind=ptr(kind),
            offsets=ptr(offsets), scales=ptr(scales), quats_n=ptr(quats_n), noise=ptr(noise), tensors=arr)
        _lib.call("gstex_density_apply", ctypes.byref(a), _lib.stream_of(dev))
    return out


class DensityPlan(NamedTuple):
    rows: torch.Tensor
    kind: torch.Tensor
    offsets: torch.Tensor
    n_new: int
    kept: int
    cloned: int
    split: int
    pruned: int
    prune_only: bool
    flagged: bool  # the caller's `check` flag, read back with the counts


def plan_event(log_scales, opac_logits, grad_sum, count, max_extent, thresholds: dict, size_prune: bool,
               max_splats: int | None = None, check: torch.Tensor | None = None) -> DensityPlan:
    """Plan, scan and the event's read-back: on HIP tensors through the kernels, on CPU tensors through the twins.
    check: a 0-dim bool tensor of the caller's (a precondition evaluated on the device), returned as `flagged` from the
    same read-back.  The cap: a first plan whose n_new exceeds max_splats is replaced by a prune-only plan."""
    fn = density_plan if log_scales.is_cuda else density_plan_eager
    n = log_scales.shape[0]
    flag = torch.zeros(1, dtype=torch.int64, device=log_scales.device) if check is None else check.reshape(1).long()
    for prune_only in (False, True):
        rows, kind, offsets = fn(log_scales.detach(), opac_logits.detach().reshape(-1), grad_sum, count, max_extent,
                                 thresholds, size_prune, prune_only)
        tally = torch.cat([offsets[n:n + 1].long(), torch.bincount(kind.long(), minlength=4)[:4], flag]).cpu().tolist()
        if prune_only or max_splats is None or tally[0] <= int(max_splats):
            break
    return DensityPlan(rows, kind, offsets, int(tally[0]), int(tally[1 + KEEP]), int(tally[1 + CLONE]),
                       int(tally[1 + SPLIT]), int(tally[1 + PRUNE]), bool(prune_only), bool(tally[5]))


def apply_event(plan: DensityPlan, named: dict, scales, quats_n, noise, log_split: float, alloc=None) -> dict:
    """The plan's scatter: gstex_density_apply on HIP tensors, density_apply_eager on CPU tensors."""
    if plan.rows.is_cuda:
        return density_apply(plan.rows, plan.kind, plan.offsets, plan.n_new, named, scales, quats_n, noise, log_split,
                             alloc)
    out = density_apply_eager(plan.rows, plan.kind, plan.offsets, named, scales, quats_n, noise, log_split)
    if alloc is not None:
        for name, t in out.items():
            dst = alloc(name, tuple(t.shape))
            dst.copy_(t)
            out[name] = dst
    return out


# ---------------------------------------------------------------------------------------- the controller
class DensityEvent(NamedTuple):
    step: int
    n_before: int
    n_after: int
    cloned: int
    split: int
    pruned: int


class DensityController:
    """The lineage's densification schedule around a one-texel GStexTrainer.  With s the trainer's step counter after
    the optimizer step (the lineage's 1-based iteration):

    * accumulate(trainer, view): after the backward, before the Adam step, while s < stop: the step's statistics;
    * update(trainer): after the Adam step, while s < stop: an event when s > start and s % every == 0 (size pruning only
      once s > reset_every), then the opacity reset when s % reset_every == 0 (reset_every 0 or None: neither).

    The split noise comes from the controller's own device generator (seeded like the trainer's background_seed)."""

    def __init__(self, n: int, device, extent: float, *, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005,
                 max_screen_px=20.0, start=500, stop=15000, every=100, reset_every=3000, max_splats=None, seed=0):
        if int(every) <= 0:
            raise ValueError(f"every must be > 0 (got {every})")
        self.device = torch.device(device)
        self.extent = float(extent)
        self.thresholds = density_thresholds(self.extent, grad_threshold=grad_threshold, percent_dense=percent_dense,
                                             min_opacity=min_opacity, max_screen_px=max_screen_px)
        self.start, self.stop, self.every = int(start), int(stop), int(every)
        self.reset_every = int(reset_every) if reset_every else 0
        self.max_splats = None if max_splats is None else int(max_splats)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self.events: list[DensityEvent] = []
        self._zero_stats(int(n))

    def _zero_stats(self, n: int):
        z = lambda: torch.zeros((n,), device=self.device, dtype=torch.float32)  # noqa: E731
        self.grad_sum, self.count, self.max_extent = z(), z(), z()

    def accumulate(self, trainer, view) -> None:
        if trainer.step + 1 >= self.stop:
            return
        vis = trainer.last_visibility
        grad = trainer.means.grad
        if vis is None or grad is None:
            raise RuntimeError("DensityController.accumulate: no differentiable render / backward since the last step")
        nth, extents = vis
        if grad.shape[0] != self.grad_sum.shape[0] or nth.shape[0] != grad.shape[0]:
            raise ValueError("DensityController.accumulate: the statistics and the trainer disagree on the splat count")
        skip = trainer._skip_flag()
        if self.device.type == "cuda":
            density_accum(trainer.means, grad.contiguous(), view, nth, extents, skip, self.grad_sum, self.count,
                          self.max_extent)
        else:
            self.grad_sum, self.count, self.max_extent = density_accum_eager(
                trainer.means.detach(), grad, view.viewmat, view.fx, view.fy, view.H, view.W, nth, extents,
                self.grad_sum, self.count, self.max_extent, skip)

    def update(self, trainer):
        s = trainer.step
        if s >= self.stop:
            return None
        event = None
        if s > self.start and s % self.every == 0:
            n = trainer.means.shape[0]
            noise = torch.randn((n, 2, 2), generator=self.generator, device=self.device, dtype=torch.float32)
            plan = trainer.apply_density(self.grad_sum, self.count, self.max_extent, noise, self.thresholds,
                                         size_prune=bool(self.reset_every) and s > self.reset_every,
                                         max_splats=self.max_splats)
            self._zero_stats(plan.n_new)
            event = DensityEvent(s, n, plan.n_new, plan.cloned, plan.split, plan.pruned)
            self.events.append(event)
        if self.reset_every and s % self.reset_every == 0:
            trainer.reset_opacity(0.01)
        return event
