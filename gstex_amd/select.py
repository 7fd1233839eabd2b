"""Keep a subset of the splats of a textured model: the per-splat tensors' rows gathered and the jagged texel store
compacted by a per-splat mask (not in the reference, whose clustering tool writes a new file; DESIGN.md "Selecting
splats").

* select_texture        (texture_dims, n_texels, keep, tensors) -> (new_dims, new_tensors, n_texels_new): plan, dims and
                        the jagged gather of the texel tensors sharing the charts (a parameter and its two Adam moments
                        in one pass); HIP tensors run the kernels of gstex_amd/csrc/select.hip, CPU
                        tensors the eager twin
* select_plan / select_dims / select_texels / select_rows     the steps, each on HIP or CPU tensors
* select_texture_eager  the twin: repeat_interleave plus index arithmetic (what the tests compare against and what a
                        CPU trainer runs)
* plan_selection        plan, both scans and the operation's ONE read-back (n_new, T_new, flag) -> SelectPlan
* Selection             what GStexTrainer.select returns

The store: chart i's h_i * w_i texels are rows [offset_i, offset_i + h_i * w_i) of every texel tensor, texture_dims
(n, 3) int32 = (h, w, offset); blocks may lie in any order and a tensor may have spare rows past n_texels, which are
never read.  The result holds the kept charts' blocks back to back in splat order: new offsets are the exclusive sum
of the kept h * w.  Values are copied, never rounded, so kernels and twin agree exactly.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib
from ._lib import DENSITY_ROLE_COPY as ROLE_COPY, ptr

INT32_MAX = (1 << 31) - 1


class Selection(NamedTuple):
    n_before: int
    n_after: int
    texels_before: int
    texels_after: int


class SelectPlan(NamedTuple):
    keep: torch.Tensor     # (n,) bool, contiguous, on the dims' device
    rows: torch.Tensor     # (n,) int32: 1 kept, 0 dropped
    texels: torch.Tensor   # (n,) int32: h * w of a kept splat, else 0
    row_off: torch.Tensor  # (n + 1,) int32: the exclusive scan of rows
    tex_off: torch.Tensor  # (n + 1,) int32: the exclusive scan of texels
    n_new: int
    n_texels_new: int
    flagged: bool          # some dims row, kept or not, is malformed


def _check(texture_dims, n_texels, keep):
    if not (isinstance(texture_dims, torch.Tensor) and texture_dims.dim() == 2 and texture_dims.shape[1] == 3
            and texture_dims.dtype == torch.int32):
        raise ValueError("texture_dims: expected an int32 (n, 3) tensor")
    n = texture_dims.shape[0]
    if not (isinstance(keep, torch.Tensor) and keep.dtype == torch.bool and tuple(keep.shape) == (n,)):
        raise ValueError(f"keep: expected a bool ({n},) tensor")
    if not 0 <= int(n_texels) <= INT32_MAX:
        raise ValueError(f"n_texels must be in [0, 2^31) (got {n_texels})")
    return texture_dims.contiguous(), keep.to(texture_dims.device).contiguous()


# ---------------------------------------------------------------------------------------- eager twins
def _scan_eager(x):
    """gstex_scan_offsets restated: the exclusive int32 sum, (n + 1,)."""
    return torch.cat([x.new_zeros(1), torch.cumsum(x, 0, dtype=torch.int32)])


def select_plan_eager(texture_dims, n_texels: int, keep):
    """gstex_select_plan and the two scans restated: -> (rows, texels, row_off, tex_off, flag (1,) int32)."""
    d = texture_dims.long()
    h, w, off = d[:, 0], d[:, 1], d[:, 2]
    hw = h * w
    bad = (h < 0) | (w < 0) | (off < 0) | (hw > INT32_MAX) | (off + hw > int(n_texels))
    rows = keep.to(torch.int32)
    texels = torch.where(keep & ~bad, hw, torch.zeros_like(hw)).to(torch.int32)
    return rows, texels, _scan_eager(rows), _scan_eager(texels), bad.any().to(torch.int32).reshape(1)


def select_dims_eager(texture_dims, keep, tex_off):
    """gstex_select_dims restated: -> (new_dims (n_new, 3), src_off (n_new,))."""
    kept = torch.nonzero(keep, as_tuple=True)[0]
    new_dims = texture_dims[kept].clone()
    new_dims[:, 2] = tex_off[kept]
    return new_dims.contiguous(), texture_dims[kept, 2].contiguous()


def select_texels_eager(new_dims, src_off, tensors):
    """gstex_select_texels restated: the source row of every destination texel by repeat_interleave, one index_select
    per tensor."""
    size = new_dims[:, 0].long() * new_dims[:, 1].long()
    chart = torch.repeat_interleave(torch.arange(size.shape[0], device=size.device), size)
    local = torch.arange(chart.shape[0], device=size.device) - new_dims[:, 2].long()[chart]
    src = src_off.long()[chart] + local
    return [t.detach().index_select(0, src).contiguous() for t in tensors]


def select_texture_eager(texture_dims, n_texels: int, keep, tensors):
    """The twin of select_texture: -> (new_dims, new_tensors, n_texels_new).  ValueError on a malformed dims row."""
    texture_dims, keep = _check(texture_dims, n_texels, keep)
    _, _, _, tex_off, flag = select_plan_eager(texture_dims, n_texels, keep)
    if int(flag):
        raise ValueError(_MALFORMED)
    new_dims, src_off = select_dims_eager(texture_dims, keep, tex_off)
    return new_dims, select_texels_eager(new_dims, src_off, tensors), int(tex_off[-1])


def select_rows_eager(keep, named: dict) -> dict:
    """select_rows restated: the kept rows of every per-splat tensor, in order."""
    kept = torch.nonzero(keep, as_tuple=True)[0]
    return {name: t.detach().index_select(0, kept).contiguous() for name, t in named.items()}


# ---------------------------------------------------------------------------------------- HIP entry points
_MALFORMED = ("texture_dims has a malformed row: h < 0, w < 0, offset < 0, h * w above 2^31 - 1 or "
              "offset + h * w > n_texels")


def _dev_i32(t, name, shape):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == tuple(shape)
            and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous HIP int32 tensor of shape {tuple(shape)}")
    return t


def select_plan(texture_dims, n_texels: int, keep):
    """gstex_select_plan, then the binning's scan over rows and over texels: -> (rows, texels, row_off, tex_off, flag),
    all on the dims' device, nothing read back.  CPU tensors: the twin."""
    texture_dims, keep = _check(texture_dims, n_texels, keep)
    if not texture_dims.is_cuda:
        return select_plan_eager(texture_dims, n_texels, keep)
    from .ops import _scan_offsets

    n, dev = texture_dims.shape[0], texture_dims.device
    rows = torch.empty((n,), device=dev, dtype=torch.int32)
    texels = torch.empty((n,), device=dev, dtype=torch.int32)
    flag = torch.zeros((1,), device=dev, dtype=torch.int32)
    a = _lib.GstexSelectPlanArgs(n=n, n_texels=int(n_texels), keep=ptr(keep), texture_dims=ptr(texture_dims),
                                 rows=ptr(rows), texels=ptr(texels), flag=ptr(flag))
    _lib.call("gstex_select_plan", ctypes.byref(a), _lib.stream_of(dev))
    return rows, texels, _scan_offsets(rows), _scan_offsets(texels), flag


def plan_selection(texture_dims, n_texels: int, keep) -> SelectPlan:
    """select_plan and the operation's one read-back: (n_new, T_new, flag) in a single device-to-host copy."""
    texture_dims, keep = _check(texture_dims, n_texels, keep)
    rows, texels, row_off, tex_off, flag = select_plan(texture_dims, n_texels, keep)
    n = rows.shape[0]
    n_new, t_new, flagged = torch.cat([row_off[n:n + 1], tex_off[n:n + 1], flag]).cpu().tolist()
    # (blocks that overlap can sum past int32: a negative total is a malformed store as well)
    return SelectPlan(keep, rows, texels, row_off, tex_off, int(n_new), int(t_new), bool(flagged) or int(t_new) < 0)


def select_dims(texture_dims, plan: SelectPlan):
    """gstex_select_dims: -> (new_dims (n_new, 3) int32, src_off (n_new,) int32).  CPU tensors: the twin."""
    if not texture_dims.is_cuda:
        return select_dims_eager(texture_dims, plan.keep, plan.tex_off)
    n, dev = texture_dims.shape[0], texture_dims.device
    _dev_i32(texture_dims, "texture_dims", (n, 3))
    _dev_i32(plan.row_off, "row_off", (n + 1,))
    _dev_i32(plan.tex_off, "tex_off", (n + 1,))
    new_dims = torch.empty((plan.n_new, 3), device=dev, dtype=torch.int32)
    src_off = torch.empty((plan.n_new,), device=dev, dtype=torch.int32)
    a = _lib.GstexSelectDimsArgs(n=n, n_new=plan.n_new, keep=ptr(plan.keep), texture_dims=ptr(texture_dims),
                                 row_off=ptr(plan.row_off), tex_off=ptr(plan.tex_off), new_dims=ptr(new_dims),
                                 src_off=ptr(src_off))
    _lib.call("gstex_select_dims", ctypes.byref(a), _lib.stream_of(dev))
    return new_dims, src_off


def _texel_tensors(tensors, n_texels, dev):
    tensors = [t.detach() for t in tensors]
    if not tensors:
        return tensors, 0
    tail = tuple(tensors[0].shape[1:])
    for k, t in enumerate(tensors):
        if not (t.dim() >= 2 and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                and t.shape[0] >= n_texels and tuple(t.shape[1:]) == tail):
            raise ValueError(f"tensors[{k}]: expected a contiguous float32 tensor on {dev} of at least {n_texels} rows "
                             f"of shape {tail}")
    channels = 1
    for s in tail:
        channels *= int(s)
    if not 1 <= channels <= 8:
        raise ValueError(f"tensors: between 1 and 8 floats per texel (got {channels})")
    return tensors, channels


def select_texels(new_dims, src_off, n_texels: int, n_texels_new: int, tensors, alloc=None):
    """gstex_select_texels: every tensor's kept blocks gathered into a fresh (n_texels_new, ...) tensor, one launch per
    GSTEX_SELECT_MAX_TENSORS tensors.  alloc(k, shape): where result k goes (default: torch.empty); it must not
    overlap its source.  CPU tensors: the twin."""
    dev = new_dims.device
    tensors, channels = _texel_tensors(tensors, n_texels, dev)
    shape = lambda t: (int(n_texels_new),) + tuple(t.shape[1:])  # noqa: E731
    if alloc is None:
        alloc = lambda k, s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    if not new_dims.is_cuda:
        out = []
        for k, t in enumerate(select_texels_eager(new_dims, src_off, tensors)):
            dst = alloc(k, shape(t))
            dst.copy_(t)
            out.append(dst)
        return out
    n_new = new_dims.shape[0]
    _dev_i32(new_dims, "new_dims", (n_new, 3))
    _dev_i32(src_off, "src_off", (n_new,))
    out = []
    for k, t in enumerate(tensors):
        dst = alloc(k, shape(t))
        if not (dst.is_contiguous() and tuple(dst.shape) == shape(t) and dst.dtype == torch.float32
                and dst.device == dev):
            raise ValueError(f"tensors[{k}]: the destination must be a contiguous float32 {shape(t)} tensor on {dev}")
        out.append(dst)
    for i in range(0, len(tensors), _lib.SELECT_MAX_TENSORS):
        a = _lib.GstexSelectTexelsArgs(n_new=n_new, channels=channels, n_texels_new=int(n_texels_new),
                                       n_texels=int(n_texels), new_dims=ptr(new_dims), src_off=ptr(src_off))
        chunk = list(zip(tensors, out))[i:i + _lib.SELECT_MAX_TENSORS]
        a.n_tensors = len(chunk)
        for k, (s, d) in enumerate(chunk):
            a.tensors[k] = _lib.GstexSelectPair(ptr(s), ptr(d))
        _lib.call("gstex_select_texels", ctypes.byref(a), _lib.stream_of(dev))
    return out


def select_texture(texture_dims, n_texels: int, keep, tensors, alloc=None):
    """Compact the texel store to the splats with keep[i]: -> (new_dims (n_new, 3) int32, new_tensors, n_texels_new).
    tensors: texel tensors (>= n_texels, ...) of 1 to 8 floats per texel sharing the charts, e.g. a parameter and its two
    Adam moments; each result has exactly n_texels_new rows.  alloc: as select_texels.  One read-back; ValueError on a
    malformed dims row (nothing is moved)."""
    plan = plan_selection(texture_dims, n_texels, keep)
    if plan.flagged:
        raise ValueError(_MALFORMED)
    new_dims, new_tensors = apply_selection(texture_dims.contiguous(), n_texels, plan, tensors, alloc)
    return new_dims, new_tensors, plan.n_texels_new


def apply_selection(texture_dims, n_texels: int, plan: SelectPlan, tensors, alloc=None):
    """The plan's dims and texel gather: -> (new_dims, new_tensors)."""
    new_dims, src_off = select_dims(texture_dims, plan)
    return new_dims, select_texels(new_dims, src_off, n_texels, plan.n_texels_new, tensors, alloc)


def select_rows(plan: SelectPlan, named: dict, alloc=None) -> dict:
    """The kept rows of per-splat tensors {name: (n, ...)} -> {name: (n_new, ...)}, in order, by gstex_density_apply with
    the plan's rows, row_off as offsets, every kind KEEP and role COPY (a kept row of an Adam moment is the source row
    too), one launch per GSTEX_DENSITY_MAX_TENSORS tensors; the split inputs are not needed and not passed.
    alloc(name, shape): where a result goes.  CPU tensors: index_select."""
    n, dev = plan.rows.shape[0], plan.rows.device
    if alloc is None:
        alloc = lambda name, s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    if not plan.rows.is_cuda:
        out = {}
        for name, t in select_rows_eager(plan.keep, named).items():
            out[name] = alloc(name, tuple(t.shape))
            out[name].copy_(t)
        return out
    kind = torch.zeros((n,), device=dev, dtype=torch.int32)  # GSTEX_DENSITY_KEEP
    out, descs = {}, []
    for name, t in named.items():
        src = t.detach()
        if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.shape[0] == n):
            raise ValueError(f"{name}: expected a contiguous HIP float32 tensor of {n} rows")
        shape = (plan.n_new,) + tuple(src.shape[1:])
        dst = alloc(name, shape)
        if not (dst.is_contiguous() and tuple(dst.shape) == shape and dst.dtype == torch.float32 and dst.device == dev):
            raise ValueError(f"{name}: the destination must be a contiguous float32 {shape} tensor on {dev}")
        out[name] = dst
        descs.append(_lib.GstexDensityTensor(ptr(src), ptr(dst), src.numel() // n if n else 0, ROLE_COPY))
    for i in range(0, len(descs), _lib.DENSITY_MAX_TENSORS):
        chunk = descs[i:i + _lib.DENSITY_MAX_TENSORS]
        arr = (_lib.GstexDensityTensor * len(chunk))(*chunk)
        a = _lib.GstexDensityApplyArgs(n=n, n_tensors=len(chunk), n_new=plan.n_new, log_split=0.0, rows=ptr(plan.rows),
                                       kind=ptr(kind), offsets=ptr(plan.row_off), tensors=arr)
        _lib.call("gstex_density_apply", ctypes.byref(a), _lib.stream_of(dev))
    return out
