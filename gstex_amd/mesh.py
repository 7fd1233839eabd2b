"""Mesh extraction: the training views' rendered depth fused into a truncated signed distance volume and the zero
surface extracted by marching tetrahedra, on the device (not in the reference, whose lineage leaves both to Open3D;
DESIGN.md "Mesh extraction").

* TSDFVolume            a dense (nz, ny, nx) volume on one device: integrate(views, renders), extract(), reset()
* tsdf_integrate / mesh_extract          the HIP entry points (gstex_amd/csrc/tsdf.hip)
* tsdf_integrate_eager / mesh_extract_eager   their eager torch twins, operation for operation, usable on CPU tensors:
                        every kernel operation is one correctly rounded fp32 + - * / in a fixed order, so kernel and twin
                        agree bit for bit, output order included
* MT_TABLE, MT_CORNERS, table_words      the marching-tetrahedra case table, derived by geometry at import; kernel and
                        twin read the same words
* largest_components    the lineage's floater removal on the host

Sample (i, j, k) of the volume sits at origin + voxel_size * (i, j, k) and has the linear index v = (k ny + j) nx + i.
One extraction: mark (which edges carry a vertex, how many faces each cell emits) -> the exclusive scans of the two
counts (the binning's scan) -> ONE read-back (the vertex and face totals) -> emit.
"""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import torch

from . import _lib
from ._lib import ptr

# the seven differences upper - lower corner of a tetrahedron edge, in the order that ranks an owner's vertices
EDGE_CLASSES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))


def _kuhn_corners():
    """The six Kuhn tetrahedra of the unit cube: for each permutation (a, b, c) of the axes the corners
    0, e_a, e_a + e_b, (1, 1, 1).  Every edge runs from a componentwise-lower to a higher corner."""
    tets = []
    for perm in itertools.permutations(range(3)):
        corner, corners = [0, 0, 0], [(0, 0, 0)]
        for axis in perm[:2]:
            corner[axis] = 1
            corners.append(tuple(corner))
        corners.append((1, 1, 1))
        tets.append(tuple(corners))
    return tuple(tets)


MT_CORNERS = _kuhn_corners()


def _case_table():
    """MT_TABLE[tet][case]: a tuple of triangles, each three edges (lower corner, upper corner) of the tetrahedron's
    corners 0..3; bit k of `case` says corner k is inside.  One inside or one outside corner: the triangle of the three
    edges at it.  Two inside corners a < b, outside c < d: the quad (a,c), (a,d), (b,d), (b,c) split along its first
    diagonal.  Each triangle is wound so that its normal (at the edge midpoints) points from the inside corners' centroid
    to the outside corners'."""
    table = []
    for corners in MT_CORNERS:
        P = np.asarray(corners, np.float64)
        row = []
        for case in range(16):
            ins = [k for k in range(4) if (case >> k) & 1]
            out = [k for k in range(4) if not (case >> k) & 1]
            if not ins or not out:
                row.append(())
                continue
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in out]]
            elif len(out) == 1:
                tris = [[(i, out[0]) for i in ins]]
            else:
                (a, b), (c, d) = ins, out
                quad = [(a, c), (a, d), (b, d), (b, c)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            outward = P[out].mean(0) - P[ins].mean(0)
            entry = []
            for tri in tris:
                mid = [0.5 * (P[p] + P[q]) for p, q in tri]
                if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), outward) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                entry.append(tuple((min(e), max(e)) for e in tri))
            row.append(tuple(entry))
        table.append(tuple(row))
    return tuple(table)


MT_TABLE = _case_table()


def table_words() -> np.ndarray:
    """The table as the int32[GSTEX_MESH_TABLE_WORDS] the kernels read (include/gstex_hip.h): word [tet * 16 + case] =
    triangle count << 24 | for slot s = 3 * triangle + index: lower corner << 4s | upper corner << (4s + 2); word
    [96 + tet] = for corner k: (dx | dy << 1 | dz << 2) << 3k."""
    words = np.zeros(_lib.MESH_TABLE_WORDS, np.int64)
    for t in range(6):
        for case in range(16):
            w = len(MT_TABLE[t][case]) << 24
            for s, (lo, hi) in enumerate(e for tri in MT_TABLE[t][case] for e in tri):
                w |= (lo | hi << 2) << (4 * s)
            words[t * 16 + case] = w
        words[96 + t] = sum((c[0] | c[1] << 1 | c[2] << 2) << (3 * k) for k, c in enumerate(MT_CORNERS[t]))
    return words.astype(np.int32)


_TABLE_CACHE: dict = {}


def _table_on(device) -> torch.Tensor:
    key = str(device)
    if key not in _TABLE_CACHE:
        _TABLE_CACHE[key] = torch.from_numpy(table_words()).to(device)
    return _TABLE_CACHE[key]


# ---------------------------------------------------------------------------------------- eager twins
def _s(v, like: torch.Tensor) -> torch.Tensor:
    """A python number as a 0-dim fp32 tensor (rounded once, as the C call rounds its float arguments).  Dividing by
    such a tensor is a true division on every device; by a python scalar torch's device kernels multiply by the rounded
    reciprocal (the care image_loss_eager takes)."""
    return torch.tensor(float(v), dtype=torch.float32, device=like.device)


def _positions(origin, voxel_size, dims, like):
    """(px, py, pz), each (nz, ny, nx): origin + voxel_size * index, one product and one sum."""
    nx, ny, nz = dims
    h = _s(voxel_size, like)
    ax = lambda o, n: _s(o, like) + h * torch.arange(n, device=like.device, dtype=torch.float32)  # noqa: E731
    x, y, z = ax(origin[0], nx), ax(origin[1], ny), ax(origin[2], nz)
    return (x[None, None, :].expand(nz, ny, nx), y[None, :, None].expand(nz, ny, nx),
            z[:, None, None].expand(nz, ny, nx))


def tsdf_integrate_eager(tsdf, weight, color, origin, voxel_size, views, renders, sdf_trunc, alpha_min=0.5,
                         depth_trunc=0.0, near_z=0.2):
    """gstex_tsdf_integrate restated: -> the new (tsdf, weight, color).  tsdf, weight: (nz, ny, nx); color: (3, nz, ny,
    nx) or None; views: objects with viewmat (3, 4), fx, fy, cx, cy, H, W; renders: per view a dict with depth (H, W)
    (un-normalised), alpha (H, W) and, with colour, rgb (H, W, 3).  Any number of views, in order (the kernel takes 8
    per launch, which changes nothing: a voxel's views are applied in view order either way)."""
    nz, ny, nx = tsdf.shape
    px, py, pz = _positions(origin, voxel_size, (nx, ny, nz), tsdf)
    tsdf, weight = tsdf.clone(), weight.clone()
    color = None if color is None else color.clone()
    trunc, amin, dtr, near = (_s(v, tsdf) for v in (sdf_trunc, alpha_min, depth_trunc, near_z))
    one = _s(1.0, tsdf)
    for view, r in zip(views, renders):
        st = _view_terms(view, r, px, py, pz, trunc, amin, dtr, near, float(depth_trunc) > 0)
        hit, t, pix = st["hit"], torch.minimum(one, st["s"] / trunc), st["pix"]
        w1 = weight + one
        tsdf = torch.where(hit, (tsdf * weight + t) / w1, tsdf)
        if color is not None:
            rgb = r["rgb"].detach().to(torch.float32).reshape(-1, 3)[pix]  # (nz, ny, nx, 3)
            color = torch.where(hit[None], (color * weight[None] + rgb.permute(3, 0, 1, 2)) / w1[None], color)
        weight = torch.where(hit, w1, weight)
    return tsdf, weight, color


def _view_terms(view, render, px, py, pz, trunc, amin, dtr, near, use_dtr):
    """One view's per-voxel decisions, in the kernel's order; each mask is the voxels that reached that test."""
    V = view.viewmat.detach().to(torch.float32).to(px.device)
    fx, fy, cx, cy = (_s(v, px) for v in (view.fx, view.fy, view.cx, view.cy))
    H, W = int(view.H), int(view.W)
    x = ((V[0, 0] * px + V[0, 1] * py) + V[0, 2] * pz) + V[0, 3]
    y = ((V[1, 0] * px + V[1, 1] * py) + V[1, 2] * pz) + V[1, 3]
    z = ((V[2, 0] * px + V[2, 1] * py) + V[2, 2] * pz) + V[2, 3]
    front = z > near
    u = fx * (x / z) + cx
    v = fy * (y / z) + cy
    inside = front & (u >= 0) & (u < _s(W, px)) & (v >= 0) & (v < _s(H, px))
    zero = torch.zeros_like(u)
    c = torch.where(inside, u, zero).to(torch.int64)
    r = torch.where(inside, v, zero).to(torch.int64)
    pix = r * W + c
    alpha = render["alpha"].detach().to(torch.float32).reshape(-1)[pix]
    opaque = inside & (alpha >= amin)
    d = render["depth"].detach().to(torch.float32).reshape(-1)[pix] / alpha
    ranged = opaque & (d > 0)
    if use_dtr:
        ranged = ranged & ~(d > dtr)
    s = d - z
    hit = ranged & ~(s < -trunc)
    return dict(z=z, u=u, v=v, front=front, inside=inside, opaque=opaque, ranged=ranged, hit=hit, s=s, pix=pix,
                d=d)


def classify_eager(origin, voxel_size, dims, view, render, sdf_trunc, alpha_min=0.5, depth_trunc=0.0, near_z=0.2):
    """The states one view puts the voxels of a grid in, from the twin's own decisions: a dict of (nz, ny, nx) bool
    masks -- behind (z <= 0), near (0 < z <= near_z), left / right / above / below (projecting outside that image
    border), faint (alpha < alpha_min), far (beyond depth_trunc), occluded (behind the surface by more than sdf_trunc),
    ramp (t < 1) and clamped (t == 1)."""
    like = render["alpha"].detach().to(torch.float32)
    px, py, pz = _positions(origin, voxel_size, dims, like)
    trunc, amin, dtr, near = (_s(v, like) for v in (sdf_trunc, alpha_min, depth_trunc, near_z))
    st = _view_terms(view, render, px, py, pz, trunc, amin, dtr, near, float(depth_trunc) > 0)
    f, t = st["front"], st["s"] / trunc
    return dict(behind=st["z"] <= 0, near=(st["z"] > 0) & ~f, left=f & (st["u"] < 0),
                right=f & (st["u"] >= float(view.W)), above=f & (st["v"] < 0), below=f & (st["v"] >= float(view.H)),
                faint=st["inside"] & ~st["opaque"], far=st["opaque"] & (st["d"] > 0) & ~st["ranged"],
                occluded=st["ranged"] & ~st["hit"], ramp=st["hit"] & (t < 1), clamped=st["hit"] & ~(t < 1))


def _table_tensors(device):
    """(ntri (6, 16), lo (6, 16, 6), hi (6, 16, 6), corner bits (6, 4)) decoded from table_words()."""
    w = torch.from_numpy(table_words().astype(np.int64)).to(device)
    cases = w[:96].reshape(6, 16)
    slots = torch.arange(6, device=device)
    lo = (cases[..., None] >> (4 * slots)) & 3
    hi = (cases[..., None] >> (4 * slots + 2)) & 3
    corners = (w[96:, None] >> (3 * torch.arange(4, device=device))) & 7
    return (cases >> 24) & 3, lo, hi, corners


_CLASS_OF_DIFF = (0, 0, 1, 3, 2, 5, 4, 6)  # dx | dy << 1 | dz << 2 -> the index in EDGE_CLASSES


def mesh_extract_eager(tsdf, weight, color, origin, voxel_size):
    """gstex_mesh_extract_mark / _emit and the scans restated: -> (vertices (V, 3) f32, colors (V, 3) f32 or None,
    faces (F, 3) int32), in the kernels' order: vertices ascending in 7 * v(owner) + class, faces in (cell,
    tetrahedron, triangle)."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    ntri_t, lo_t, hi_t, corners_t = _table_tensors(dev)
    class_of = torch.tensor(_CLASS_OF_DIFF, device=dev)
    flat_t, flat_w = tsdf.reshape(-1), weight.reshape(-1)
    k, j, i = torch.meshgrid(torch.arange(nz - 1, device=dev), torch.arange(ny - 1, device=dev),
                             torch.arange(nx - 1, device=dev), indexing="ij")
    cell = ((k * ny + j) * nx + i).reshape(-1)  # ascending: the cells in their linear order
    step = lambda bits: (bits & 1) + ((bits >> 1) & 1) * nx + ((bits >> 2) & 1) * nx * ny  # noqa: E731
    keys, counts = [], []
    for t in range(6):
        vox = cell[:, None] + step(corners_t[t])[None, :]  # (cells, 4)
        ok = (flat_w[vox] > 0).all(dim=1)
        case = ((flat_t[vox] < 0).long() << torch.arange(4, device=dev)).sum(dim=1)
        case = torch.where(ok, case, torch.zeros_like(case))
        lo, hi = lo_t[t][case], hi_t[t][case]  # (cells, 6)
        blo, bhi = corners_t[t][lo], corners_t[t][hi]
        owner = cell[:, None] + step(blo)
        keys.append(7 * owner + class_of[bhi - blo])
        counts.append(ntri_t[t][case])
    key = torch.stack(keys, 1).reshape(-1, 6, 2, 3)  # (cells, tet, triangle, index)
    ntri = torch.stack(counts, 1)  # (cells, tet)
    emitted = torch.arange(2, device=dev)[None, None, :] < ntri[..., None]
    face_keys = key[emitted]  # (F, 3), in (cell, tet, triangle) order
    vkeys = torch.unique(face_keys)  # sorted
    faces = torch.searchsorted(vkeys, face_keys.reshape(-1)).reshape(-1, 3).to(torch.int32)
    a = vkeys // 7
    diff = torch.tensor([c[0] | c[1] << 1 | c[2] << 2 for c in EDGE_CLASSES], device=dev)[vkeys % 7]
    b = a + step(diff)
    ta, tb = flat_t[a], flat_t[b]
    t = ta / (ta - tb)
    ai = torch.stack([a % nx, (a // nx) % ny, a // (nx * ny)], 1)
    bi = ai + torch.stack([diff & 1, (diff >> 1) & 1, (diff >> 2) & 1], 1)
    o = torch.stack([_s(v, tsdf) for v in origin])
    h = _s(voxel_size, tsdf)
    pa, pb = o[None] + h * ai.float(), o[None] + h * bi.float()
    vertices = pa + t[:, None] * (pb - pa)
    colors = None
    if color is not None:
        c = color.reshape(3, -1)
        ca, cb = c[:, a].t(), c[:, b].t()
        colors = (ca + t[:, None] * (cb - ca)).contiguous()
    return vertices.contiguous(), colors, faces.contiguous()


# ---------------------------------------------------------------------------------------- host utilities
def largest_components(faces, n_vertices: int, keep: int):
    """The lineage's floater removal: keep the `keep` connected components with the most faces (ties: the one holding
    the lowest vertex first) and re-index.  -> (faces (F', 3) with the new indices, kept (V',) the old index of each new
    vertex, ascending).  numpy only."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    n = int(n_vertices)
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError(f"largest_components: a face index is outside [0, {n})")
    if int(keep) <= 0:
        raise ValueError(f"keep must be > 0 (got {keep})")
    label = np.arange(n, dtype=np.int64)
    ends = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]) if f.size else np.zeros((0, 2), np.int64)
    while True:  # min-label propagation along the edges with pointer jumping
        low = np.minimum(label[ends[:, 0]], label[ends[:, 1]])
        new = label.copy()
        np.minimum.at(new, ends[:, 0], low)
        np.minimum.at(new, ends[:, 1], low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    face_label = label[f[:, 0]] if f.size else np.zeros(0, np.int64)
    roots, sizes = np.unique(face_label, return_counts=True)
    order = np.lexsort((roots, -sizes))[: int(keep)]
    keep_face = np.isin(face_label, roots[order])
    f = f[keep_face]
    kept = np.unique(f)
    remap = np.full(n, -1, np.int64)
    remap[kept] = np.arange(kept.shape[0])
    return remap[f].astype(np.int32).reshape(-1, 3), kept


# ---------------------------------------------------------------------------------------- HIP entry points
def _dev_f32(t, name, shape):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)
            and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous HIP float32 tensor of shape {tuple(shape)}")
    return t


def _volume_struct(tsdf, weight, color, origin, voxel_size):
    nz, ny, nx = tsdf.shape
    _dev_f32(tsdf, "tsdf", (nz, ny, nx))
    _dev_f32(weight, "weight", (nz, ny, nx))
    if color is not None:
        _dev_f32(color, "color", (3, nz, ny, nx))
    return _lib.GstexTsdfVolume(nx, ny, nz, (ctypes.c_float * 3)(*[float(v) for v in origin]), float(voxel_size),
                                ptr(tsdf), ptr(weight), ptr(color))


def tsdf_integrate(tsdf, weight, color, origin, voxel_size, views, renders, sdf_trunc, alpha_min=0.5, depth_trunc=0.0,
                   near_z=0.2) -> None:
    """gstex_tsdf_integrate: 1..8 views fused into the volume in place, one launch, no read-back."""
    vol = _volume_struct(tsdf, weight, color, origin, voxel_size)
    if len(views) != len(renders):
        raise ValueError(f"{len(views)} views but {len(renders)} renders")
    keep, entries = [], []
    for q, (view, r) in enumerate(zip(views, renders)):
        H, W = int(view.H), int(view.W)
        vm = view.viewmat.detach()
        vm = vm if (vm.dtype == torch.float32 and vm.is_contiguous() and vm.device == tsdf.device) else \
            vm.to(tsdf.device, torch.float32).contiguous()
        depth = _dev_f32(r["depth"].detach(), f"renders[{q}]['depth']", (H, W))
        alpha = _dev_f32(r["alpha"].detach(), f"renders[{q}]['alpha']", (H, W))
        rgb = _dev_f32(r["rgb"].detach(), f"renders[{q}]['rgb']", (H, W, 3)) if color is not None else None
        keep.append((vm, depth, alpha, rgb))
        cam = _lib.make_camera(vm, None, view.fx, view.fy, view.cx, view.cy, H, W, 16)
        entries.append(_lib.GstexTsdfView(cam, ptr(depth), ptr(alpha), ptr(rgb)))
    arr = (_lib.GstexTsdfView * max(len(entries), 1))(*entries)
    a = _lib.GstexTsdfIntegrateArgs(vol=vol, n_views=len(entries), sdf_trunc=float(sdf_trunc),
                                    alpha_min=float(alpha_min), depth_trunc=float(depth_trunc), near_z=float(near_z),
                                    views=arr)
    _lib.call("gstex_tsdf_integrate", ctypes.byref(a), _lib.stream_of(tsdf.device))
    del keep


class MeshPlan:
    """What mesh_extract_mark leaves for mesh_extract_emit: the totals and the work arrays."""

    def __init__(self, args, keep, n_vertices: int, n_faces: int, has_color: bool, device):
        self.args, self.keep, self.n_vertices, self.n_faces = args, keep, n_vertices, n_faces
        self.has_color, self.device = has_color, device


def mesh_extract_mark(tsdf, weight, color, origin, voxel_size) -> MeshPlan:
    """gstex_mesh_extract_mark, the two scans (the binning's) and the extraction's ONE read-back: the vertex and face
    totals together."""
    from .ops import _scan_offsets

    dev = tsdf.device
    vol = _volume_struct(tsdf, weight, color, origin, voxel_size)
    n_vox = tsdf.numel()
    mask, vcount, fcount = (torch.empty((n_vox,), device=dev, dtype=torch.int32) for _ in range(3))
    table = _table_on(dev)
    a = _lib.GstexMeshExtractArgs(vol=vol, table=ptr(table), edge_mask=ptr(mask), vertex_count=ptr(vcount),
                                  face_count=ptr(fcount))
    _lib.call("gstex_mesh_extract_mark", ctypes.byref(a), _lib.stream_of(dev))
    voff, foff = _scan_offsets(vcount), _scan_offsets(fcount)
    nv, nf = (int(x) for x in torch.stack([voff[n_vox], foff[n_vox]]).cpu().tolist())
    a.vertex_offsets, a.face_offsets, a.n_vertices, a.n_faces = ptr(voff), ptr(foff), nv, nf
    return MeshPlan(a, (tsdf, weight, color, table, mask, vcount, fcount, voff, foff), nv, nf, color is not None, dev)


def mesh_extract_emit(plan: MeshPlan, vertices, colors, faces) -> None:
    """gstex_mesh_extract_emit into caller-sized buffers: vertices / colors of at least n_vertices rows, faces of at
    least n_faces rows; the kernels are told the plan's totals and write nothing past them."""
    _dev_f32(vertices, "vertices", (vertices.shape[0], 3))
    if colors is not None:
        _dev_f32(colors, "colors", (colors.shape[0], 3))
    if not (faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
            and faces.is_contiguous()):
        raise ValueError("faces: expected a contiguous HIP int32 tensor of shape (F, 3)")
    if vertices.shape[0] < plan.n_vertices or faces.shape[0] < plan.n_faces or \
            (colors is not None and colors.shape[0] < plan.n_vertices):
        raise ValueError(f"the outputs hold fewer rows than the plan's {plan.n_vertices} vertices and {plan.n_faces} "
                         "faces")
    if colors is not None and not plan.has_color:
        raise ValueError("colors need a colour volume")
    a = plan.args
    a.vertices, a.colors, a.faces = vertices.data_ptr(), None if colors is None else colors.data_ptr(), faces.data_ptr()
    _lib.call("gstex_mesh_extract_emit", ctypes.byref(a), _lib.stream_of(plan.device))


def mesh_extract(tsdf, weight, color, origin, voxel_size):
    """Mark, scan, read back, emit: -> (vertices (V, 3), colors (V, 3) or None, faces (F, 3) int32) on the device."""
    plan = mesh_extract_mark(tsdf, weight, color, origin, voxel_size)
    dev = tsdf.device
    vertices = torch.empty((plan.n_vertices, 3), device=dev, dtype=torch.float32)
    colors = torch.empty((plan.n_vertices, 3), device=dev, dtype=torch.float32) if color is not None else None
    faces = torch.empty((plan.n_faces, 3), device=dev, dtype=torch.int32)
    mesh_extract_emit(plan, vertices, colors, faces)
    return vertices, colors, faces


class TSDFVolume:
    """A dense truncated signed distance volume on one device (HIP: the kernels; CPU: the eager twins).  dims: (nx, ny,
    nz); arrays are (nz, ny, nx), x fastest.  Memory: 8 bytes per voxel, 20 with colour; an extraction adds 20 bytes
    per voxel of work arrays while it runs."""

    def __init__(self, device, origin, voxel_size: float, dims, sdf_trunc: float, color: bool = True):
        self.device = torch.device(device)
        self.origin = tuple(float(np.float32(v)) for v in origin)
        self.voxel_size = float(np.float32(voxel_size))
        self.dims = tuple(int(v) for v in dims)
        self.sdf_trunc = float(np.float32(sdf_trunc))
        if len(self.origin) != 3 or len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f"dims must be three sizes >= 2 (got {dims})")
        if 7 * self.dims[0] * self.dims[1] * self.dims[2] >= 1 << 31:
            raise ValueError(f"7 * n_vox must be below 2^31 (got dims {self.dims})")
        if not (self.voxel_size > 0 and self.sdf_trunc > 0):
            raise ValueError("voxel_size and sdf_trunc must be > 0")
        nx, ny, nz = self.dims
        self.tsdf = torch.zeros((nz, ny, nx), device=self.device, dtype=torch.float32)
        self.weight = torch.zeros_like(self.tsdf)
        self.color = torch.zeros((3, nz, ny, nx), device=self.device, dtype=torch.float32) if color else None

    def reset(self) -> None:
        self.tsdf.zero_()
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def integrate(self, views, renders, alpha_min: float = 0.5, depth_trunc: float = 0.0, near_z: float = 0.2) -> None:
        """Fuse the views' renders (dicts with depth, alpha and, with colour, rgb) into the volume, 8 views per launch."""
        views, renders = list(views), list(renders)
        if len(views) != len(renders):
            raise ValueError(f"{len(views)} views but {len(renders)} renders")
        if self.device.type != "cuda":
            self.tsdf, self.weight, self.color = tsdf_integrate_eager(
                self.tsdf, self.weight, self.color, self.origin, self.voxel_size, views, renders, self.sdf_trunc,
                alpha_min, depth_trunc, near_z)
            return
        for i in range(0, len(views), _lib.TSDF_MAX_VIEWS):
            tsdf_integrate(self.tsdf, self.weight, self.color, self.origin, self.voxel_size,
                           views[i:i + _lib.TSDF_MAX_VIEWS], renders[i:i + _lib.TSDF_MAX_VIEWS], self.sdf_trunc,
                           alpha_min, depth_trunc, near_z)

    def extract(self):
        """-> (vertices (V, 3) f32, colors (V, 3) f32 or None, faces (F, 3) int32)."""
        fn = mesh_extract if self.device.type == "cuda" else mesh_extract_eager
        return fn(self.tsdf, self.weight, self.color, self.origin, self.voxel_size)


def mesh_grid(lo, hi, voxel_size=None, mesh_res: int = 256, sdf_trunc=None):
    """The grid GStexTrainer.extract_mesh integrates into: -> (origin, voxel_size h, dims, sdf_trunc, (lo', hi') the
    padded bounds).  The box [lo, hi] is padded on every side by sdf_trunc + h, and by default h is the longest PADDED
    side over mesh_res, so with L the longest side of the box the two are solved together:

        sdf_trunc = 5 h (default):  h = (L + 12 h) / mesh_res  =>  h = L / (mesh_res - 12)
        sdf_trunc given:            h = (L + 2 sdf_trunc + 2 h) / mesh_res  =>  h = (L + 2 sdf_trunc) / (mesh_res - 2)

    dims = ceil(padded side / h) + 1 samples per axis, origin = lo'."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    L = float((hi - lo).max())
    if voxel_size is None:
        if sdf_trunc is None:
            if mesh_res <= 12:
                raise ValueError(f"mesh_res must be > 12 (got {mesh_res})")
            voxel_size = L / (mesh_res - 12)
        else:
            if mesh_res <= 2:
                raise ValueError(f"mesh_res must be > 2 (got {mesh_res})")
            voxel_size = (L + 2 * float(sdf_trunc)) / (mesh_res - 2)
    h = float(voxel_size)
    if not h > 0:
        raise ValueError("the bounds are empty: give voxel_size")
    trunc = 5.0 * h if sdf_trunc is None else float(sdf_trunc)
    pad = trunc + h
    lo_p, hi_p = lo - pad, hi + pad
    dims = tuple(max(2, int(np.ceil((hi_p[c] - lo_p[c]) / h - 1e-9)) + 1) for c in range(3))
    return tuple(float(v) for v in lo_p), h, dims, trunc, (lo_p, hi_p)


# ---------------------------------------------------------------------------------------- scoring
def sample_mesh(vertices, faces, spacing):
    """gstex_amd.neighbors.sample_mesh: the deterministic area sampler, -> (samples, weights, face_of)."""
    from .neighbors import sample_mesh as _sample

    return _sample(vertices, faces, spacing)


def _crop(points, bounds):
    lo = torch.as_tensor(bounds[0], dtype=torch.float32, device=points.device)
    hi = torch.as_tensor(bounds[1], dtype=torch.float32, device=points.device)
    return ((points >= lo[None]) & (points <= hi[None])).all(dim=1)


def score_mesh(vertices, faces, reference, *, spacing, max_dist=None, thresholds=(), bounds=None) -> dict:
    """A mesh against a reference point cloud, by the DTU protocol's measures, on the mesh's device (HIP: the kernels
    of gstex_amd.neighbors; CPU: their twins).  The surface is sampled at `spacing` (sample_mesh); d_i is the distance
    from sample i (area weight w_i) to its nearest reference point and e_j that from reference point j to its nearest
    sample, both clamped at max_dist when given:

        accuracy      sum w_i d_i / sum w_i          completeness   mean_j e_j         chamfer   their mean
        precision[t]  sum w_i [d_i <= t] / sum w_i   recall[t]      mean_j [e_j <= t]  fscore[t] 2 P R / (P + R), 0 at 0/0

    precision, recall and fscore are lists aligned with `thresholds`.  bounds = (lo, hi) crops samples and reference
    points to the box first (the protocol's observation box).  The dict also holds d (S,), e (R,) (f32, on the
    device), samples, weights, n_samples and n_reference.  The kernels return squared distances; the (correctly rounded) roots,
    the clamps and the float64 sums are torch ops."""
    from .neighbors import PointGrid, sqrt_rn

    vertices = vertices.detach().to(torch.float32)
    reference = reference.detach().to(device=vertices.device, dtype=torch.float32)
    if reference.dim() != 2 or reference.shape[1] != 3:
        raise ValueError("reference: expected an (R, 3) tensor")
    samples, weights, _ = sample_mesh(vertices, faces, spacing)
    if bounds is not None:
        keep = _crop(samples, bounds)
        samples, weights = samples[keep].contiguous(), weights[keep].contiguous()
        reference = reference[_crop(reference, bounds)]
    reference = reference.contiguous()
    if samples.shape[0] == 0 or reference.shape[0] == 0:
        raise ValueError(f"score_mesh: nothing to compare ({samples.shape[0]} samples, {reference.shape[0]} reference "
                         "points)")
    d = sqrt_rn(PointGrid(reference).query(samples, k=1)[0][:, 0])
    e = sqrt_rn(PointGrid(samples).query(reference, k=1)[0][:, 0])
    if max_dist is not None:
        d, e = d.clamp(max=float(max_dist)), e.clamp(max=float(max_dist))
    w = weights.double()
    w_sum = w.sum()
    accuracy = float((w * d.double()).sum() / w_sum)
    completeness = float(e.double().mean())
    out = dict(accuracy=accuracy, completeness=completeness, chamfer=0.5 * (accuracy + completeness),
               thresholds=tuple(float(t) for t in thresholds), precision=[], recall=[], fscore=[], d=d, e=e,
               samples=samples, weights=weights, n_samples=int(samples.shape[0]), n_reference=int(reference.shape[0]))
    for t in out["thresholds"]:
        p = float((w * (d <= t).double()).sum() / w_sum)
        r = float((e <= t).double().mean())
        out["precision"].append(p)
        out["recall"].append(r)
        out["fscore"].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out
