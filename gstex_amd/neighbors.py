"""Nearest neighbours on a uniform grid and a deterministic mesh surface sampler, on the device (not in the reference;
DESIGN.md "Mesh scoring and nearest neighbours").

* PointGrid             a uniform-grid index over a 3D point set on one device (HIP: the kernels of
                        gstex_amd/csrc/neighbors.hip; CPU: the eager twins): query(queries, k, exclude_self, max_radius)
* grid_build / nn_query / sample_mesh_mark / sample_mesh_emit      the HIP entry points
* grid_build_eager / nn_query_eager / sample_mesh_eager            their eager torch twins, usable on CPU tensors: every
                        kernel operation is one correctly rounded fp32 operation in a fixed order, so kernel and twin
                        agree bit for bit on every output the contract orders (a cell's records are a set: the order
                        inside a cell is an atomic cursor's)
* walk_rings_eager / nn_query_walk_eager    the kernels' ring walk on the host, stated once (it also serves
                        cluster.dbscan_walk_eager), and gstex_nn_query's kernel restated through it (tests, small sets)
* sample_mesh           (samples, weights, face_of) of a triangle mesh on the mesh's device
* knn_mean_dist_device  the initialisation's per-point scale, the mean distance to the k nearest other points

The cell of p is, per axis, (int)((p - origin) / cell_size) clamped to [0, n_axis - 1], origin the component-wise minimum
of the points, and the linear cell index is (cz ny + cy) nx + cx.  One build: the bounds (the build's ONE read-back, they
size the cell array) -> count -> the exclusive scan (the binning's) -> place.  A query reads nothing back.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr


def _s(v, like: torch.Tensor) -> torch.Tensor:
    """A python number as a 0-dim fp32 tensor (rounded once, as the C call rounds its float arguments); dividing by it
    is a true division on every device."""
    return torch.tensor(float(v), dtype=torch.float32, device=like.device)


def _f32(v) -> float:
    return float(np.float32(v))


def sqrt_rn(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root, as the kernels' sqrtf is.  torch.sqrt on CPU float32 tensors is not
    (its vector library is off by an ulp on about 0.6 % of random inputs), numpy's is; elsewhere the float64 root
    rounded once, which is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits)."""
    if x.device.type == "cpu":
        return torch.from_numpy(np.sqrt(x.detach().contiguous().numpy()))
    return torch.sqrt(x.double()).to(torch.float32)


# ---------------------------------------------------------------------------------------- the grid's shape
def grid_dims(lo, hi, cell_size):
    """n_axis = (int)((hi - lo) / cell_size) + 1, by the cell assignment's own two fp32 operations: the point at the
    maximum lands in the last cell and no point is clamped."""
    lo, hi, h = np.asarray(lo, np.float32), np.asarray(hi, np.float32), np.float32(cell_size)
    return tuple(int(np.float32(np.float32(hi[c] - lo[c]) / h)) + 1 for c in range(3))


def _fits(dims) -> bool:
    return max(dims) <= _lib.NN_MAX_AXIS_CELLS and dims[0] * dims[1] * dims[2] <= _lib.NN_MAX_CELLS


def default_cell_size(n: int, lo, hi) -> float:
    """The default cell: the geometric mean of the spacing of n points filling the bounding box, (V / n)^(1/3), and of n
    points on a surface the size of the box's, sqrt(A / n) with A the box's area -- within a factor of two of the
    points' spacing in both cases, the sets this project indexes (splat centres, mesh samples, scans) being one or the
    other.  Each extent counts as at least 1/1024 of the longest (a flat cloud has no volume).  Enlarged by a quarter
    at a time until the grid fits the cell limits.  Correctness does not depend on it."""
    ext = np.maximum(np.asarray(hi, np.float64) - np.asarray(lo, np.float64), 0.0)
    longest = float(ext.max())
    if not longest > 0 or n < 2:
        return 1.0
    e = np.maximum(ext, longest / 1024.0)
    volume = float(e[0] * e[1] * e[2])
    area = 2.0 * float(e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    h = math.sqrt((volume / n) ** (1.0 / 3.0) * math.sqrt(area / n))
    h = max(h, longest * 2.0 ** -20)
    while not _fits(grid_dims(lo, hi, _f32(h))):
        h *= 1.25
    return _f32(h)


# ---------------------------------------------------------------------------------------- eager twins
def _cells_eager(points, origin, cell_size, dims):
    """(int)((p - origin) / cell_size) per axis, clamped, NaN -> 0 as the kernel's fmaxf gives: -> (n, 3) int64."""
    o = torch.stack([_s(v, points) for v in origin])
    t = (points - o[None]) / _s(cell_size, points)
    top = torch.tensor([d - 1 for d in dims], dtype=torch.float32, device=points.device)
    return torch.minimum(torch.where(t > 0, t, torch.zeros_like(t)), top[None]).to(torch.int64)


def grid_build_eager(points, origin, cell_size, dims):
    """gstex_nn_grid_count / _place and the scan restated: -> (cell_start (n_cells + 1) int32, records (n, 4) f32 with
    the index's bits in column 3).  Inside a cell the records are in index order here; the kernel's order is free."""
    n = points.shape[0]
    nx, ny, nz = dims
    c = _cells_eager(points, origin, cell_size, dims)
    cell = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    count = torch.bincount(cell, minlength=nx * ny * nz)
    cell_start = torch.zeros(nx * ny * nz + 1, dtype=torch.int64, device=points.device)
    cell_start[1:] = torch.cumsum(count, 0)
    order = torch.sort(cell, stable=True).indices
    records = torch.empty((n, 4), dtype=torch.float32, device=points.device)
    records[:, :3] = points[order]
    records[:, 3] = order.to(torch.int32).view(torch.float32)
    return cell_start.to(torch.int32), records


def nn_query_eager(points, queries, k: int = 1, exclude_self: bool = False, max_radius=None, chunk: int = 1024):
    """gstex_nn_query's result restated as the exact brute force in the kernel's operation order and tie rule:
    d2 = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x in fp32, ascending, ties to the lower index, the point whose index
    equals the query's row skipped under exclude_self, points with d2 > max_radius * max_radius (one fp32 product)
    not counted, missing neighbours d2 = +inf and index = -1.  -> (d2 (Q, k) f32, index (Q, k) int32)."""
    points, queries = points.to(torch.float32), queries.to(torch.float32)
    n, nq = points.shape[0], queries.shape[0]
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=points.device)
    r2 = inf if max_radius is None else _s(max_radius, points) * _s(max_radius, points)
    out_d = torch.full((nq, k), float("inf"), dtype=torch.float32, device=points.device)
    out_i = torch.full((nq, k), -1, dtype=torch.int32, device=points.device)
    if n == 0:
        return out_d, out_i
    for a in range(0, nq, chunk):
        q = queries[a:a + chunk]
        dx = q[:, None, 0] - points[None, :, 0]
        dy = q[:, None, 1] - points[None, :, 1]
        dz = q[:, None, 2] - points[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        d = torch.where(d <= r2, d, inf)  # (NaN does not count either)
        if exclude_self:
            rows = torch.arange(a, a + q.shape[0], device=points.device)
            ok = rows < n
            d[torch.nonzero(ok)[:, 0], rows[ok]] = inf
        sd, si = torch.sort(d, dim=1, stable=True)  # stable: equal d2 stay in index order
        m = min(k, n)
        sd, si = sd[:, :m], si[:, :m].to(torch.int32)
        out_d[a:a + chunk, :m] = sd
        out_i[a:a + chunk, :m] = torch.where(torch.isinf(sd), torch.full_like(si, -1), si)
    return out_d, out_i


def query_cell_eager(q, origin, cell_size):
    """The unclamped cell of q (3 fp32 numbers) as the kernels' query_cell_axis gives it: per axis floor((q - o) / h)
    in fp32, kept within +-2^29, NaN -> -2^29.  -> (cx, cy, cz) python ints."""
    f, limit = np.float32, 2 ** 29
    with np.errstate(all="ignore"):
        t = [np.floor(f(f(q[c]) - f(origin[c])) / f(cell_size)) for c in range(3)]
    return tuple(-limit if v != v else int(min(max(v, -limit), limit)) for v in t)


def walk_rings_eager(q, origin, cell_size, dims, cell_start, scan, bound):
    """nn_grid.h's walk_rings on the host, the one ring walk of every host twin: the Chebyshev rings of cells around
    q's unclamped cell, from the first that meets the grid to the last, scan(a, b) for each contiguous run of records
    cell_start[c] .. cell_start[c'] of a ring's cells (a whole row x0..x1 on a face of the ring; through its inside the
    two end cells cx - r and cx + r where they are in the grid; ring 0: one cell, not twice), and after every ring
    r >= 1 the stop test ((float)r * h) * (1 - 2^-10), squared, >= bound(), the fp32 squared radius still of
    interest.  Every fp32 value is one individually rounded operation, as in the kernel."""
    f = np.float32
    nx, ny, nz = (int(d) for d in dims)
    h, margin = f(cell_size), f(1.0 - 2.0 ** -10)
    cx, cy, cz = query_cell_eager(q, origin, cell_size)
    r_first = max(-cx, cx - (nx - 1), -cy, cy - (ny - 1), -cz, cz - (nz - 1), 0)
    r_last = max(cx, nx - 1 - cx, cy, ny - 1 - cy, cz, nz - 1 - cz)
    for r in range(r_first, r_last + 1):
        x0, x1 = max(cx - r, 0), min(cx + r, nx - 1)
        ends = [x for x in ((cx - r, cx + r) if r > 0 else (cx,)) if 0 <= x < nx]
        for z in range(max(cz - r, 0), min(cz + r, nz - 1) + 1):
            for y in range(max(cy - r, 0), min(cy + r, ny - 1) + 1):
                base = (z * ny + y) * nx
                if abs(z - cz) == r or abs(y - cy) == r:
                    if x0 <= x1:
                        scan(cell_start[base + x0], cell_start[base + x1 + 1])
                else:
                    for x in ends:
                        scan(cell_start[base + x], cell_start[base + x + 1])
        if r >= 1:
            lb = f(f(r) * h) * margin
            if lb * lb >= bound():
                break


def nn_query_walk_eager(origin, cell_size, dims, cell_start, records, queries, k: int = 1, exclude_self: bool = False,
                        max_radius=None):
    """gstex_nn_query's kernel restated on the host, one python loop per query (for tests and small sets):
    walk_rings_eager carrying the top-k under (d2, index), stopped on min(k-th best, max_radius^2).  -> (d2 (Q, k) f32,
    index (Q, k) int32), which must equal nn_query_eager's."""
    f = np.float32
    rec = records.detach().cpu().numpy()
    pts, idx = rec[:, :3], np.ascontiguousarray(rec[:, 3]).view(np.int32)
    cs = cell_start.detach().cpu().numpy().astype(np.int64)
    qs = queries.detach().cpu().to(torch.float32).numpy()
    r2max = f(np.inf) if max_radius is None else f(max_radius) * f(max_radius)
    out_d = np.full((qs.shape[0], k), np.inf, np.float32)
    out_i = np.full((qs.shape[0], k), -1, np.int32)
    for row, q in enumerate(qs):
        best = []  # (d2, index), ascending

        def scan(a, b):
            nonlocal best
            if b <= a:
                return
            d = q[None, :] - pts[a:b]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            for dv, iv in zip(d2, idx[a:b]):
                if (exclude_self and iv == row) or not dv <= r2max:
                    continue
                best = sorted(best + [(dv, int(iv))])[:k]

        walk_rings_eager(q, origin, cell_size, dims, cs, scan,
                         lambda: min(best[k - 1][0] if len(best) == k else f(np.inf), r2max))
        for s, (dv, iv) in enumerate(best):
            out_d[row, s], out_i[row, s] = dv, iv
    return torch.from_numpy(out_d), torch.from_numpy(out_i)


def _isqrt_ceil(x: torch.Tensor) -> torch.Tensor:
    m = torch.sqrt(x.double()).to(torch.int64)
    m = torch.where(m * m < x, m + 1, m)
    return torch.where((m - 1) * (m - 1) >= x, m - 1, m)


def _face_counts_eager(vertices, faces, spacing):
    """n per face: (n (F,) int64, pa, e1, e2).  L = sqrt(max of the three squared edge lengths), n = max(1, ceil(L /
    spacing))."""
    f = faces.to(torch.int64)
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= vertices.shape[0]):
        raise ValueError(f"sample_mesh: a face index is outside [0, {vertices.shape[0]})")
    pa, pb, pc = vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]]
    e1, e2, e3 = pb - pa, pc - pa, pc - pb
    len2 = lambda e: (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]  # noqa: E731
    L = sqrt_rn(torch.maximum(torch.maximum(len2(e1), len2(e2)), len2(e3)))
    q = torch.ceil(L / _s(spacing, vertices))
    n = torch.where(q < 2.0 ** 30, q.clamp(min=1.0), torch.full_like(q, 2.0 ** 30)).to(torch.int64)
    return n, pa, e1, e2


def _check_sample_totals(total: int, n_max: int, bad: int, n_vertices: int) -> None:
    if bad:
        raise ValueError(f"sample_mesh: {bad} faces have an index outside [0, {n_vertices})")
    if n_max > _lib.SAMPLE_MAX_N:
        raise ValueError(f"sample_mesh: a face needs n = {n_max} subdivisions (longest edge / spacing), more than "
                         f"{_lib.SAMPLE_MAX_N}: the spacing is too fine for this mesh")
    if total >= 1 << 31:
        raise ValueError(f"sample_mesh: {total} samples, not below 2^31: the spacing is too fine for this mesh")


def sample_mesh_eager(vertices, faces, spacing):
    """gstex_mesh_sample_mark / _emit and the scan restated, order included: -> (samples (S, 3) f32, weights (S,) f32,
    face_of (S,) int32)."""
    if not float(spacing) > 0:
        raise ValueError(f"spacing must be > 0 (got {spacing})")
    vertices = vertices.to(torch.float32)
    dev = vertices.device
    n, pa, e1, e2 = _face_counts_eager(vertices, faces, spacing)
    F = n.shape[0]
    _check_sample_totals(int((n * n)[n <= _lib.SAMPLE_MAX_N].sum()) if F else 0, int(n.max()) if F else 0, 0,
                         vertices.shape[0])
    nn = n * n
    offsets = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(nn, 0)
    face_of = torch.repeat_interleave(torch.arange(F, device=dev), nn)
    t = torch.arange(int(offsets[F]), device=dev) - offsets[face_of]
    nf = n[face_of]
    i = nf - _isqrt_ceil(nf * nf - t)  # row i starts at i (2 n - i)
    tt = t - i * (2 * nf - i)
    j = tt >> 1
    one, two, three = (torch.tensor(v, dtype=torch.float32, device=dev) for v in (1.0, 2.0, 3.0))
    third = torch.where((tt & 1) == 1, two / three, one / three)
    fn = nf.to(torch.float32)
    u, v = (i.to(torch.float32) + third) / fn, (j.to(torch.float32) + third) / fn
    a, b, c = pa[face_of], e1[face_of], e2[face_of]
    samples = (a + u[:, None] * b) + v[:, None] * c
    cr = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    area = torch.tensor(0.5, dtype=torch.float32, device=dev) * sqrt_rn(
        (cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    weights = area[face_of] / (fn * fn)
    return samples.contiguous(), weights.contiguous(), face_of.to(torch.int32)


# ---------------------------------------------------------------------------------------- HIP entry points
def _dev(t, name, dtype, cols):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == cols
            and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous HIP {dtype} tensor of shape (n, {cols})")
    return t


def _grid_struct(origin, cell_size, dims):
    return _lib.GstexNnGrid((ctypes.c_float * 3)(*[float(v) for v in origin]), float(cell_size), *[int(d) for d in dims])


def grid_build(points, origin, cell_size, dims):
    """gstex_nn_grid_count, the scan (the binning's) and gstex_nn_grid_place: -> (cell_start (n_cells + 1) int32,
    records (n, 4) f32).  No read-back."""
    from .ops import _scan_offsets

    _dev(points, "points", torch.float32, 3)
    dev, n = points.device, points.shape[0]
    g = _grid_struct(origin, cell_size, dims)
    n_cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    if not _fits(dims):  # (the library refuses it too; its message names the limits)
        _lib.call("gstex_nn_grid_count", ctypes.byref(g), n, None, None, None)
    work = torch.empty((n_cells,), device=dev, dtype=torch.int32)
    st = _lib.stream_of(dev)
    _lib.call("gstex_nn_grid_count", ctypes.byref(g), n, ptr(points), ptr(work), st)
    cell_start = _scan_offsets(work)
    records = torch.empty((n, 4), device=dev, dtype=torch.float32)
    _lib.call("gstex_nn_grid_place", ctypes.byref(g), n, ptr(points), ptr(cell_start), ptr(work), ptr(records), st)
    return cell_start, records


def nn_query(origin, cell_size, dims, cell_start, records, query_records, k=1, exclude_self=False, max_radius=None):
    """gstex_nn_query: query_records (Q, 4) = (x, y, z, row) -> (d2 (Q, k) f32, index (Q, k) int32), row `row` holding
    that query's result."""
    _dev(records, "records", torch.float32, 4)
    _dev(query_records, "query_records", torch.float32, 4)
    dev, nq = records.device, query_records.shape[0]
    d2 = torch.empty((nq, int(k)), device=dev, dtype=torch.float32)
    index = torch.empty((nq, int(k)), device=dev, dtype=torch.int32)
    a = _lib.GstexNnQueryArgs(grid=_grid_struct(origin, cell_size, dims), n_points=records.shape[0],
                              cell_start=ptr(cell_start), records=ptr(records), n_queries=nq,
                              queries=ptr(query_records), k=int(k), exclude_self=int(bool(exclude_self)),
                              max_radius=float("inf") if max_radius is None else float(max_radius), d2=ptr(d2),
                              index=ptr(index))
    _lib.call("gstex_nn_query", ctypes.byref(a), _lib.stream_of(dev))
    return d2, index


class SamplePlan:
    """What sample_mesh_mark leaves for sample_mesh_emit: the total and the work arrays."""

    def __init__(self, args, keep, n_samples: int, n_max: int, device):
        self.args, self.keep, self.n_samples, self.n_max, self.device = args, keep, n_samples, n_max, device


def sample_mesh_mark(vertices, faces, spacing) -> SamplePlan:
    """gstex_mesh_sample_mark, the scan (the binning's) and the sampler's ONE read-back: the total, the largest n and
    the count of faces with an index outside the vertices, together.  Refuses what emit must not be given."""
    from .ops import _scan_offsets

    _dev(vertices, "vertices", torch.float32, 3)
    _dev(faces, "faces", torch.int32, 3)
    if not float(spacing) > 0:
        raise ValueError(f"spacing must be > 0 (got {spacing})")
    dev, F = vertices.device, faces.shape[0]
    count = torch.empty((F,), device=dev, dtype=torch.int32)
    stats = torch.zeros((4,), device=dev, dtype=torch.int32)
    a = _lib.GstexMeshSampleArgs(n_vertices=vertices.shape[0], n_faces=F, vertices=ptr(vertices), faces=ptr(faces),
                                 spacing=float(spacing), count=ptr(count), stats=ptr(stats))
    _lib.call("gstex_mesh_sample_mark", ctypes.byref(a), _lib.stream_of(dev))
    lo, hi, n_max, bad = (int(v) for v in stats.cpu().tolist())
    total = (lo & 0xffffffff) | (hi << 32)
    _check_sample_totals(total, n_max, bad, vertices.shape[0])
    offsets = _scan_offsets(count)  # total < 2^31: the int32 scan holds it
    a.offsets, a.n_samples = ptr(offsets), total
    return SamplePlan(a, (vertices, faces, count, stats, offsets), total, n_max, dev)


def sample_mesh_emit(plan: SamplePlan, samples, weights, face_of) -> None:
    """gstex_mesh_sample_emit into caller-sized buffers of at least n_samples rows; the kernel is told the plan's
    total and writes nothing past it."""
    _dev(samples, "samples", torch.float32, 3)
    ok = lambda t, dt: t.is_cuda and t.dtype == dt and t.dim() == 1 and t.is_contiguous()  # noqa: E731
    if not (ok(weights, torch.float32) and ok(face_of, torch.int32)):
        raise ValueError("weights / face_of: expected contiguous HIP float32 / int32 vectors")
    if min(samples.shape[0], weights.shape[0], face_of.shape[0]) < plan.n_samples:
        raise ValueError(f"the outputs hold fewer rows than the plan's {plan.n_samples} samples")
    a = plan.args
    a.samples, a.weights, a.face_of = samples.data_ptr(), weights.data_ptr(), face_of.data_ptr()
    _lib.call("gstex_mesh_sample_emit", ctypes.byref(a), _lib.stream_of(plan.device))


def sample_mesh(vertices, faces, spacing):
    """The deterministic area sampler: face (a, b, c) with longest edge L gets n = max(1, ceil(L / spacing)) and one
    sample at the centroid of each of its n^2 congruent sub-triangles, weight area / n^2; ascending face, then i, then
    j, upright before inverted.  Every point of the surface is within (2/3) spacing of a sample.  On the mesh's device
    (HIP: the kernels; CPU: the twin).  -> (samples (S, 3) f32, weights (S,) f32, face_of (S,) int32)."""
    if not vertices.is_cuda:
        return sample_mesh_eager(vertices, faces, spacing)
    vertices = vertices.detach().to(torch.float32).contiguous()
    faces = faces.to(torch.int32).contiguous()
    plan = sample_mesh_mark(vertices, faces, spacing)
    dev, S = vertices.device, plan.n_samples
    samples = torch.empty((S, 3), device=dev, dtype=torch.float32)
    weights = torch.empty((S,), device=dev, dtype=torch.float32)
    face_of = torch.empty((S,), device=dev, dtype=torch.int32)
    sample_mesh_emit(plan, samples, weights, face_of)
    return samples, weights, face_of


# ---------------------------------------------------------------------------------------- the index
class PointGrid:
    """A uniform-grid nearest-neighbour index over points (n, 3) fp32, built on the points' device (HIP: the kernels;
    CPU: the twins).  origin (the component-wise minimum), cell_size, dims (nx, ny, nz), cell_start (n_cells + 1) int32
    and records (n, 4) f32 = (x, y, z, index bits), a cell's records contiguous.  cell_size: default
    default_cell_size(n, bounds), enlarged to fit the cell limits; an explicit one that does not fit is refused, or,
    with fit=True, enlarged by a quarter at a time until it does."""

    def __init__(self, points, cell_size=None, fit: bool = False):
        if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[1] == 3):
            raise ValueError("points: expected an (n, 3) tensor")
        if points.shape[0] < 1 or points.shape[0] >= 1 << 31:
            raise ValueError(f"points: the count must be in [1, 2^31) (got {points.shape[0]})")
        self.points = points.detach().to(torch.float32).contiguous()
        self.device = self.points.device
        lo_hi = torch.stack([self.points.min(dim=0).values, self.points.max(dim=0).values]).cpu().numpy()  # the read-back
        if not np.isfinite(lo_hi).all():
            raise ValueError("points: the bounds are not finite")
        lo, hi = lo_hi[0], lo_hi[1]
        self.origin = tuple(float(v) for v in lo)
        if cell_size is None:
            self.cell_size = default_cell_size(self.points.shape[0], lo, hi)
        else:
            self.cell_size = _f32(cell_size)
            if not (self.cell_size > 0 and math.isfinite(self.cell_size)):
                raise ValueError(f"cell_size must be finite and > 0 (got {cell_size})")
            if fit:  # (as the default: no cell below 2^-20 of the longest extent)
                self.cell_size = max(self.cell_size, _f32(float((hi - lo).max()) * 2.0 ** -20))
            while fit and not _fits(grid_dims(lo, hi, self.cell_size)):
                self.cell_size = _f32(self.cell_size * 1.25)
        self.dims = grid_dims(lo, hi, self.cell_size)
        if self.device.type == "cuda":
            self.cell_start, self.records = grid_build(self.points, self.origin, self.cell_size, self.dims)
        else:
            if not _fits(self.dims):
                raise _lib.GstexError(f"PointGrid: too many cells {self.dims} (at most {_lib.NN_MAX_AXIS_CELLS} per "
                                      f"axis and {_lib.NN_MAX_CELLS} in all)")
            self.cell_start, self.records = grid_build_eager(self.points, self.origin, self.cell_size, self.dims)

    @property
    def n(self) -> int:
        return self.points.shape[0]

    def query(self, queries, k: int = 1, exclude_self: bool = False, max_radius=None):
        """The k (1..8) nearest points of each query, exactly as brute force gives them: -> (d2 (Q, k) f32 ascending,
        index (Q, k) int32), ties to the lower index, missing neighbours (+inf, -1).  exclude_self: the point whose
        index equals the query's row is skipped (a set queried against itself).  max_radius: points farther do not
        count.  Queries may lie anywhere, far outside the grid included; they must be finite."""
        if not 1 <= int(k) <= _lib.NN_MAX_K:
            raise ValueError(f"k must be in [1, {_lib.NN_MAX_K}] (got {k})")
        if max_radius is not None and not float(max_radius) >= 0:
            raise ValueError(f"max_radius must be >= 0 (got {max_radius})")
        if not (isinstance(queries, torch.Tensor) and queries.dim() == 2 and queries.shape[1] == 3
                and queries.device == self.device):
            raise ValueError(f"queries: expected a (Q, 3) tensor on {self.device}")
        queries = queries.detach().to(torch.float32).contiguous()
        if self.device.type != "cuda":
            return nn_query_eager(self.points, queries, int(k), exclude_self, max_radius)
        if queries.shape[0] == 0:
            return (torch.empty((0, int(k)), device=self.device), torch.empty((0, int(k)), device=self.device,
                                                                              dtype=torch.int32))
        # the queries in the order of their own (clamped) cells of this grid, by the same count -> scan -> place:
        # a wave's lanes then walk neighbouring cells
        if queries.data_ptr() == self.points.data_ptr() and queries.shape == self.points.shape:
            qrec = self.records
        else:
            _, qrec = grid_build(queries, self.origin, self.cell_size, self.dims)
        return nn_query(self.origin, self.cell_size, self.dims, self.cell_start, self.records, qrec, k, exclude_self,
                        max_radius)


def knn_mean_dist_device(points, k: int = 3) -> torch.Tensor:
    """The mean distance of each point to its k nearest other points (the initialisation's scale,
    scene.knn_mean_dist) on the points' device: -> (n,) f32.  The kernels give d2 in fp32; the roots and the mean are
    float64 torch ops, rounded once.  Fewer than k other points give inf."""
    grid = PointGrid(points)
    d2, _ = grid.query(grid.points, k=k, exclude_self=True)
    return torch.sqrt(d2.double()).mean(dim=-1).to(torch.float32)
