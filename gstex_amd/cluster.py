"""DBSCAN over the splats under the squared 2-Wasserstein distance of their flat Gaussians, on the device (the
reference's dbscan_clustering/dbscan_ballquery.py; DESIGN.md "Clustering the splats").

* dbscan                 (means, scales, quats, eps, min_pts) -> ClusterResult(labels, degree, core, n_clusters) on the
                         tensors' device (HIP: the kernels of gstex_amd/csrc/cluster.hip on a PointGrid of the means;
                         CPU: the brute-force twin)
* wasserstein2_eager     the distance contract in torch, operation for operation: (w2, d2, tr) of index pairs
* dbscan_eager           the brute-force twin: chunked O(N^2), no grid, labels by propagating the lowest core index
* dbscan_walk_eager      the kernels restated on the host, walk for walk and hook for hook (tests, small sets)
* pair_w2                gstex_cluster_pair_w2: (w2, d2, tr) of index pairs by the kernel
* keep_mask              labels -> the bool mask GStexTrainer.select takes (chosen ids, or clusters of a minimum size)
* cluster_summary / cluster_report / label_colors        the reference's analyze_clusters dictionary, its per-cluster
                         text report (statistics by index_add_ / scatter_reduce on the labels' device) and a colour per
                         label from a fixed hash

scales are ACTIVATED (n, >= 2; the first two columns count, the third scale of a flat splat is taken as zero) and quats
are UNIT quaternions (w, x, y, z): the caller activates, as GStexTrainer.cluster and export.cluster_ply do.  eps is a
threshold on the SQUARED distance, as throughout the reference; self is not counted towards min_pts (scikit-learn's
min_samples is min_pts + 1).  Labels are 1..K in the order of each cluster's lowest core index, -1 is noise; the result
depends on neither visit order nor thread timing, so kernels and twins agree exactly.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .neighbors import PointGrid, _f32, _s, grid_build_eager, sqrt_rn, walk_rings_eager


@dataclass
class ClusterResult:
    labels: torch.Tensor  # (n,) int32: 1..n_clusters, -1 noise
    degree: torch.Tensor  # (n,) int32: neighbours, self not counted
    core: torch.Tensor    # (n,) bool: degree >= min_pts
    n_clusters: int


# ---------------------------------------------------------------------------------------- the distance
def shapes_eager(scales, quats):
    """The scaled tangent axes a = s0 R[:, 0], b = s1 R[:, 1] and T = s0 s0 + s1 s1 of unit quaternions (w, x, y, z),
    in the kernel's operations: -> (a (n, 3), b (n, 3), T (n,))."""
    s0, s1 = scales[:, 0], scales[:, 1]
    w, x, y, z = quats[:, 0], quats[:, 1], quats[:, 2], quats[:, 3]
    r00 = 1.0 - 2.0 * (y * y + z * z)
    r10 = 2.0 * (x * y + w * z)
    r20 = 2.0 * (x * z - w * y)
    r01 = 2.0 * (x * y - w * z)
    r11 = 1.0 - 2.0 * (x * x + z * z)
    r21 = 2.0 * (y * z + w * x)
    a = torch.stack([s0 * r00, s0 * r10, s0 * r20], 1)
    b = torch.stack([s1 * r01, s1 * r11, s1 * r21], 1)
    return a, b, s0 * s0 + s1 * s1


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _trace_eager(ai, bi, Ti, aj, bj, Tj):
    m00, m01, m10, m11 = _dot(ai, aj), _dot(ai, bj), _dot(bi, aj), _dot(bi, bj)
    fro = (m00 * m00 + m11 * m11) + (m01 * m01 + m10 * m10)
    det = m00 * m11 - m01 * m10
    root = sqrt_rn(fro + 2.0 * det.abs())
    return torch.clamp((Ti + Tj) - 2.0 * root, min=0.0)


def _d2_eager(pi, pj):
    dx, dy, dz = pi[..., 0] - pj[..., 0], pi[..., 1] - pj[..., 1], pi[..., 2] - pj[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _splats(means, scales, quats):
    ok = lambda t, c: isinstance(t, torch.Tensor) and t.dim() == 2 and (t.shape[1] >= 2 if c == 2 else t.shape[1] == c)  # noqa: E731
    if not (ok(means, 3) and ok(scales, 2) and ok(quats, 4)):
        raise ValueError("expected means (n, 3), activated scales (n, >= 2) and unit quats (n, 4)")
    if not (means.shape[0] == scales.shape[0] == quats.shape[0]) or means.shape[0] >= 1 << 31:
        raise ValueError("means, scales and quats must hold the same number of splats, below 2^31")
    if not (means.device == scales.device == quats.device):
        raise ValueError("means, scales and quats must be on one device")
    f = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    return f(means), f(scales), f(quats)


def _check_params(eps, min_pts):
    eps = _f32(eps)
    if not (math.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0 (got {eps})")
    if int(min_pts) < 1:
        raise ValueError(f"min_pts must be >= 1 (got {min_pts})")
    return eps, int(min_pts)


def wasserstein2_eager(means, scales, quats, i, j):
    """The contract of gstex_hip.h in torch, one rounded fp32 operation each, roots through neighbors.sqrt_rn:
    -> (w2, d2, tr) of the pairs (i[k], j[k])."""
    means, scales, quats = _splats(means, scales, quats)
    i, j = i.long(), j.long()
    a, b, T = shapes_eager(scales, quats)
    d2 = _d2_eager(means[i], means[j])
    tr = _trace_eager(a[i], b[i], T[i], a[j], b[j], T[j])
    return d2 + tr, d2, tr


# ---------------------------------------------------------------------------------------- the brute-force twin
def neighbor_pairs_eager(means, scales, quats, eps, budget: int = 1 << 24):
    """Every ordered pair (i, j), j != i, with w2 <= eps, by brute force over rows in chunks of about `budget`
    distances: d2 <= eps first (w2 >= d2 holds in fp32), the trace term for the survivors.  -> (i, j) int64, sorted."""
    n = means.shape[0]
    a, b, T = shapes_eager(scales, quats)
    e = _s(eps, means)
    src, dst = [], []
    rows = max(1, budget // max(n, 1))
    for r0 in range(0, n, rows):
        d2 = _d2_eager(means[r0:r0 + rows, None, :], means[None, :, :])
        near = d2 <= e
        near[torch.arange(near.shape[0], device=means.device), torch.arange(r0, r0 + near.shape[0], device=means.device)] = False
        i, j = torch.nonzero(near, as_tuple=True)
        d, i = d2[i, j], i + r0
        keep = (d + _trace_eager(a[i], b[i], T[i], a[j], b[j], T[j])) <= e
        src.append(i[keep])
        dst.append(j[keep])
    if not src:
        z = torch.zeros(0, dtype=torch.int64, device=means.device)
        return z, z
    return torch.cat(src), torch.cat(dst)


def labels_from_pairs(n: int, src, dst, min_pts: int) -> ClusterResult:
    """The labelling's definitions on a neighbour list: the lowest core index of each component of the cores by
    propagating minima along core-core pairs (with pointer jumping) to the fixed point, ids by rank, the others by
    the lowest id among their core neighbours."""
    dev = src.device
    degree = torch.bincount(src, minlength=n)
    core = degree >= min_pts
    cc = core[src] & core[dst]
    s, d = src[cc], dst[cc]
    low = torch.arange(n, device=dev)
    while True:
        nxt = low.clone().scatter_reduce_(0, s, low[d], "amin")
        nxt = nxt[nxt]
        if torch.equal(nxt, low):
            break
        low = nxt
    roots = core & (low == torch.arange(n, device=dev))
    rank = torch.cumsum(roots.to(torch.int64), 0) - roots.to(torch.int64)  # the exclusive scan
    ids = torch.where(core, rank[low] + 1, torch.full_like(low, -1))
    big = n + 1
    border = torch.full((n,), big, dtype=torch.int64, device=dev)
    to_core = core[dst] & ~core[src]
    border.scatter_reduce_(0, src[to_core], ids[dst[to_core]], "amin")
    labels = torch.where(core, ids, torch.where(border < big, border, torch.full_like(border, -1)))
    return ClusterResult(labels.to(torch.int32), degree.to(torch.int32), core, int(roots.sum()))


def dbscan_eager(means, scales, quats, eps, min_pts) -> ClusterResult:
    """The brute-force twin of the kernels: chunked O(N^2), no grid, on the tensors' device."""
    means, scales, quats = _splats(means, scales, quats)
    eps, min_pts = _check_params(eps, min_pts)
    src, dst = neighbor_pairs_eager(means, scales, quats, eps)
    return labels_from_pairs(means.shape[0], src, dst, min_pts)


# ---------------------------------------------------------------------------------------- the grid
def cluster_grid(means, eps, cell_size=None) -> PointGrid:
    """The PointGrid of the means for a fixed-radius walk of squared radius eps.  Default cell: sqrt(eps) (1 + 2^-9),
    just enough above sqrt(eps) for the ring-stop test ((float)r h)(1 - 2^-10), squared, >= eps to end the walk after
    ring 1 (27 cells), enlarged a quarter at a time until the grid fits the cell limits; eps = 0 (or a root that
    underflows): the PointGrid default.  An explicit cell_size is taken as it is, and refused if the grid does not
    fit.  Correctness does not depend on it."""
    if cell_size is not None:
        return PointGrid(means, cell_size=cell_size)
    h = _f32(math.sqrt(eps) * (1.0 + 2.0 ** -9))
    return PointGrid(means, cell_size=h, fit=True) if h > 0 else PointGrid(means)


# ---------------------------------------------------------------------------------------- the kernels on the host
def dbscan_walk_eager(means, scales, quats, eps, min_pts, cell_size=None) -> ClusterResult:
    """gstex_cluster_degree / _link / _roots / _assign restated on the host in python loops (for tests and small sets):
    the twin-built grid, each record's ring walk (neighbors.walk_rings_eager, stopped on eps), d2 <= eps before the
    trace term, the union-find with path halving and the higher root hooked under the lower, the flags' exclusive scan
    and the second walk of the splats that are no core.  Must equal dbscan_eager."""
    means, scales, quats = _splats(means.cpu(), scales.cpu(), quats.cpu())
    eps, min_pts = _check_params(eps, min_pts)
    n = means.shape[0]
    if n == 0:
        return _empty(means.device)
    f = np.float32
    # the grid of the finite means (PointGrid refuses other bounds); the kernels place every record they are given,
    # a NaN coordinate in cell 0, and walk from it by the query cell's own NaN rule
    grid = cluster_grid(means[torch.isfinite(means).all(dim=1)], eps, cell_size)
    cell_start, records = grid_build_eager(means, grid.origin, grid.cell_size, grid.dims)
    rec = records.numpy()
    pts, idx = rec[:, :3], np.ascontiguousarray(rec[:, 3]).view(np.int32).astype(np.int64)
    cs = cell_start.numpy().astype(np.int64)
    a, b, T = shapes_eager(scales, quats)
    a, b, T = a[idx], b[idx], T[idx]  # the shape records, in record order
    e = f(eps)

    def neighbors_of(t):
        q = pts[t]
        out = []

        def scan(p, pe):
            if pe <= p:
                return
            d = q[None, :] - pts[p:pe]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            near = np.nonzero((d2 <= e) & (idx[p:pe] != idx[t]))[0]
            if near.size:
                s = torch.from_numpy(near + p)
                tr = _trace_eager(a[t], b[t], T[t], a[s], b[s], T[s]).numpy()
                out.extend(int(v) for v in idx[p:pe][near[(d2[near] + tr) <= e]])

        walk_rings_eager(q, grid.origin, grid.cell_size, grid.dims, cs, scan, lambda: e)
        return out

    nbrs = {int(idx[t]): neighbors_of(t) for t in range(n)}
    degree = np.array([len(nbrs[i]) for i in range(n)], np.int32)
    core = degree >= min_pts
    parent = np.arange(n)

    def find(x):
        while True:
            p = parent[x]
            if p >= x:
                return x
            gp = parent[p]
            if gp < p:
                parent[x] = min(parent[x], gp)
                x = gp
            else:
                x = p

    for t in range(n):  # in record order, as the kernel's threads are laid out
        i = int(idx[t])
        if core[i]:
            for j in nbrs[i]:
                if j < i and core[j]:
                    u, v = find(i), find(j)
                    if u != v:
                        parent[max(u, v)] = min(u, v)
    for i in range(n):
        parent[i] = find(i)
    flag = (core & (parent == np.arange(n))).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(flag)])
    labels = np.full(n, -1, np.int32)
    for i in range(n):
        if core[i]:
            labels[i] = offsets[parent[i]] + 1
        elif degree[i] > 0:
            ids = [offsets[parent[j]] + 1 for j in nbrs[i] if core[j]]
            if ids:
                labels[i] = min(ids)
    return ClusterResult(torch.from_numpy(labels), torch.from_numpy(degree), torch.from_numpy(core), int(offsets[n]))


# ---------------------------------------------------------------------------------------- HIP entry points
def _empty(dev) -> ClusterResult:
    return ClusterResult(torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                         torch.empty(0, dtype=torch.bool, device=dev), 0)


def pair_w2(means, scales, quats, pairs):
    """gstex_cluster_pair_w2: pairs (P, 2) of splat indices -> (w2, d2, tr), (P,) f32 each, on the device."""
    means, scales, quats = _splats(means, scales, quats)
    if not (means.is_cuda and isinstance(pairs, torch.Tensor) and pairs.dim() == 2 and pairs.shape[1] == 2
            and pairs.device == means.device):
        raise ValueError("pair_w2: expected HIP tensors and pairs (P, 2) on the same device")
    pairs = pairs.to(torch.int32).contiguous()
    P = pairs.shape[0]
    d2, tr, w2 = (torch.empty((P,), device=means.device, dtype=torch.float32) for _ in range(3))
    _lib.call("gstex_cluster_pair_w2", means.shape[0], ptr(means), ptr(scales), scales.shape[1], ptr(quats), P,
              ptr(pairs), ptr(d2), ptr(tr), ptr(w2), _lib.stream_of(means.device))
    return w2, d2, tr


def dbscan_device(means, scales, quats, eps, min_pts, cell_size=None, timings=None) -> ClusterResult:
    """The kernels, in order: the grid (PointGrid: the bounds read-back, count, scan, place), shapes, degree, link,
    roots, the scan of the root flags, ONE read-back (the number of clusters), assign.  timings: a dict that receives
    each step's milliseconds by timing events (tools/cluster_bench.py); it synchronises."""
    from .ops import _scan_offsets

    dev, n = means.device, means.shape[0]
    st = _lib.stream_of(dev)
    marks = []

    def mark(name):
        if timings is not None:
            ev = _lib.TimingEvent()
            ev.record(dev)
            marks.append((name, ev))

    mark("start")
    grid = cluster_grid(means, eps, cell_size)
    mark("grid")
    shapes = torch.empty((n, 8), device=dev, dtype=torch.float32)
    _lib.call("gstex_cluster_shapes", n, ptr(grid.records), ptr(scales), scales.shape[1], ptr(quats), ptr(shapes), st)
    mark("shapes")
    degree, parent, flag, labels = (torch.empty((n,), device=dev, dtype=torch.int32) for _ in range(4))
    g = _lib.GstexNnGrid((ctypes.c_float * 3)(*grid.origin), grid.cell_size, *grid.dims)
    a = _lib.GstexClusterArgs(grid=g, n=n, cell_start=ptr(grid.cell_start), records=ptr(grid.records),
                              shapes=ptr(shapes), eps=eps, min_pts=min_pts, degree=ptr(degree), parent=ptr(parent))
    _lib.call("gstex_cluster_degree", ctypes.byref(a), st)
    mark("degree")
    _lib.call("gstex_cluster_link", ctypes.byref(a), st)
    mark("link")
    _lib.call("gstex_cluster_roots", n, min_pts, ptr(degree), ptr(parent), ptr(flag), st)
    mark("roots")
    offsets = _scan_offsets(flag)
    mark("scan")
    a.offsets, a.labels = ptr(offsets), ptr(labels)
    _lib.call("gstex_cluster_assign", ctypes.byref(a), st)
    mark("assign")
    n_clusters = int(offsets[n])  # the read-back
    if timings is not None:
        torch.cuda.synchronize(dev)
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            timings[name + "_ms"] = e0.elapsed_time(e1)
        timings["cell_size"], timings["dims"] = grid.cell_size, grid.dims
    return ClusterResult(labels, degree, degree >= min_pts, n_clusters)


def dbscan(means, scales, quats, eps, min_pts, cell_size=None) -> ClusterResult:
    """DBSCAN of the splats under w2 <= eps (the module's docstring has the definitions).  On the tensors' device: HIP
    tensors run the kernels, CPU tensors the brute-force twin (which has no grid: cell_size is then unused).
    cell_size: the grid's cell, for tests; the result does not depend on it."""
    means, scales, quats = _splats(means, scales, quats)
    eps, min_pts = _check_params(eps, min_pts)
    if means.shape[0] == 0:
        return _empty(means.device)
    if not means.is_cuda:
        return dbscan_eager(means, scales, quats, eps, min_pts)
    return dbscan_device(means, scales, quats, eps, min_pts, cell_size)


# ---------------------------------------------------------------------------------------- acting on the labels
def keep_mask(labels_or_result, *, labels=None, min_size: int = 1, drop_noise: bool = True) -> torch.Tensor:
    """The bool (n,) mask GStexTrainer.select takes, from a ClusterResult or its labels (n,), on the labels' device.
    labels: the cluster ids to keep (min_size is then not applied); otherwise every cluster of at least min_size
    members.  Noise (-1) is kept only with drop_noise=False."""
    lab = labels_or_result.labels if isinstance(labels_or_result, ClusterResult) else torch.as_tensor(labels_or_result)
    if lab.dim() != 1 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError("keep_mask: expected integer labels of shape (n,)")
    lab = lab.long()
    member = lab >= 1
    if labels is not None:
        ids = torch.as_tensor(list(labels) if not isinstance(labels, torch.Tensor) else labels, dtype=torch.int64,
                              device=lab.device).reshape(-1)
        if bool((ids < 1).any()):
            raise ValueError("keep_mask: cluster ids are >= 1 (noise is kept with drop_noise=False)")
        keep = member & torch.isin(lab, ids)
    else:
        if int(min_size) < 1:
            raise ValueError(f"keep_mask: min_size must be >= 1 (got {min_size})")
        sizes = torch.bincount(lab[member])  # sizes[k]: members of cluster k
        keep = member.clone()
        keep[member] = sizes[lab[member]] >= int(min_size)
    return keep if drop_noise else keep | (lab == -1)


# ---------------------------------------------------------------------------------------- reports
def cluster_summary(labels) -> dict:
    """The reference's analyze_clusters dictionary (dbscan_ballquery.py:509-518), same keys: cluster_sizes in
    ascending label order."""
    labels = torch.as_tensor(labels)
    n_total = int(labels.shape[0])
    n_noise = int((labels == -1).sum())
    ids, counts = torch.unique(labels[labels >= 0], return_counts=True)
    sizes = [int(c) for c in counts.cpu()]
    return {"n_clusters": len(sizes), "n_noise_points": n_noise, "n_total_points": n_total,
            "noise_ratio": n_noise / n_total if n_total else 0.0, "cluster_sizes": sizes,
            "avg_cluster_size": float(np.mean(sizes)) if sizes else 0, "largest_cluster_size": max(sizes) if sizes else 0,
            "smallest_cluster_size": min(sizes) if sizes else 0}


def cluster_stats(result: ClusterResult, means, opacities, scales) -> dict:
    """Per-cluster size, centre, box minimum and maximum, mean opacity and mean scale, row k for label k + 1, by
    index_add_ / scatter_reduce on the labels' device (no loop over clusters)."""
    lab = result.labels.long()
    dev, K = lab.device, int(result.n_clusters)
    member = lab >= 1
    k = lab[member] - 1
    f = lambda t: torch.as_tensor(t).detach().to(dev, torch.float64).reshape(lab.shape[0], -1)[member]  # noqa: E731
    xyz, op, sc = f(means), f(opacities), f(scales)
    size = torch.bincount(k, minlength=K).to(torch.float64)
    total = lambda v: torch.zeros((K, v.shape[1]), dtype=torch.float64, device=dev).index_add_(0, k, v)  # noqa: E731
    ki = k[:, None].expand(-1, 3)
    lo = torch.full((K, 3), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, ki, xyz, "amin")
    hi = torch.full((K, 3), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, ki, xyz, "amax")
    return {"size": size.to(torch.int64), "center": total(xyz) / size[:, None], "lo": lo, "hi": hi,
            "opacity": total(op)[:, 0] / size, "scale": total(sc) / size[:, None]}


def cluster_report(path, result: ClusterResult, means, opacities, scales) -> dict:
    """The reference's per-cluster text report (demo_ballquery_dbscan.py save_cluster_results): the totals, then per
    cluster its size, centre, bounding box, mean opacity and mean scale (of the opacities and scales passed in), then
    the summary.  -> cluster_stats' dictionary."""
    st = {k: v.cpu().numpy() for k, v in cluster_stats(result, means, opacities, scales).items()}
    n_total, K = int(result.labels.shape[0]), int(result.n_clusters)
    n_noise = int((result.labels == -1).sum())
    fmt = lambda v: ", ".join(f"{x:.3f}" for x in v)  # noqa: E731
    lines = ["Ball Query DBSCAN Clustering Results", "=" * 50, "", f"Total points: {n_total}",
             f"Number of clusters: {K}", f"Noise points: {n_noise}",
             f"Noise ratio: {n_noise / max(n_total, 1):.2%}", ""]
    for k in range(K):
        box = st["hi"][k] - st["lo"][k]
        lines += [f"Cluster {k + 1}:", f"  Size: {st['size'][k]} points ({st['size'][k] / n_total * 100:.1f}%)",
                  f"  Center: ({fmt(st['center'][k])})", f"  Bounding box: {' x '.join(f'{x:.3f}' for x in box)}",
                  f"  Avg opacity: {st['opacity'][k]:.3f}", f"  Avg scale: ({fmt(st['scale'][k])})", ""]
    if K:
        sizes = st["size"]
        lines += ["Summary Statistics:", "-" * 30, f"Average cluster size: {sizes.mean():.1f}",
                  f"Largest cluster: {sizes.max()} points", f"Smallest cluster: {sizes.min()} points",
                  f"Cluster size std dev: {sizes.std():.1f}", f"Average cluster opacity: {st['opacity'].mean():.3f}",
                  f"Average cluster scale: ({fmt(st['scale'].mean(axis=0))})", ""]
    with open(path, "w") as out:
        out.write("\n".join(lines))
    return st


def label_colors(labels) -> np.ndarray:
    """A colour per label from a fixed hash (Knuth's multiplicative constant on the label, three of its bytes), grey
    for noise: -> (n, 3) uint8.  No random generator is involved."""
    lab = np.asarray(torch.as_tensor(labels).cpu()).astype(np.int64)
    h = (lab * 2654435761) & 0xFFFFFFFF
    rgb = np.stack([(h >> 24) & 255, (h >> 16) & 255, (h >> 8) & 255], 1).astype(np.uint8)
    rgb[lab < 1] = 128
    return rgb
