"""Nearest neighbours, the mesh sampler and the mesh score without a GPU: the eager twins of gstex_amd.neighbors against
independent float64 searches and the contract's own formulas, the kernel's ring walk restated on the host against exact
brute force on the grid's edge cases, score_mesh's semantics, the opt-in initialisation route and the C ABI's argument
checks."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mesh_cases as MC
import neighbor_cases as NC
from gstex_amd import _lib
from gstex_amd import mesh as M
from gstex_amd import neighbors as N

U = 2.0 ** -24  # the unit round-off of fp32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_golden.npz")


# ---------------------------------------------------------------------------------------- 1. twin vs cKDTree
@pytest.mark.parametrize("k", [1, 3, 8])
def test_twin_matches_an_independent_search(k):
    """nn_query_eager on 3,000 x 2,000 uniform points against scipy's k-d tree in float64.

    The bound.  The inputs are fp32 numbers, exact in float64.  d2 = (dx*dx + dy*dy) + dz*dz takes, on its longest
    path, five rounded operations: the subtraction (relative u = 2^-24 on dx, so 2 u on its square), the product (u)
    and the two sums (u each; every term is >= 0, so a sum's relative error is at most the larger of its terms' plus
    u).  d2 is therefore within 5 u = 2.98e-7 of the exact value, relatively, and its float64 root within 2.5 u; the
    tree's own float64 rounding is 1e-16.  The issue's bound of 1e-6 is asserted; 5 u is what the figures must meet
    and is asserted as well.  A row's indices are compared unless two consecutive of its first k + 1 float64 distances
    are closer than 1e-6 relatively (their order is then not decided in fp32); such rows are at most 1 % by the
    issue, and on these inputs none is expected: a gap below 1e-6 d between two of 3,000 uniform neighbours has a
    probability near 3 d^3 * 4 pi * 3000 * 1e-6, about 1e-4 per row at the eighth neighbour's d = 0.08."""
    from scipy.spatial import cKDTree

    g = torch.Generator().manual_seed(100)
    P, Q = torch.rand((3000, 3), generator=g), torch.rand((2000, 3), generator=g)
    d2, idx = N.nn_query_eager(P, Q, k)
    dd, ii = cKDTree(P.double().numpy()).query(Q.double().numpy(), k=k + 1)
    got = np.sqrt(d2.double().numpy())
    rel = np.abs(got / dd[:, :k] - 1.0).max()
    print(f"k = {k}: max relative distance error {rel:.3e} (5 u = {5 * U:.3e})")
    assert rel <= 5 * U and rel <= 1e-6
    assert bool((d2[:, 1:] >= d2[:, :-1]).all())
    close = ((dd[:, 1:] - dd[:, :-1]) <= 1e-6 * dd[:, 1:]).any(axis=1)
    share = float(close.mean())
    print(f"k = {k}: rows excused {share:.4%}")
    assert share <= 0.01 and share <= 0.001
    assert (idx.numpy()[~close] == ii[~close, :k]).all()


# ---------------------------------------------------------------------------------------- 2. grid cases
def _brute64(P, Q, k, exclude_self, max_radius):
    """Exact brute force on the fp32 d2 values, sorted by (d2, index) in python: independent of torch.sort."""
    p, q = P.numpy(), Q.numpy()
    r2 = np.float32(np.inf) if max_radius is None else np.float32(max_radius) * np.float32(max_radius)
    out_d = np.full((q.shape[0], k), np.inf, np.float32)
    out_i = np.full((q.shape[0], k), -1, np.int32)
    for row in range(q.shape[0]):
        d = q[row][None] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cand = sorted((dv, i) for i, dv in enumerate(d2) if dv <= r2 and not (exclude_self and i == row))[:k]
        for s, (dv, i) in enumerate(cand):
            out_d[row, s], out_i[row, s] = dv, i
    return torch.from_numpy(out_d), torch.from_numpy(out_i)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", list(NC.grid_cases()))
def test_grid_cases_equal_brute_force(name):
    """Each edge case of the grid on the twins with an explicit cell size: the kernel's ring walk restated on the host
    (nn_query_walk_eager, on the twin-built grid) and the brute-force twin (what PointGrid.query runs on the CPU) both
    equal an exact brute force written here, bit for bit."""
    c = NC.grid_cases()[name]
    grid = N.PointGrid(c["points"], cell_size=c["cell_size"])
    kw = dict(k=c["k"], exclude_self=c["exclude_self"], max_radius=c["max_radius"])
    want = _brute64(c["points"], c["queries"], **kw)
    twin = grid.query(c["queries"], **kw)
    walk = N.nn_query_walk_eager(grid.origin, grid.cell_size, grid.dims, grid.cell_start, grid.records, c["queries"],
                                 **kw)
    for got, what in ((twin, "brute-force twin"), (walk, "ring walk")):
        assert torch.equal(_bits(got[0]), _bits(want[0])), (name, what)
        assert torch.equal(got[1], want[1]), (name, what)
    # the grid itself: every point in the cell the contract names, the maximum in the last cell
    nx, ny, nz = grid.dims
    assert int(grid.cell_start[0]) == 0 and int(grid.cell_start[-1]) == grid.n == c["points"].shape[0]
    rec_idx = grid.records[:, 3].contiguous().view(torch.int32).long()
    assert torch.equal(torch.sort(rec_idx).values, torch.arange(grid.n))
    assert torch.equal(_bits(grid.records[:, :3].contiguous()), _bits(c["points"][rec_idx].contiguous()))
    hi_cell = N._cells_eager(c["points"].max(dim=0).values[None], grid.origin, grid.cell_size, grid.dims)[0]
    assert hi_cell.tolist() == [nx - 1, ny - 1, nz - 1]


def test_grid_cases_are_what_they_claim():
    cs = NC.grid_cases()
    g = {n: N.PointGrid(c["points"], cell_size=c["cell_size"]) for n, c in cs.items()}
    assert g["one_cell"].dims == (1, 1, 1)
    assert g["tiny_cells"].dims == (101, 101, 1) and 1.0 / g["tiny_cells"].cell_size >= 49.9
    assert g["boundaries"].dims == (5, 5, 5) and int(g["boundaries"].cell_start[-1] - g["boundaries"].cell_start[-2]) == 1
    assert g["coincident"].dims == (1, 1, 1) and g["single_point"].n == 1
    d2, idx = g["k_above_n"].query(cs["k_above_n"]["queries"], k=8)
    assert bool(torch.isinf(d2[:, 5:]).all()) and bool((idx[:, 5:] == -1).all()) and bool((idx[:, :5] >= 0).all())
    d2, idx = g["radius_excludes_all"].query(cs["radius_excludes_all"]["queries"], k=3, max_radius=0.5)
    assert bool(torch.isinf(d2).all()) and bool((idx == -1).all())
    d2, idx = g["radius_cuts_2_3"].query(cs["radius_cuts_2_3"]["queries"], k=4, max_radius=2.0)
    assert idx.tolist() == [[0, 1, -1, -1]] and d2[0, :2].tolist() == [0.25, 2.25]
    c = cs["duplicates_exclude_self"]
    d2, idx = g["duplicates_exclude_self"].query(c["queries"], k=3, exclude_self=True)
    assert bool((d2[:, 0] == 0).all()) and bool((idx[:, 0] != torch.arange(idx.shape[0])).all())  # the twin point stays
    d2, idx = g["lattice_ties"].query(cs["lattice_ties"]["queries"], k=8)
    assert bool((d2[:27] == 0.75).all()) and bool((idx[:27, 1:] > idx[:27, :-1]).all())  # eight ties, ascending index
    far = g["far_outside"].query(cs["far_outside"]["queries"], k=3)[0]
    assert bool(torch.isfinite(far).all()) and float(far.min()) > 50.0 ** 2


def _walk(grid, q, scan, bound):
    N.walk_rings_eager(np.asarray(q, np.float32), grid.origin, grid.cell_size, grid.dims,
                       grid.cell_start.numpy().astype(np.int64), scan, bound)


@pytest.mark.parametrize("name, row", [("tiny_cells", 4), ("boundaries", 62), ("one_cell", 0), ("far_outside", 7)])
def test_walk_delivers_every_record_exactly_once(name, row):
    """walk_rings_eager on its own, never stopped (bound = +inf): the runs it delivers, concatenated, hold every record
    index of [0, n) exactly once -- each ring's cells once, no cell twice, none missed.  One query of the case's own
    per grid: between the points of the plane and off it (tiny_cells: about fifty rings, the first ones empty), the
    lattice's centre (boundaries: rings with rows through their inside), inside the only cell, and 1e6 away."""
    c = NC.grid_cases()[name]
    grid = N.PointGrid(c["points"], cell_size=c["cell_size"])
    if name == "far_outside":
        assert c["queries"][row].tolist() == [1e6, -1e6, 1e6]
    runs = []
    _walk(grid, c["queries"][row].numpy(), lambda a, b: runs.append((int(a), int(b))), lambda: np.float32(np.inf))
    assert all(0 <= a <= b <= grid.n for a, b in runs)
    seen = np.concatenate([np.arange(a, b) for a, b in runs])
    assert seen.shape[0] == grid.n and (np.sort(seen) == np.arange(grid.n)).all()


def test_walk_stops_on_its_bound():
    """radius_cuts_2_3 with the fixed bound r2 = 2 * 2 (fp32): once a ring r >= 1 has ((float)r h)(1 - 2^-10), squared,
    >= r2, no further run is delivered, and every point within r2 of the query lies in a delivered run.  bound() is
    called once after each ring r >= 1, which numbers the rings from the first one (query_cell_eager is the
    walker's own cell)."""
    f = np.float32
    c = NC.grid_cases()["radius_cuts_2_3"]
    grid = N.PointGrid(c["points"], cell_size=c["cell_size"])
    q = c["queries"][0].numpy()
    r2 = f(2.0) * f(2.0)
    cell = N.query_cell_eager(q, grid.origin, grid.cell_size)
    r_first = max(max(-v, v - (d - 1), 0) for v, d in zip(cell, grid.dims))
    state = {"r": max(r_first, 1), "stopped": False}
    runs = []

    def scan(a, b):
        assert not state["stopped"], f"a run of ring {state['r']} after the bound was reached"
        runs.append((int(a), int(b)))

    def bound():
        lb = f(f(state["r"]) * f(grid.cell_size)) * f(1.0 - 2.0 ** -10)
        state["stopped"] = bool(lb * lb >= r2)
        state["r"] += 1
        return r2

    _walk(grid, q, scan, bound)
    assert state["stopped"]  # the walk ended on the test, not on the grid's last ring
    seen = set(int(i) for a, b in runs for i in range(a, b))
    assert len(seen) < grid.n
    rec = grid.records.numpy()
    d = q[None] - rec[:, :3]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    within = set(np.nonzero(d2 <= r2)[0].tolist())
    assert len(within) == 2 and within <= seen


def test_walk_cell_rule_and_the_cluster_twin():
    """A NaN coordinate gives the cell -2^29 and one at 1e30 the cell +2^29 on that axis, and the walk of such a query
    returns.  dbscan_walk_eager has the rule from the shared walker: with one mean NaN it returns, that splat noise (a
    NaN query passes no d2 <= eps test, and no other record's scan admits the NaN record), as the kernels give."""
    import cluster_cases as CC
    from gstex_amd import cluster as C

    c = NC.grid_cases()["one_cell"]
    grid = N.PointGrid(c["points"], cell_size=c["cell_size"])
    q = np.array([float("nan"), 0.5, 1e30], np.float32)
    assert N.query_cell_eager(q, grid.origin, grid.cell_size) == (-2 ** 29, 0, 2 ** 29)
    for bad in (np.array([float("nan"), 0.5, 0.5], np.float32), np.array([0.5, 0.5, 1e30], np.float32)):
        runs = []
        _walk(grid, bad, lambda a, b: runs.append((int(a), int(b))), lambda: np.float32(np.inf))
        assert runs == [(0, grid.n)]
    s = CC.cases()["two_blobs_noise"]
    means = s["means"].clone()
    means[17, 1] = float("nan")
    got = C.dbscan_walk_eager(means, s["scales"], s["quats"], s["eps"], 5)
    assert int(got.labels[17]) == -1 and int(got.degree[17]) == 0
    want = C.dbscan_eager(means, s["scales"], s["quats"], s["eps"], 5)
    assert torch.equal(got.labels, want.labels) and torch.equal(got.degree, want.degree)
    assert got.n_clusters == want.n_clusters >= 2


def test_default_cell_size_and_limits():
    P, _ = NC.random_case()
    grid = N.PointGrid(P)
    per_cell = grid.n / (grid.dims[0] * grid.dims[1] * grid.dims[2])
    assert 0.05 < per_cell < 50  # a heuristic: correctness does not depend on it (the cases above fix the cell size)
    with pytest.raises(_lib.GstexError, match="too many cells"):
        N.PointGrid(P, cell_size=1e-5)
    with pytest.raises(ValueError):
        N.PointGrid(P, cell_size=0.0)
    bad = P.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        N.PointGrid(bad)
    flat = P.clone()
    flat[:, 2] = 0.25
    assert N.PointGrid(flat).dims[2] == 1
    with pytest.raises(ValueError):
        grid.query(P[:4], k=9)
    with pytest.raises(ValueError):
        grid.query(P[:4], k=0)


# ---------------------------------------------------------------------------------------- 3. sampler
def _expected_samples64(vertices, faces, spacing):
    """The contract in float64, by python loops in the contract's order."""
    V = vertices.double().numpy()
    pts, wts, fo, bary = [], [], [], []
    for f, (a, b, c) in enumerate(faces.tolist()):
        pa, pb, pc = V[a], V[b], V[c]
        L = max(np.linalg.norm(pb - pa), np.linalg.norm(pc - pa), np.linalg.norm(pc - pb))
        n = max(1, math.ceil(L / spacing))
        area = 0.5 * np.linalg.norm(np.cross(pb - pa, pc - pa))
        for i in range(n):
            for j in range(n - i):
                for inv in (0, 1):
                    if inv and i + j > n - 2:
                        continue
                    u, v = (i + (1 + inv) / 3) / n, (j + (1 + inv) / 3) / n
                    pts.append(pa + u * (pb - pa) + v * (pc - pa))
                    wts.append(area / n ** 2)
                    fo.append(f)
                    bary.append((u, v))
    return np.array(pts), np.array(wts), np.array(fo), np.array(bary)


def _sampler_meshes():
    V, F, r, h = NC.sphere_mesh()
    hv, hf, hs, _ = NC.hand_mesh()
    return {"sphere": (V, F, 0.5 * h), "sphere_coarse": (V, F, 4.0 * h), "hand": (hv, hf, hs)}


@pytest.mark.parametrize("name", ["sphere", "sphere_coarse", "hand"])
def test_sampler_follows_the_contract(name):
    """n^2 samples per face in the contract's order at the contract's positions (float64 restatement; the fp32 result
    within 8 u of the face's largest coordinate, so on the face's plane and inside it within rounding), barycentric
    coordinates in [0, 1], weights summing to the float64 area within 1e-5, and every vertex and face centroid within
    (2/3) spacing of a sample."""
    V, F, spacing = _sampler_meshes()[name]
    S, W, face_of = N.sample_mesh_eager(V, F, spacing)
    pts, wts, fo, bary = _expected_samples64(V, F, spacing)
    assert S.shape == (pts.shape[0], 3) and S.dtype == torch.float32 and face_of.dtype == torch.int32
    assert (face_of.numpy() == fo).all()
    counts = np.bincount(fo, minlength=F.shape[0])
    assert (np.sqrt(counts).round() ** 2 == counts).all() and counts.min() >= 1
    if name == "hand":
        assert counts.tolist() == [n * n for n in NC.hand_mesh()[3]]
    scale = float(V.abs().max())
    assert float(np.abs(S.double().numpy() - pts).max()) <= 8 * U * scale
    assert bary.min() > 0 and bary.max() < 1 and (bary.sum(1) < 1).all()
    area = NC.mesh_area64(V, F)
    assert abs(float(W.double().sum()) - area) <= 1e-5 * area
    assert float(np.abs(W.double().numpy() - wts).max()) <= 1e-5 * max(wts.max(), 1e-30) + 4 * U * scale * scale
    targets = torch.cat([V.double(), V.double()[F.long()].mean(dim=1)])
    nearest = torch.cdist(targets, S.double()).min(dim=1).values
    assert float(nearest.max()) <= (2.0 / 3.0) * spacing + 8 * U * scale


def test_sampler_refusals():
    V, F, spacing, _ = NC.hand_mesh()
    with pytest.raises(ValueError, match="subdivisions"):
        N.sample_mesh_eager(V, F, 1e-3)
    bad = F.clone()
    bad[2, 1] = V.shape[0]
    with pytest.raises(ValueError, match="outside"):
        N.sample_mesh_eager(V, bad, spacing)
    with pytest.raises(ValueError):
        N.sample_mesh_eager(V, F, 0.0)
    S, W, fo = N.sample_mesh_eager(V, F[:0], spacing)
    assert S.shape == (0, 3) and W.shape == (0,) and fo.shape == (0,)


# ---------------------------------------------------------------------------------------- 4. score semantics
def test_score_of_a_mesh_against_its_own_samples():
    V, F, r, h = NC.sphere_mesh()
    S, _, _ = M.sample_mesh(V, F, h)  # (faces of n = 1 and 2)
    assert F.shape[0] < S.shape[0] < 4 * F.shape[0]
    sc = M.score_mesh(V, F, S, spacing=h, thresholds=(1e-6, 0.1))
    assert sc["accuracy"] == 0 and sc["completeness"] == 0 and sc["chamfer"] == 0
    assert sc["precision"] == [1.0, 1.0] and sc["recall"] == [1.0, 1.0] and sc["fscore"] == [1.0, 1.0]
    assert sc["n_samples"] == S.shape[0] == sc["n_reference"]


@pytest.fixture(scope="module")
def offset_sphere():
    """The sphere mesh of radius r, 2,000 reference points on the sphere of radius r + delta and the terms of the
    bound, none of them from the code under test."""
    V, F, r, h = NC.sphere_mesh()
    delta, spacing = 0.05, 0.5 * h
    ref = NC.sphere_points(2000, r + delta)
    # a: every point of the mesh surface is within a of the sphere of radius r.  Its vertices are within
    # eb = sphere_error_bound (the extraction's own tested bound).  A surface point x = sum l_i v_i of a face
    # (l_i >= 0, sum 1) has |x| <= max |v_i| <= r + eb, and |x|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2
    # >= (r - eb)^2 - L^2 / 3 (sum_{i<j} l_i l_j <= 1/3); a face lies in one cell, so L <= sqrt(3) h and the chord's
    # sagitta gives |x| >= sqrt((r - eb)^2 - h^2).
    eb = MC.sphere_error_bound(r, h)
    a = r - math.sqrt((r - eb) ** 2 - h * h)
    assert a >= eb
    # c_ref: the covering radius of the reference points on their sphere, by float64 brute force over a latitude-
    # longitude probe grid of steps dt, dp.  Every point of the sphere is within R sqrt(dt^2 + dp^2) / 2 of a probe
    # (ds^2 = dt^2 + sin^2 t dp^2 <= dt^2 + dp^2, and a chord is shorter than its arc), so c_ref <= the largest
    # probe-to-reference distance + that.
    nt, npi = 120, 240
    R = r + delta
    t = (torch.arange(nt, dtype=torch.float64) + 0.5) * (math.pi / nt)
    p = torch.arange(npi, dtype=torch.float64) * (2 * math.pi / npi)
    tt, pp = torch.meshgrid(t, p, indexing="ij")
    probes = R * torch.stack([torch.sin(tt) * torch.cos(pp), torch.sin(tt) * torch.sin(pp), torch.cos(tt)], -1)
    worst = max(float(torch.cdist(chunk, ref.double()).min(dim=1).values.max())
                for chunk in probes.reshape(-1, 3).split(4096))
    c_ref = worst + R * math.hypot(math.pi / nt, 2 * math.pi / npi) / 2 + 4 * float(np.spacing(np.float32(R)))
    c_samples = (2.0 / 3.0) * spacing  # the sampler's covering radius, by its construction
    return dict(V=V, F=F, r=r, h=h, delta=delta, spacing=spacing, ref=ref, a=a, c_ref=c_ref, c_samples=c_samples)


def test_score_of_an_offset_sphere(offset_sphere):
    """Mesh of radius r against points on the sphere of radius r + delta.  A sample x (|x| within a of r) is at least
    delta - a from every reference point (their radii differ by that), and its radial projection onto the reference
    sphere is within delta + a of it and within c_ref of a reference point: accuracy in [delta - a, delta + a +
    c_ref].  A reference point y is at least delta - a from every sample; the ray to y meets the closed mesh at a point
    within delta + a of y, and a sample lies within c_samples = (2/3) spacing of that: completeness in [delta - a,
    delta + a + c_samples]."""
    o = offset_sphere
    sc = M.score_mesh(o["V"], o["F"], o["ref"], spacing=o["spacing"])
    lo = o["delta"] - o["a"]
    print(f"accuracy {sc['accuracy']:.5f} in [{lo:.5f}, {o['delta'] + o['a'] + o['c_ref']:.5f}]; completeness "
          f"{sc['completeness']:.5f} in [{lo:.5f}, {o['delta'] + o['a'] + o['c_samples']:.5f}]")
    assert lo > 0
    assert lo <= sc["accuracy"] <= o["delta"] + o["a"] + o["c_ref"]
    assert lo <= sc["completeness"] <= o["delta"] + o["a"] + o["c_samples"]
    assert sc["chamfer"] == 0.5 * (sc["accuracy"] + sc["completeness"])
    assert float(sc["d"].min()) >= lo * (1 - 1e-6) and float(sc["e"].min()) >= lo * (1 - 1e-6)
    assert float(sc["d"].max()) <= (o["delta"] + o["a"] + o["c_ref"]) * (1 + 1e-6)
    assert float(sc["e"].max()) <= (o["delta"] + o["a"] + o["c_samples"]) * (1 + 1e-6)
    assert sc["d"].shape[0] == sc["n_samples"] and sc["e"].shape[0] == sc["n_reference"] == 2000


def test_score_clamp_thresholds_and_bounds(offset_sphere):
    o = offset_sphere
    lo, hi = o["delta"] - o["a"], o["delta"] + o["a"] + max(o["c_ref"], o["c_samples"])
    # the clamp below every distance: both means are the clamp itself
    clamp = 0.5 * lo
    sc = M.score_mesh(o["V"], o["F"], o["ref"], spacing=o["spacing"], max_dist=clamp,
                      thresholds=(0.999 * lo, 1.001 * hi))
    c32 = float(np.float32(clamp))
    assert math.isclose(sc["accuracy"], c32, rel_tol=1e-12) and math.isclose(sc["completeness"], c32, rel_tol=1e-12)
    assert sc["precision"] == [1.0, 1.0] and sc["recall"] == [1.0, 1.0]  # clamped distances are below both
    # thresholds on both sides of delta, unclamped
    sc = M.score_mesh(o["V"], o["F"], o["ref"], spacing=o["spacing"], thresholds=(0.999 * lo, 1.001 * hi))
    assert sc["precision"] == [0.0, 1.0] and sc["recall"] == [0.0, 1.0] and sc["fscore"] == [0.0, 1.0]
    # a threshold inside the range: the definitions, from the returned distances
    tau = float(sc["d"].median())
    mid = M.score_mesh(o["V"], o["F"], o["ref"], spacing=o["spacing"], thresholds=(tau,))
    w = mid["weights"].double()
    p = float((w * (mid["d"] <= tau).double()).sum() / w.sum())
    r = float((mid["e"] <= tau).double().mean())
    assert mid["precision"] == [p] and mid["recall"] == [r] and 0 < p < 1
    assert math.isclose(mid["fscore"][0], 2 * p * r / (p + r) if p + r else 0.0, rel_tol=1e-12)
    # bounds crop both sets: the upper half space
    box = ((-1.0, -1.0, 0.0), (1.0, 1.0, 1.0))
    S, _, _ = M.sample_mesh(o["V"], o["F"], o["spacing"])
    half = M.score_mesh(o["V"], o["F"], o["ref"], spacing=o["spacing"], bounds=box)
    assert half["n_samples"] == int((S[:, 2] >= 0).sum()) < S.shape[0]
    assert half["n_reference"] == int((o["ref"][:, 2] >= 0).sum()) < 2000
    assert float(half["samples"][:, 2].min()) >= 0 and half["d"].shape[0] == half["n_samples"]
    with pytest.raises(ValueError, match="nothing to compare"):
        M.score_mesh(o["V"], o["F"], o["ref"], spacing=o["spacing"], bounds=((5.0, 5.0, 5.0), (6.0, 6.0, 6.0)))


# ---------------------------------------------------------------------------------------- 5. init
@pytest.mark.parametrize("tag", ["raw", "fix"])
def test_knn_mean_dist_through_the_twin_matches_the_reference(tag):
    """scene.knn_mean_dist(points, 3, device="cpu") (the grid's twins) against the reference's own sklearn distances of
    the golden point cloud, within the relative 1e-6 of test 1; the default route is untouched."""
    from gstex_amd.scene import knn_mean_dist

    with np.load(GOLDEN) as z:
        xyz, want = z[f"lod_{tag}_xyz"], z[f"lod_{tag}_knn_dist"].astype(np.float64).mean(axis=-1)
    got = knn_mean_dist(xyz, 3, device="cpu")
    assert got.dtype == np.float32 and got.shape == (xyz.shape[0],)
    assert np.abs(got / want - 1).max() <= 1e-6
    assert np.abs(knn_mean_dist(xyz, 3) / want - 1).max() <= 1e-6
    dev = N.knn_mean_dist_device(torch.from_numpy(xyz), 3)
    assert torch.equal(dev, torch.from_numpy(got))


def test_scene_from_point_cloud_knn_route(tmp_path):
    from gstex_amd.init import scene_from_point_cloud
    from gstex_amd.ply import write_ply

    g = torch.Generator().manual_seed(8)
    xyz = torch.rand((300, 3), generator=g).double().numpy()
    rgb = torch.randint(0, 256, (300, 3), generator=g).to(torch.uint8).numpy()
    path = tmp_path / "cloud.ply"
    write_ply(path, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "red": rgb[:, 0], "green": rgb[:, 1],
                     "blue": rgb[:, 2]}, binary=True)
    a, b = scene_from_point_cloud(path), scene_from_point_cloud(path, knn_device="cpu")
    assert torch.allclose(a.log_scales, b.log_scales, rtol=1e-6, atol=0.0)
    assert torch.equal(a.means, b.means) and torch.equal(a.quats, b.quats)


# ---------------------------------------------------------------------------------------- 6. C ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


_BUF = (ctypes.c_float * 8)()  # stands for a device pointer: null-checked only, never read before a launch


def _status(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, _lib.last_error()


def _grid(h=0.5, dims=(4, 4, 4)):
    return _lib.GstexNnGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), h, *dims)


def test_nn_entry_points_reject_bad_arguments(lib):
    p = ctypes.addressof(_BUF)
    for name, tail in (("gstex_nn_grid_count", (p, p, None)), ("gstex_nn_grid_place", (p, p, p, p, None))):
        rc, msg = _status(lib, name, None, 10, *tail)
        assert rc == 1 and f"{name}: null grid" in msg
        for h in (0.0, -1.0, float("nan"), float("inf")):
            rc, msg = _status(lib, name, ctypes.byref(_grid(h=h)), 10, *tail)
            assert rc == 1 and "cell_size must be finite and > 0" in msg, h
        rc, msg = _status(lib, name, ctypes.byref(_grid(dims=(4, 0, 4))), 10, *tail)
        assert rc == 1 and "every dim must be >= 1" in msg
        for dims in ((4097, 1, 1), (512, 512, 512)):
            rc, msg = _status(lib, name, ctypes.byref(_grid(dims=dims)), 10, *tail)
            assert rc == 3 and "too many cells" in msg, dims
        for n in (-1, 1 << 31):
            rc, msg = _status(lib, name, ctypes.byref(_grid()), n, *tail)
            assert rc == 1 and "n must be in [0, 2^31)" in msg, n
        nulls = (None,) + tail[1:] if name.endswith("count") else (p, None) + tail[2:]
        rc, msg = _status(lib, name, ctypes.byref(_grid()), 10, *nulls)
        assert rc == 1 and "null pointer" in msg
    rc, msg = _status(lib, "gstex_nn_grid_place", ctypes.byref(_grid()), 10, p, p, p, p + 4, None)
    assert rc == 1 and "misaligned" in msg


def _query_args(**kw):
    p = ctypes.addressof(_BUF)
    base = dict(grid=_grid(), n_points=10, cell_start=p, records=p, n_queries=10, queries=p, k=1, exclude_self=0,
                max_radius=float("inf"), d2=p, index=p)
    base.update(kw)
    return _lib.GstexNnQueryArgs(**base)


def test_nn_query_rejects_bad_arguments(lib):
    rc, msg = _status(lib, "gstex_nn_query", None, None)
    assert rc == 1 and "null args" in msg
    for k in (0, -1, 9):
        rc, msg = _status(lib, "gstex_nn_query", ctypes.byref(_query_args(k=k)), None)
        assert rc == 1 and "k must be in [1, 8]" in msg, k
    for r in (-1.0, float("nan")):
        rc, msg = _status(lib, "gstex_nn_query", ctypes.byref(_query_args(max_radius=r)), None)
        assert rc == 1 and "max_radius" in msg, r
    for field in ("cell_start", "records", "queries", "d2", "index"):
        rc, msg = _status(lib, "gstex_nn_query", ctypes.byref(_query_args(**{field: None})), None)
        assert rc == 1 and "null pointer" in msg, field
    rc, msg = _status(lib, "gstex_nn_query", ctypes.byref(_query_args(grid=_grid(h=0.0))), None)
    assert rc == 1 and "cell_size" in msg
    rc, msg = _status(lib, "gstex_nn_query", ctypes.byref(_query_args(grid=_grid(dims=(1024, 1024, 65)))), None)
    assert rc == 3 and "too many cells" in msg
    rc, msg = _status(lib, "gstex_nn_query", ctypes.byref(_query_args(n_points=1 << 31)), None)
    assert rc == 1 and "2^31" in msg
    assert _status(lib, "gstex_nn_query", ctypes.byref(_query_args(n_queries=0, queries=None, d2=None, index=None)),
                   None)[0] == 0  # empty: no launch


def _sample_args(**kw):
    p = ctypes.addressof(_BUF)
    base = dict(n_vertices=3, n_faces=1, vertices=p, faces=p, spacing=0.5, count=p, stats=p, offsets=p, n_samples=4,
                samples=p, weights=p, face_of=p)
    base.update(kw)
    return _lib.GstexMeshSampleArgs(**base)


def test_mesh_sample_rejects_bad_arguments(lib):
    for name in ("gstex_mesh_sample_mark", "gstex_mesh_sample_emit"):
        rc, msg = _status(lib, name, None, None)
        assert rc == 1 and f"{name}: null args" in msg
        for s in (0.0, -2.0, float("nan")):
            rc, msg = _status(lib, name, ctypes.byref(_sample_args(spacing=s)), None)
            assert rc == 1 and "spacing must be finite and > 0" in msg, s
        rc, msg = _status(lib, name, ctypes.byref(_sample_args(n_faces=-1)), None)
        assert rc == 1 and "invalid sizes" in msg
        rc, msg = _status(lib, name, ctypes.byref(_sample_args(vertices=None)), None)
        assert rc == 1 and "null pointer" in msg
    rc, msg = _status(lib, "gstex_mesh_sample_mark", ctypes.byref(_sample_args(stats=None)), None)
    assert rc == 1 and "null pointer (count / stats)" in msg
    rc, msg = _status(lib, "gstex_mesh_sample_emit", ctypes.byref(_sample_args(offsets=None)), None)
    assert rc == 1 and "null pointer (offsets" in msg
    rc, msg = _status(lib, "gstex_mesh_sample_emit", ctypes.byref(_sample_args(n_samples=1 << 31)), None)
    assert rc == 1 and "n_samples" in msg
    assert _status(lib, "gstex_mesh_sample_emit", ctypes.byref(_sample_args(n_samples=0, samples=None)), None)[0] == 0


def test_new_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors of the new structs have the header's sizes and field offsets (gcc on the header)."""
    import subprocess

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    structs = {"gstex_nn_grid": _lib.GstexNnGrid, "gstex_nn_query_args": _lib.GstexNnQueryArgs,
               "gstex_mesh_sample_args": _lib.GstexMeshSampleArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", header, str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[f"{cname} size"]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got[f"{cname} {f[0]}"]) == getattr(cls, f[0]).offset, f"{cname}.{f[0]}"
