"""The splat clustering without a GPU: the eager twins of gstex_amd.cluster against a restatement of the reference's
sequential loop, scikit-learn on a precomputed distance matrix and the reference's own float64 results
(tests/golden/cluster.npz), the kernels' host restatement against the brute-force twin, the reports, the PLY route and
the C ABI's declarations and argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import cluster_cases as CC
from gstex_amd import _lib
from gstex_amd import cluster as C

U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "cluster.npz")
SYMBOLS = ("gstex_cluster_shapes", "gstex_cluster_degree", "gstex_cluster_link", "gstex_cluster_roots",
           "gstex_cluster_assign", "gstex_cluster_pair_w2")


def _splats(c):
    return c["means"], c["scales"], c["quats"]


@pytest.fixture(scope="module")
def matrices():
    """Per case: the dense w2 matrix of the twin's distance (computed once, shared, not modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            c = CC.cases()[name]
            n = c["means"].shape[0]
            i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
            w2, d2, tr = C.wasserstein2_eager(*_splats(c), i.reshape(-1), j.reshape(-1))
            cache[name] = tuple(t.reshape(n, n) for t in (w2, d2, tr))
        return cache[name]

    return get


def _twin(name, min_pts):
    c = CC.cases()[name]
    return C.dbscan_eager(*_splats(c), c["eps"], min_pts)


# ---------------------------------------------------------------------------------------- 1. the distance
def test_distance_contract_properties(matrices):
    """w2 = d2 + tr with tr >= 0, so w2 >= d2 in fp32 (what lets the grid prune on d2); the matrix is symmetric bit
    for bit; and against float64 of the same formula the fp32 value is within 16 u (d2 + 2 (T_i + T_j))."""
    for name in ("two_blobs_noise", "n=65", "orientation_splits"):
        c = CC.cases()[name]
        w2, d2, tr = matrices(name)
        assert bool((tr >= 0).all()) and bool((w2 >= d2).all())
        assert torch.equal(w2.view(torch.int32), w2.t().contiguous().view(torch.int32)), name
        a, b, T = C.shapes_eager(c["scales"].double(), c["quats"].double())
        n = T.shape[0]
        i, j = (t.reshape(-1) for t in torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij"))
        d64 = C._d2_eager(c["means"].double()[i], c["means"].double()[j])
        w64 = d64 + C._trace_eager(a[i], b[i], T[i], a[j], b[j], T[j])
        bound = 16 * U * (d64 + 2 * (T[i] + T[j]))
        assert bool(((w2.reshape(-1).double() - w64).abs() <= bound).all()), name


def test_orientation_splits_is_decided_by_the_trace_term(matrices):
    c = CC.cases()["orientation_splits"]
    w2, d2, tr = matrices("orientation_splits")
    same = c["normal_x"][:, None] == c["normal_x"][None, :]
    assert float(d2.max()) < 1e-5  # a Euclidean DBSCAN sees one blob
    assert float(tr[same].max()) < 1e-6 and abs(float(tr[~same].min()) - 0.02) < 1e-6 and float(tr[~same].max()) < 0.0201
    r = _twin("orientation_splits", 5)
    assert r.n_clusters == 2
    assert len(set(r.labels[c["normal_x"]].tolist())) == 1 and len(set(r.labels[~c["normal_x"]].tolist())) == 1
    assert int(r.labels[c["normal_x"]][0]) != int(r.labels[~c["normal_x"]][0])


# ---------------------------------------------------------------------------------------- 2. the labelling
def _sequential(adj, min_pts):
    """The reference's BallQueryDBSCAN.fit restated on exact neighbour lists: -2 unclassified, -1 noise, ids from 1;
    a cluster is expanded to the end before the next starts, noise marks are overwritten."""
    n = adj.shape[0]
    nbrs = [np.nonzero(adj[i])[0].tolist() for i in range(n)]
    labels = [-2] * n
    cid = 0
    for p in range(n):
        if labels[p] != -2:
            continue
        if len(nbrs[p]) < min_pts:
            labels[p] = -1
            continue
        cid += 1
        labels[p] = cid
        queue, queued = list(nbrs[p]), set(nbrs[p])
        k = 0
        while k < len(queue):
            q = queue[k]
            if labels[q] in (-2, -1):
                labels[q] = cid
                if len(nbrs[q]) >= min_pts:
                    for r in nbrs[q]:
                        if labels[r] in (-2, -1) and r not in queued:
                            queue.append(r)
                            queued.add(r)
            k += 1
    return np.array(labels)


RUNS = [(name, m) for name, c in CC.cases().items() for m in c["min_pts"]]


@pytest.mark.parametrize("name,min_pts", RUNS)
def test_twin_equals_the_sequential_loop_and_sklearn(matrices, name, min_pts):
    c = CC.cases()[name]
    w2 = matrices(name)[0]
    n = w2.shape[0]
    adj = (w2 <= np.float32(c["eps"])).numpy() & ~np.eye(n, dtype=bool)
    r = _twin(name, min_pts)
    assert r.labels.dtype == torch.int32 and r.degree.dtype == torch.int32 and r.core.dtype == torch.bool
    assert (r.degree.numpy() == adj.sum(1)).all() and (r.core.numpy() == (adj.sum(1) >= min_pts)).all()
    want = _sequential(adj, min_pts)
    assert (r.labels.numpy() == want).all(), name
    assert r.n_clusters == max(int(want.max()), 0)
    sk = pytest.importorskip("sklearn.cluster")
    D = np.where(adj | np.eye(n, dtype=bool), 0.0, 1.0)  # the neighbour relation itself, self included
    fit = sk.DBSCAN(eps=0.5, min_samples=min_pts + 1, metric="precomputed").fit(D)
    assert sorted(fit.core_sample_indices_.tolist()) == np.nonzero(r.core.numpy())[0].tolist()
    lab = r.labels.numpy()
    assert ((fit.labels_ == -1) == (lab == -1)).all()
    cores = r.core.numpy()
    pairs = set(zip(lab[cores].tolist(), fit.labels_[cores].tolist()))
    assert len(pairs) == r.n_clusters == len({a for a, _ in pairs}) == len({b for _, b in pairs})


def test_cases_are_what_they_claim():
    r = _twin("two_blobs_noise", 5)
    assert r.n_clusters >= 2 and int((r.labels == -1).sum()) >= 30 and bool((~r.core & (r.labels > 0)).any())
    r = _twin("chain", 2)
    assert r.n_clusters == 1 and bool((r.labels == 1).all()) and sorted(r.degree.tolist())[:3] == [1, 1, 2]
    r = _twin("chain", 3)
    assert r.n_clusters == 0 and bool((r.labels == -1).all())
    c = CC.cases()["contested_border"]
    r = _twin("contested_border", 3)
    d2 = ((c["means"][10] - c["means"]) ** 2).sum(-1)
    assert r.labels.tolist() == [1] * 5 + [2] * 5 + [1] and not bool(r.core[10])
    assert float(d2[5]) < float(d2[0]) <= 1.0 and int(r.labels[5]) == 2  # the nearer core is the higher id's
    c = CC.cases()["ties"]
    r = _twin("ties", 6)
    inner = ((c["means"] >= 1) & (c["means"] <= 3)).all(1)
    assert bool((r.degree[inner] == 6).all()) and bool((r.core == inner).all()) and r.n_clusters == 1
    assert int((r.labels == 1).sum()) == 27 + 54 and _twin("ties", 7).n_clusters == 0
    r1, r2 = _twin("duplicates", 1), _twin("duplicates", 2)
    assert sorted(r1.degree.tolist()) == [0] * 10 + [1] * 20 + [2] * 30
    assert r1.n_clusters == 20 and r2.n_clusters == 10 and int((r2.labels == -1).sum()) == 30
    r = _twin("single", 10)
    assert r.labels.tolist() == [-1] and r.degree.tolist() == [0] and r.n_clusters == 0
    r = _twin("n=4001", 10)
    assert r.n_clusters > 10 and bool((r.labels == -1).any()) and bool((~r.core & (r.labels > 0)).any())
    from gstex_amd import neighbors as N

    big = CC.cases()["n=4001"]
    one, default, fine = big["cell_sizes"]
    lo, hi = big["means"].min(0).values.numpy(), big["means"].max(0).values.numpy()
    assert N.grid_dims(lo, hi, one) == (1, 1, 1) and default is None and fine == math.sqrt(big["eps"]) / 20
    dims = N.grid_dims(lo, hi, np.float32(fine))
    assert N._fits(dims) and min(dims) > 300  # the walk crosses 20 rings of cells and more
    e = C.dbscan(torch.zeros((0, 3)), torch.zeros((0, 2)), torch.zeros((0, 4)), 0.1, 3)
    assert e.labels.shape == (0,) and e.n_clusters == 0
    for bad in (dict(eps=-1.0, min_pts=3), dict(eps=float("nan"), min_pts=3), dict(eps=0.1, min_pts=0)):
        with pytest.raises(ValueError):
            C.dbscan(*_splats(CC.cases()["n=65"]), **bad)


@pytest.mark.parametrize("name,min_pts,cell_size", CC.runs(small_only=True) + [("n=65", 10, 4.0), ("n=65", 10, 0.03),
                                                                              ("ties", 6, 0.3), ("chain", 2, 7.0)])
def test_host_restatement_of_the_kernels_equals_the_twin(name, min_pts, cell_size):
    """The ring walk with its stop test, the union-find and the second walk, on the default cell and on cells far above
    and far below the radius."""
    c = CC.cases()[name]
    want = _twin(name, min_pts)
    got = C.dbscan_walk_eager(*_splats(c), c["eps"], min_pts, cell_size=cell_size)
    assert torch.equal(got.labels, want.labels) and torch.equal(got.degree, want.degree)
    assert torch.equal(got.core, want.core) and got.n_clusters == want.n_clusters


def test_default_cell_ends_the_walk_after_one_ring():
    c = CC.cases()["n=65"]
    g = C.cluster_grid(c["means"], np.float32(c["eps"]))
    lb = np.float32(np.float32(1.0) * np.float32(g.cell_size)) * np.float32(1.0 - 2.0 ** -10)
    assert lb * lb >= np.float32(c["eps"]) and g.cell_size < math.sqrt(c["eps"]) * 1.01
    tiny = C.cluster_grid(c["means"], 1e-12)  # enlarged to fit the cell limits instead of refused
    assert max(tiny.dims) <= _lib.NN_MAX_AXIS_CELLS and tiny.cell_size > 1e-6
    assert C.cluster_grid(c["means"], 0.0).cell_size > 0


# ---------------------------------------------------------------------------------------- 3. the reference's results
def test_golden_distances_and_labels():
    """tests/golden/cluster.npz (make_cluster_golden.py): per stored pair the fp32 twin is within
    gap + 16 u (d2 + 2 (T_i + T_j)) of the reference's float64 W^2, gap being the generator's measured difference
    between the closed form in float64 and the reference; and the labels equal the reference's."""
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    means = torch.from_numpy(g["means"]).float()
    scales = torch.exp(torch.from_numpy(g["log_scales"])[:, :2]).float()
    q = torch.from_numpy(g["quats"])
    quats = (q / q.norm(dim=1, keepdim=True)).float()
    eps, min_pts, gap = float(g["eps"]), int(g["min_pts"]), float(g["gap"])
    assert 250 <= means.shape[0] <= 350 and os.path.getsize(GOLDEN) < 100 * 1024
    assert eps * float(g["multiplier"]) >= math.sqrt(eps)
    assert float(np.abs(g["pair_w2"] - eps).min()) >= 10 * gap
    i, j = torch.from_numpy(g["pair_i"].astype(np.int64)), torch.from_numpy(g["pair_j"].astype(np.int64))
    w2, d2, _ = C.wasserstein2_eager(means, scales, quats, i, j)
    T = (scales.double() ** 2).sum(1)
    bound = gap + 16 * U * (d2.double() + 2 * (T[i] + T[j]))
    err = (w2.double() - torch.from_numpy(g["pair_w2"])).abs()
    print(f"golden: gap {gap:.3e}, max error {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all())
    r = C.dbscan_eager(means, scales, quats, eps, min_pts)
    assert (r.labels.numpy() == g["labels"]).all() and r.n_clusters == int(g["labels"].max()) >= 3


# ---------------------------------------------------------------------------------------- 4. reports and files
def test_cluster_summary_keys_and_values():
    labels = torch.tensor([1, 1, -1, 2, 2, 2, -1, 3], dtype=torch.int32)
    s = C.cluster_summary(labels)
    assert list(s) == ["n_clusters", "n_noise_points", "n_total_points", "noise_ratio", "cluster_sizes",
                       "avg_cluster_size", "largest_cluster_size", "smallest_cluster_size"]
    assert s == {"n_clusters": 3, "n_noise_points": 2, "n_total_points": 8, "noise_ratio": 0.25,
                 "cluster_sizes": [2, 3, 1], "avg_cluster_size": 2.0, "largest_cluster_size": 3,
                 "smallest_cluster_size": 1}
    s = C.cluster_summary(torch.full((4,), -1, dtype=torch.int32))
    assert s["n_clusters"] == 0 and s["cluster_sizes"] == [] and s["avg_cluster_size"] == 0 and s["noise_ratio"] == 1.0


def test_cluster_report(tmp_path):
    c = CC.cases()["two_blobs_noise"]
    r = _twin("two_blobs_noise", 5)
    op = torch.rand((c["means"].shape[0], 1), generator=torch.Generator().manual_seed(3))
    st = C.cluster_report(tmp_path / "report.txt", r, c["means"], op, c["scales"])
    text = (tmp_path / "report.txt").read_text()
    assert f"Number of clusters: {r.n_clusters}" in text and text.count("  Size: ") == r.n_clusters
    for k in range(r.n_clusters):  # against a loop over the clusters
        m = r.labels == k + 1
        assert int(st["size"][k]) == int(m.sum())
        assert np.allclose(st["center"][k], c["means"][m].double().mean(0).numpy(), rtol=1e-12, atol=1e-15)
        assert np.array_equal(st["lo"][k], c["means"][m].double().min(0).values.numpy())
        assert np.array_equal(st["hi"][k], c["means"][m].double().max(0).values.numpy())
        assert math.isclose(st["opacity"][k], float(op[m].double().mean()), rel_tol=1e-12)
        assert np.allclose(st["scale"][k], c["scales"][m].double().mean(0).numpy(), rtol=1e-12)
        assert f"Cluster {k + 1}:\n  Size: {int(m.sum())} points" in text


def test_label_colors_are_a_fixed_function_of_the_label():
    lab = torch.tensor([-1, 1, 2, 3, 2, 1], dtype=torch.int32)
    torch.manual_seed(0)
    a = C.label_colors(lab)
    torch.manual_seed(1)
    np.random.seed(5)
    b = C.label_colors(lab)
    assert a.dtype == np.uint8 and a.shape == (6, 3) and (a == b).all()
    assert (a[0] == 128).all() and (a[1] == a[5]).all() and (a[2] == a[4]).all()
    assert len({tuple(v) for v in a[1:4].tolist()}) == 3
    assert a[1].tolist() == [(2654435761 >> s) & 255 for s in (24, 16, 8)]


def test_cluster_ply_round_trip(tmp_path):
    from gstex_amd.export import cluster_ply
    from gstex_amd.init import scene_from_2dgs_ply
    from gstex_amd.ply import read_ply

    src = os.path.join(HERE, "golden", "init_2dgs.ply")
    scene = scene_from_2dgs_ply(src, sh_degree=3)
    means, scales, quats, _ = scene.activated()
    d = torch.cdist(means.double(), means.double())
    eps = float(d.topk(4, dim=1, largest=False).values[:, 3].median()) ** 2  # the median third neighbour's distance
    res = cluster_ply(src, tmp_path / "out.ply", eps, 3, report=tmp_path / "out.txt", device="cpu")
    want = C.dbscan_eager(means, scales[:, :2], quats, eps, 3)
    assert torch.equal(res.labels, want.labels) and res.n_clusters == want.n_clusters
    cols = read_ply(tmp_path / "out.ply")
    assert list(cols) == ["x", "y", "z", "label", "red", "green", "blue"]
    assert cols["label"].dtype == np.int32 and (cols["label"] == want.labels.numpy()).all()
    assert np.array_equal(np.stack([cols["x"], cols["y"], cols["z"]], 1), means.numpy())
    assert (np.stack([cols["red"], cols["green"], cols["blue"]], 1) == C.label_colors(want.labels)).all()
    assert "Ball Query DBSCAN Clustering Results" in (tmp_path / "out.txt").read_text()


# ---------------------------------------------------------------------------------------- 5. C ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "gstex_hip.h")).read()
    assert re.search(r"#define GSTEX_ABI_VERSION 19\b", header) and _lib.ABI_VERSION == 19
    assert lib.gstex_abi_version() == 19
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert "cluster.hip" in open(os.path.join(ROOT, "gstex_amd", "csrc", "Makefile")).read()


_BUF = (ctypes.c_float * 16)()  # stands for a device pointer: null- and alignment-checked only, never read


def _status(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, _lib.last_error()


def _args(**kw):
    p = ctypes.addressof(_BUF)
    base = dict(grid=_lib.GstexNnGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), 0.5, 4, 4, 4), n=10, cell_start=p, records=p,
                shapes=p, eps=0.25, min_pts=3, degree=p, parent=p, offsets=p, labels=p)
    base.update(kw)
    return _lib.GstexClusterArgs(**base)


def test_walk_entry_points_reject_bad_arguments(lib):
    for name in ("gstex_cluster_degree", "gstex_cluster_link", "gstex_cluster_assign"):
        rc, msg = _status(lib, name, None, None)
        assert rc == 1 and f"{name}: null args" in msg
        for eps in (-0.5, float("nan"), float("inf")):
            rc, msg = _status(lib, name, ctypes.byref(_args(eps=eps)), None)
            assert rc == 1 and "eps must be finite and >= 0" in msg, eps
        for m in (0, -2):
            rc, msg = _status(lib, name, ctypes.byref(_args(min_pts=m)), None)
            assert rc == 1 and "min_pts must be >= 1" in msg
        for n in (-1, 1 << 31):
            rc, msg = _status(lib, name, ctypes.byref(_args(n=n)), None)
            assert rc == 1 and "n must be in [0, 2^31)" in msg
        for field in ("cell_start", "records", "shapes", "degree", "parent"):
            rc, msg = _status(lib, name, ctypes.byref(_args(**{field: None})), None)
            assert rc == 1 and "null pointer" in msg, field
        p = ctypes.addressof(_BUF)
        for field, off in (("records", 4), ("shapes", 8), ("degree", 2)):
            rc, msg = _status(lib, name, ctypes.byref(_args(**{field: p + off})), None)
            assert rc == 1 and "misaligned" in msg, field
        bad = _lib.GstexNnGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), 0.0, 4, 4, 4)
        rc, msg = _status(lib, name, ctypes.byref(_args(grid=bad)), None)
        assert rc == 1 and "cell_size" in msg
        big = _lib.GstexNnGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), 0.5, 4097, 1, 1)
        rc, msg = _status(lib, name, ctypes.byref(_args(grid=big)), None)
        assert rc == 3 and "too many cells" in msg
        assert _status(lib, name, ctypes.byref(_args(n=0, records=None, shapes=None, degree=None, parent=None)),
                       None)[0] == 0  # empty: no launch
    for field in ("offsets", "labels"):
        rc, msg = _status(lib, "gstex_cluster_assign", ctypes.byref(_args(**{field: None})), None)
        assert rc == 1 and "null pointer (offsets / labels)" in msg


def test_other_entry_points_reject_bad_arguments(lib):
    p = ctypes.addressof(_BUF)
    for n in (-1, 1 << 31):
        assert _status(lib, "gstex_cluster_shapes", n, p, p, 2, p, p, None)[0] == 1
        assert _status(lib, "gstex_cluster_roots", n, 3, p, p, p, None)[0] == 1
        assert _status(lib, "gstex_cluster_pair_w2", n, p, p, 2, p, 4, p, p, p, p, None)[0] == 1
    rc, msg = _status(lib, "gstex_cluster_shapes", 10, p, p, 1, p, p, None)
    assert rc == 1 and "scale_cols must be >= 2" in msg
    for tail in ((None, p, 2, p, p), (p, None, 2, p, p), (p, p, 2, None, p), (p, p, 2, p, None)):
        rc, msg = _status(lib, "gstex_cluster_shapes", 10, *tail, None)
        assert rc == 1 and "null pointer" in msg
    rc, msg = _status(lib, "gstex_cluster_shapes", 10, p, p, 2, p, p + 4, None)
    assert rc == 1 and "misaligned" in msg
    assert _status(lib, "gstex_cluster_shapes", 0, None, None, 2, None, None, None)[0] == 0
    rc, msg = _status(lib, "gstex_cluster_roots", 10, 0, p, p, p, None)
    assert rc == 1 and "min_pts must be >= 1" in msg
    for tail in ((None, p, p), (p, None, p), (p, p, None)):
        rc, msg = _status(lib, "gstex_cluster_roots", 10, 3, *tail, None)
        assert rc == 1 and "null pointer" in msg
    assert _status(lib, "gstex_cluster_roots", 10, 3, p, p + 2, p, None)[0] == 1
    assert _status(lib, "gstex_cluster_roots", 0, 3, None, None, None, None)[0] == 0
    for np_ in (-1, 1 << 30):
        rc, msg = _status(lib, "gstex_cluster_pair_w2", 10, p, p, 2, p, np_, p, p, p, p, None)
        assert rc == 1 and "n_pairs" in msg
    for k in (1, 2, 4, 6, 7, 8, 9):  # means, scales, quats, pairs, d2, tr, w2
        args = [10, p, p, 2, p, 4, p, p, p, p]
        args[k] = None
        rc, msg = _status(lib, "gstex_cluster_pair_w2", *args, None)
        assert rc == 1 and "null pointer" in msg, k
    assert _status(lib, "gstex_cluster_pair_w2", 10, p, p, 2, p, 0, None, None, None, None, None)[0] == 0


def test_struct_layout_matches_header(tmp_path):
    import subprocess

    cls, cname = _lib.GstexClusterArgs, "gstex_cluster_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
