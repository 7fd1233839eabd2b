"""The nearest-neighbour and mesh-sampler kernels (gstex_amd/csrc/neighbors.hip) against the eager twins of
gstex_amd.neighbors run on the CPU, bit for bit on every output the contract orders; the guard behind the caller-sized
sampler outputs; score_mesh, the initialisation's neighbour distances and GStexTrainer.score_mesh on the device."""
import math

import numpy as np
import pytest
import torch

import mesh_cases as MC
import neighbor_cases as NC
from gstex_amd import mesh as M
from gstex_amd import neighbors as N

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    for a, b, name in zip(got, want, ("d2", "index")):
        a, b = _bits(a), _bits(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} of {a.numel()} values"


def _cell_sets(grid):
    """cell_start and, per cell, its records sorted by index (the order inside a cell is free)."""
    start = grid.cell_start.cpu()
    rec = grid.records.cpu()
    idx = rec[:, 3].contiguous().view(torch.int32).long()
    cell = torch.searchsorted(start[1:].long().contiguous(), torch.arange(rec.shape[0]), right=True)
    order = torch.argsort(cell * rec.shape[0] + idx)
    return start, rec[order].contiguous().view(torch.int32)


def _check_grid(points, cell_size, what):
    dev, cpu = N.PointGrid(points.to(DEV), cell_size=cell_size), N.PointGrid(points, cell_size=cell_size)
    assert dev.dims == cpu.dims and dev.origin == cpu.origin and dev.cell_size == cpu.cell_size, what
    (s_dev, r_dev), (s_cpu, r_cpu) = _cell_sets(dev), _cell_sets(cpu)
    assert torch.equal(s_dev, s_cpu), f"{what}: cell_start differs"
    assert torch.equal(r_dev, r_cpu), f"{what}: a cell's record set differs"
    return dev, cpu


# ---------------------------------------------------------------------------------------- 1. kernels vs twins
@pytest.mark.parametrize("name", list(NC.grid_cases()))
def test_grid_cases_match_twin(name):
    c = NC.grid_cases()[name]
    dev, cpu = _check_grid(c["points"], c["cell_size"], name)
    kw = dict(k=c["k"], exclude_self=c["exclude_self"], max_radius=c["max_radius"])
    got = dev.query(c["queries"].to(DEV), **kw)
    _same(got, cpu.query(c["queries"], **kw), name)


@pytest.fixture(scope="module")
def random_grids():
    P, Q = NC.random_case()
    dev, cpu = _check_grid(P, None, "random 5000")
    return P, Q, dev, cpu


@pytest.mark.parametrize("k", [1, 3, 8])
def test_random_case_matches_twin(random_grids, k):
    """5,000 points, 4,001 queries: plain, with max_radius (about the third neighbour's distance, so rows are partly
    padded), and the point set against itself with exclude_self, also under a radius."""
    P, Q, dev, cpu = random_grids
    assert Q.shape[0] % 64 != 0 and Q.shape[0] % 256 != 0
    _same(dev.query(Q.to(DEV), k=k), cpu.query(Q, k=k), f"k={k}")
    radius = 0.045
    got = dev.query(Q.to(DEV), k=k, max_radius=radius)
    want = cpu.query(Q, k=k, max_radius=radius)
    if k > 1:
        assert bool(torch.isinf(want[0]).any()) and bool(torch.isfinite(want[0]).any())
    _same(got, want, f"k={k} max_radius")
    _same(dev.query(dev.points, k=k, exclude_self=True), cpu.query(P, k=k, exclude_self=True), f"k={k} exclude_self")
    _same(dev.query(dev.points, k=k, exclude_self=True, max_radius=radius),
          cpu.query(P, k=k, exclude_self=True, max_radius=radius), f"k={k} exclude_self max_radius")


def test_explicit_cell_sizes_give_the_same_result(random_grids):
    """Correctness does not depend on the cell size: cells far smaller and far larger than the default."""
    P, Q, dev, cpu = random_grids
    want = cpu.query(Q, k=3)
    for scale in (0.25, 4.0, 40.0):
        g, _ = _check_grid(P, dev.cell_size * scale, f"cell x{scale}")
        _same(g.query(Q.to(DEV), k=3), want, f"cell x{scale}")


def test_permuted_reference_set(random_grids):
    """The result for a permutation of the reference set: equal d2, and indices equal after mapping back (no two
    neighbours of a query tie in d2 here, which the test checks, so the tie rule does not enter)."""
    P, Q, dev, cpu = random_grids
    perm = torch.randperm(P.shape[0], generator=torch.Generator().manual_seed(5))
    d2, idx = dev.query(Q.to(DEV), k=8)
    d2p, idxp = N.PointGrid(P[perm].contiguous().to(DEV)).query(Q.to(DEV), k=8)
    assert not bool((d2[:, 1:] == d2[:, :-1]).any())
    assert torch.equal(_bits(d2), _bits(d2p))
    assert torch.equal(perm[idxp.cpu().long()], idx.cpu().long())


# ---------------------------------------------------------------------------------------- 2. sampler
def _meshes():
    V, F, r, h = NC.sphere_mesh()
    hv, hf, hs, _ = NC.hand_mesh()
    return {"sphere": (V, F, 0.5 * h), "sphere_coarse": (V, F, 4.0 * h), "hand": (hv, hf, hs)}


def _same_samples(got, want, what):
    for a, b, name in zip(got, want, ("samples", "weights", "face_of")):
        a, b = _bits(a), _bits(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} of {a.numel()} values"


@pytest.mark.parametrize("name", ["sphere", "sphere_coarse", "hand"])
def test_sampler_matches_twin(name):
    V, F, spacing = _meshes()[name]
    want = N.sample_mesh_eager(V, F, spacing)
    got = N.sample_mesh(V.to(DEV), F.to(DEV), spacing)
    assert want[0].shape[0] >= F.shape[0] and got[0].is_cuda
    _same_samples(got, want, name)


def test_sampler_writes_nothing_past_the_sizes_passed_in():
    """Sentinels laid after the caller-sized rows survive, also when the kernel is told fewer rows than the total;
    outputs smaller than the plan, a spacing too fine and a face index outside the vertices are refused before emit."""
    V, F, spacing = _meshes()["hand"]
    want = N.sample_mesh_eager(V, F, spacing)
    Vd, Fd = V.to(DEV), F.to(DEV)
    plan = N.sample_mesh_mark(Vd, Fd, spacing)
    S, pad = plan.n_samples, 64
    assert S == want[0].shape[0] and plan.n_max == max(NC.hand_mesh()[3])
    out = (torch.full((S + pad, 3), -7.5, device=DEV), torch.full((S + pad,), -7.5, device=DEV),
           torch.full((S + pad,), -12345, device=DEV, dtype=torch.int32))
    N.sample_mesh_emit(plan, *out)
    _same_samples([t[:S] for t in out], want, "padded outputs")
    assert bool((out[0][S:] == -7.5).all()) and bool((out[1][S:] == -7.5).all()) and bool((out[2][S:] == -12345).all())
    plan.args.n_samples = S - 7
    out[0].fill_(-7.5), out[1].fill_(-7.5), out[2].fill_(-12345)
    N.sample_mesh_emit(plan, *out)
    _same_samples([t[:S - 7] for t in out], [t[:S - 7] for t in want], "fewer")
    assert bool((out[0][S - 7:] == -7.5).all()) and bool((out[1][S - 7:] == -7.5).all()) and \
        bool((out[2][S - 7:] == -12345).all())
    plan.args.n_samples = S
    with pytest.raises(ValueError, match="fewer rows"):
        N.sample_mesh_emit(plan, out[0][:S - 1], out[1], out[2])
    with pytest.raises(ValueError, match="subdivisions"):
        N.sample_mesh_mark(Vd, Fd, 1e-3)
    bad = F.clone()
    bad[2, 1] = V.shape[0]
    with pytest.raises(ValueError, match="outside"):
        N.sample_mesh_mark(Vd, bad.to(DEV), spacing)


# ---------------------------------------------------------------------------------------- 3. score
def test_score_mesh_on_the_device_equals_the_twins():
    V, F, r, h = NC.sphere_mesh()
    ref = NC.sphere_points(2000, r + 0.05)
    kw = dict(spacing=0.5 * h, max_dist=0.058, thresholds=(0.04, 0.053, 0.07), bounds=((-1.0, -1.0, -0.1), (1.0, 1.0, 1.0)))
    want = M.score_mesh(V, F, ref, **kw)
    got = M.score_mesh(V.to(DEV), F.to(DEV), ref.to(DEV), **kw)
    assert got["d"].is_cuda and got["n_samples"] == want["n_samples"] and got["n_reference"] == want["n_reference"]
    for name in ("d", "e", "samples", "weights"):  # the roots of equal d2 are equal: sqrt is correctly rounded
        assert torch.equal(_bits(got[name]), _bits(want[name])), name
    for name in ("accuracy", "completeness", "chamfer"):
        assert math.isclose(got[name], want[name], rel_tol=1e-12), name  # float64 sums, in the device's order
    for name in ("precision", "recall", "fscore"):
        assert len(got[name]) == 3
        for a, b in zip(got[name], want[name]):
            assert math.isclose(a, b, rel_tol=1e-12, abs_tol=1e-15), name
    assert 0 < got["precision"][1] < 1 and 0 < got["recall"][1] < 1  # the middle threshold splits both sets
    assert float(got["d"].max()) == float(np.float32(0.058))  # and the clamp acts


# ---------------------------------------------------------------------------------------- 4. init
def test_knn_mean_dist_device_matches_the_reference(tmp_path):
    """The golden point cloud's neighbour distances (the reference's own) within the relative 1e-6 that
    tests/test_neighbors.py derives; a 2,000-point cloud against the host tree; and the opt-in initialisation route."""
    import os

    from scipy.spatial import cKDTree

    from gstex_amd.init import scene_from_point_cloud
    from gstex_amd.ply import write_ply
    from gstex_amd.scene import knn_mean_dist

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_golden.npz")) as z:
        for tag in ("raw", "fix"):
            xyz, want = z[f"lod_{tag}_xyz"], z[f"lod_{tag}_knn_dist"].astype(np.float64).mean(axis=-1)
            got = N.knn_mean_dist_device(torch.from_numpy(xyz).to(DEV), 3)
            assert got.is_cuda and got.dtype == torch.float32
            assert np.abs(got.cpu().numpy() / want - 1).max() <= 1e-6, tag
            assert np.abs(knn_mean_dist(xyz, 3, device=DEV) / want - 1).max() <= 1e-6, tag
    g = torch.Generator().manual_seed(8)
    xyz = torch.rand((2000, 3), generator=g)
    d, _ = cKDTree(xyz.double().numpy()).query(xyz.double().numpy(), k=4)
    got = N.knn_mean_dist_device(xyz.to(DEV), 3).cpu().numpy()
    assert np.abs(got / d[:, 1:].mean(-1) - 1).max() <= 1e-6
    rgb = torch.randint(0, 256, (2000, 3), generator=g).to(torch.uint8).numpy()
    x64 = xyz.double().numpy()
    path = tmp_path / "cloud.ply"
    write_ply(path, {"x": x64[:, 0], "y": x64[:, 1], "z": x64[:, 2], "red": rgb[:, 0], "green": rgb[:, 1],
                     "blue": rgb[:, 2]}, binary=True)
    a, b = scene_from_point_cloud(path), scene_from_point_cloud(path, knn_device=DEV)
    assert torch.allclose(torch.exp(a.log_scales), torch.exp(b.log_scales), rtol=1e-6, atol=0.0)
    assert torch.equal(a.means, b.means) and torch.equal(a.quats, b.quats)


# ---------------------------------------------------------------------------------------- 5. end to end
def _training_state(tr):
    st = {f"param {k}": p.detach().clone() for k, ps in tr.param_groups().items() for p in ps}
    st.update({f"grad {k}": (None if p.grad is None else p.grad.detach().clone())
               for k, ps in tr.param_groups().items() for p in ps})
    for p, s in tr.optimizer.state.items():
        for k, v in s.items():
            st[f"adam {id(p)} {k}"] = v.detach().clone() if isinstance(v, torch.Tensor) else v
    st["step"] = tr.step
    st["texel_grad"] = tr.texel_grad.state()
    st["sink"] = None if tr.texture_grad_sink is None else tr.texture_grad_sink.detach().clone()
    st["control"] = tr.step_control.clone()
    st["capacity"] = None if tr.pairs is None else tr.pairs.capacity
    st["background"] = tr.background.clone()
    return st


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            x, y = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a[k], b[k]))
            assert torch.equal(x, y), k
        else:
            assert a[k] == b[k], k


def test_trainer_score_mesh_end_to_end(tmp_path):
    """GStexTrainer.score_mesh on the tangent-splat sphere of mesh_cases.E2E against points on that sphere.  Every mesh
    vertex is within sqrt(3) h of the sphere (the extraction's end-to-end bound), so every surface point x has
    |x| <= R + sqrt(3) h and, by the chord argument of tests/test_neighbors.py with faces inside one cell,
    |x| >= sqrt((R - sqrt(3) h)^2 - h^2): within sqrt(3) h + sagitta of the sphere.  Its radial projection is within
    c (the reference points' covering radius, float64 brute force over a probe grid plus the grid's own analytic
    radius) of a reference point: accuracy <= sqrt(3) h + sagitta + c.  Completeness is not bounded: the views see a
    patch of the sphere."""
    from gstex_amd.export import score_mesh_ply
    from gstex_amd.model import GStexTrainer
    from gstex_amd.ply import write_ply

    E = MC.E2E
    R = E["R"]
    scene = MC.sphere_splat_scene(E["n"], R)
    tr = GStexTrainer(scene, DEV, sh_degree=3, start_step=3000)
    with torch.no_grad():
        tr.texture_dc.copy_(scene.features_dc.to(DEV))
    views = MC.e2e_views()
    h = 2 * R / (E["mesh_res"] - 12)
    ref = NC.sphere_points(6000, R)
    nt, npi = 90, 180
    t = (torch.arange(nt, dtype=torch.float64) + 0.5) * (math.pi / nt)
    p = torch.arange(npi, dtype=torch.float64) * (2 * math.pi / npi)
    tt, pp = torch.meshgrid(t, p, indexing="ij")
    probes = R * torch.stack([torch.sin(tt) * torch.cos(pp), torch.sin(tt) * torch.sin(pp), torch.cos(tt)], -1)
    worst = max(float(torch.cdist(c, ref.double()).min(dim=1).values.max()) for c in probes.reshape(-1, 3).split(4096))
    c = worst + R * math.hypot(math.pi / nt, 2 * math.pi / npi) / 2 + 4 * float(np.spacing(np.float32(R)))
    sagitta = (R - math.sqrt(3) * h) - math.sqrt((R - math.sqrt(3) * h) ** 2 - h * h)
    bound = math.sqrt(3) * h + sagitta + c

    before = _training_state(tr)
    sc = tr.score_mesh(views, ref, spacing=0.5 * h, thresholds=(bound,), mesh_res=E["mesh_res"])
    _assert_same_state(before, _training_state(tr))
    print(f"end to end: {sc['n_samples']} samples, accuracy {sc['accuracy']:.4f} (bound {bound:.4f}, h {h:.4f}), "
          f"completeness {sc['completeness']:.4f}")
    assert sc["faces"].shape[0] > 0 and sc["d"].is_cuda
    assert sc["accuracy"] <= bound and float(sc["d"].max()) <= bound * (1 + 1e-6) and sc["precision"] == [1.0]
    # it is score_mesh on extract_mesh's own output
    V, _, F = tr.extract_mesh(views, mesh_res=E["mesh_res"], color=False)
    assert torch.equal(V, sc["vertices"]) and torch.equal(F, sc["faces"])
    again = M.score_mesh(V, F, ref.to(DEV), spacing=0.5 * h, thresholds=(bound,))
    assert torch.equal(again["d"], sc["d"]) and torch.equal(again["e"], sc["e"])
    assert again["accuracy"] == sc["accuracy"] and again["completeness"] == sc["completeness"]
    # through the exporter, the reference read from a PLY
    r64 = ref.double().numpy()
    path = tmp_path / "ref.ply"
    write_ply(path, {"x": r64[:, 0], "y": r64[:, 1], "z": r64[:, 2]}, binary=True)
    ply = score_mesh_ply(tr, views, path, spacing=0.5 * h, mesh_res=E["mesh_res"])
    assert ply["accuracy"] == sc["accuracy"] and ply["completeness"] == sc["completeness"]
