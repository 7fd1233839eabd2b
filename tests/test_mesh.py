"""gstex_amd.mesh without a GPU: the C-ABI of the three mesh-extraction entry points and their argument checks, the
marching-tetrahedra table, the eager twins on analytic volumes (closed, oriented, chi = 2, the interpolation bound),
the mesh PLY writer, the component filter, and the whole pipeline on CPU-oracle renders of the tangent-splat sphere."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mesh_cases as C
from gstex_amd import _lib
from gstex_amd import mesh as M
from gstex_amd.ply import read_ply, write_mesh_ply

NEW = ("gstex_tsdf_integrate", "gstex_mesh_extract_mark", "gstex_mesh_extract_emit")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 3  # GSTEX_ERR_INVALID_ARG, GSTEX_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _status(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, _lib.last_error()


# ---------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "gstex_hip.h")).read()
    for s in NEW:
        assert f"int {s}(" in header and hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert "#define GSTEX_ABI_VERSION 19" in header
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19
    assert "tsdf.hip" in open(os.path.join(ROOT, "gstex_amd", "csrc", "Makefile")).read()


def test_struct_layouts_match_header(tmp_path):
    import subprocess

    structs = {"gstex_tsdf_volume": _lib.GstexTsdfVolume, "gstex_tsdf_view": _lib.GstexTsdfView,
               "gstex_tsdf_integrate_args": _lib.GstexTsdfIntegrateArgs,
               "gstex_mesh_extract_args": _lib.GstexMeshExtractArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append('printf("views %d\\n", GSTEX_TSDF_MAX_VIEWS);')
    lines.append('printf("words %d\\n", GSTEX_MESH_TABLE_WORDS);')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    assert int(got["views"]) == _lib.TSDF_MAX_VIEWS == 8
    assert int(got["words"]) == _lib.MESH_TABLE_WORDS == M.table_words().shape[0]
    for cname, cls in structs.items():
        assert int(got[f"{cname} size"]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got[f"{cname} {f[0]}"]) == getattr(cls, f[0]).offset, f"{cname}.{f[0]}"


def _buf():
    """A host word array's address: compared, null- and alignment-checked only (rejected before any launch)."""
    keep = (ctypes.c_float * 64)()
    return keep, ctypes.addressof(keep)


def _volume(b, dims=(4, 4, 4), color=None, **kw):
    a = dict(nx=dims[0], ny=dims[1], nz=dims[2], origin=(ctypes.c_float * 3)(0.0, 0.0, 0.0), voxel_size=0.1, tsdf=b,
             weight=b, color=color)
    a.update(kw)
    return _lib.GstexTsdfVolume(**a)


def _integrate_args(b, n_views=1, rgb=None, vol=None, **kw):
    cam = _lib.GstexCamera(b, None, 50.0, 50.0, 8.0, 8.0, 16, 16, 16)
    views = (_lib.GstexTsdfView * 9)(*[_lib.GstexTsdfView(cam, b, b, rgb) for _ in range(9)])
    a = dict(vol=vol if vol is not None else _volume(b), n_views=n_views, sdf_trunc=0.5, alpha_min=0.5,
             depth_trunc=0.0, near_z=0.2, views=views)
    a.update(kw)
    return _lib.GstexTsdfIntegrateArgs(**a), views


def test_integrate_rejects_bad_arguments(lib):
    keep, b = _buf()

    def status(**kw):
        a, views = _integrate_args(b, **kw)
        return _status(lib, "gstex_tsdf_integrate", ctypes.byref(a), None)

    rc, msg = _status(lib, "gstex_tsdf_integrate", None, None)
    assert rc == INVALID and "null args" in msg
    rc, msg = status(vol=_volume(b, tsdf=None))
    assert rc == INVALID and "null volume" in msg
    rc, msg = status(vol=_volume(b, weight=None))
    assert rc == INVALID and "null volume" in msg
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -3, 4)):
        rc, msg = status(vol=_volume(b, dims=dims))
        assert rc == INVALID and "dim must be >= 2" in msg, dims
    for n_views in (0, 9, -1):
        rc, msg = status(n_views=n_views)
        assert rc == INVALID and "n_views must be in [1, 8]" in msg, n_views
    # 7 * n_vox >= 2^31: 675^3 = 307,546,875 voxels is the first cube over it; 674^3 is under it and reaches the
    # next check (a null view table), so the limit is where the header puts it
    rc, msg = status(vol=_volume(b, dims=(675, 675, 675)))
    assert rc == UNSUPPORTED and "2^31" in msg
    assert 7 * 675 ** 3 >= 2 ** 31 > 7 * 674 ** 3
    rc, msg = status(vol=_volume(b, dims=(674, 674, 674)), views=None)
    assert rc == INVALID and "null view table" in msg
    rc, msg = status(vol=_volume(b, dims=(2048, 2048, 2048)))
    assert rc == UNSUPPORTED
    rc, msg = status(vol=_volume(b, color=b), rgb=None)
    assert rc == INVALID and "null rgb" in msg
    for name in ("sdf_trunc", "alpha_min", "near_z"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            rc, msg = status(**{name: v})
            assert rc == INVALID and f"{name} must be finite and > 0" in msg, (name, v)
    rc, msg = status(depth_trunc=-1.0)
    assert rc == INVALID and "depth_trunc" in msg
    rc, msg = status(vol=_volume(b, voxel_size=0.0))
    assert rc == INVALID and "voxel_size" in msg
    rc, msg = status(vol=_volume(b, tsdf=b + 2))
    assert rc == INVALID and "misaligned" in msg
    del keep


def test_extract_rejects_bad_arguments(lib):
    keep, b = _buf()

    def args(**kw):
        a = dict(vol=_volume(b), table=b, edge_mask=b, vertex_count=b, face_count=b, vertex_offsets=b,
                 face_offsets=b, n_vertices=4, n_faces=4, vertices=b, colors=None, faces=b)
        a.update(kw)
        return _lib.GstexMeshExtractArgs(**a)

    for fn in ("gstex_mesh_extract_mark", "gstex_mesh_extract_emit"):
        rc, msg = _status(lib, fn, None, None)
        assert rc == INVALID and "null args" in msg
        rc, msg = _status(lib, fn, ctypes.byref(args(vol=_volume(b, weight=None))), None)
        assert rc == INVALID and "null volume" in msg
        rc, msg = _status(lib, fn, ctypes.byref(args(vol=_volume(b, dims=(4, 1, 4)))), None)
        assert rc == INVALID and "dim must be >= 2" in msg
        rc, msg = _status(lib, fn, ctypes.byref(args(vol=_volume(b, dims=(675, 675, 675)))), None)
        assert rc == UNSUPPORTED and "2^31" in msg
        for name in ("table", "edge_mask", "vertex_count", "face_count"):
            rc, msg = _status(lib, fn, ctypes.byref(args(**{name: None})), None)
            assert rc == INVALID and "null pointer" in msg, name
    emit = "gstex_mesh_extract_emit"
    rc, msg = _status(lib, emit, ctypes.byref(args(n_vertices=-1)), None)
    assert rc == INVALID and "invalid sizes" in msg
    rc, msg = _status(lib, emit, ctypes.byref(args(vertex_offsets=None)), None)
    assert rc == INVALID and "null offsets" in msg
    rc, msg = _status(lib, emit, ctypes.byref(args(vertices=None)), None)
    assert rc == INVALID and "null vertices" in msg
    rc, msg = _status(lib, emit, ctypes.byref(args(faces=None)), None)
    assert rc == INVALID and "null faces" in msg
    rc, msg = _status(lib, emit, ctypes.byref(args(colors=b)), None)
    assert rc == INVALID and "colour volume" in msg
    # nothing to emit: a successful no-op before the outputs are looked at
    empty = args(n_vertices=0, n_faces=0, vertices=None, faces=None, vertex_offsets=None, face_offsets=None)
    assert lib.gstex_mesh_extract_emit(ctypes.byref(empty), None) == 0
    del keep


# ---------------------------------------------------------------------------------------- the table
def test_table_is_derived_by_geometry():
    assert len(M.MT_TABLE) == 6 and all(len(row) == 16 for row in M.MT_TABLE)
    assert len(M.MT_CORNERS) == 6 and len(set(M.MT_CORNERS)) == 6
    for corners in M.MT_CORNERS:
        assert corners[0] == (0, 0, 0) and corners[3] == (1, 1, 1)
        for a, b in zip(corners, corners[1:]):  # componentwise ascending, one axis at a time
            assert sum(q - p for p, q in zip(a, b)) == 1 and all(q >= p for p, q in zip(a, b))
    for t in range(6):
        assert M.MT_TABLE[t][0] == () and M.MT_TABLE[t][15] == ()
        for case in range(1, 15):
            tris, mirror = M.MT_TABLE[t][case], M.MT_TABLE[t][15 - case]
            inside = bin(case).count("1")
            assert len(tris) == (2 if inside == 2 else 1)
            # every edge joins an inside corner to an outside one
            assert all(((case >> lo) & 1) != ((case >> hi) & 1) and lo < hi for tri in tris for lo, hi in tri)
            # the complement: the same edge sets, every triangle wound the other way
            assert len(mirror) == len(tris)
            assert {frozenset(tri) for tri in tris} == {frozenset(tri) for tri in mirror}
            cyc = lambda tri: {(tri[k], tri[(k + 1) % 3]) for k in range(3)}  # noqa: E731
            for tri in tris:
                other = next(m for m in mirror if frozenset(m) == frozenset(tri))
                assert cyc(tri) == {(q, p) for p, q in cyc(other)}
            if inside == 2:  # the quad (a,c), (a,d), (b,d), (b,c) split along its first diagonal
                a, b = [k for k in range(4) if (case >> k) & 1]
                c, d = [k for k in range(4) if not (case >> k) & 1]
                edge = lambda p, q: (min(p, q), max(p, q))  # noqa: E731
                diagonal = {edge(a, c), edge(b, d)}
                assert all(diagonal <= set(tri) for tri in tris)
                assert set(tris[0]) == {edge(a, c), edge(a, d), edge(b, d)}
    words = M.table_words()
    assert words.dtype == np.int32 and words.shape == (102,)
    for t in range(6):
        for case in range(16):
            w = int(words[t * 16 + case])
            flat = [e for tri in M.MT_TABLE[t][case] for e in tri]
            assert (w >> 24) & 3 == len(M.MT_TABLE[t][case])
            assert [((w >> 4 * s) & 3, (w >> (4 * s + 2)) & 3) for s in range(len(flat))] == flat
        cw = int(words[96 + t])
        assert [((cw >> 3 * k) & 1, (cw >> (3 * k + 1)) & 1, (cw >> (3 * k + 2)) & 1) for k in range(4)] == \
            list(M.MT_CORNERS[t])


# ---------------------------------------------------------------------------------------- extraction twin
@pytest.mark.parametrize("n,r_over_h", [(16, 5.3), (12, 3.1)])
def test_extract_eager_sphere(n, r_over_h):
    """The prototype of the table rule measured 0.070 h (bound 0.105 h) at 16^3 and 0.119 h (bound 0.274 h) at 12^3."""
    tsdf, weight, origin, h, r = C.sphere_field(n, r_over_h)
    V, colors, F = M.mesh_extract_eager(tsdf, weight, None, origin, h)
    assert colors is None and V.dtype == torch.float32 and F.dtype == torch.int32
    p = C.mesh_properties(V, F)
    assert p["closed"] and p["chi"] == 2 and p["outward"] == 1.0 and p["referenced"] and p["degenerate"] == 0, p
    err = float((V.double().norm(dim=1) - r).abs().max())
    print(f"sphere {n}^3: V {V.shape[0]} F {F.shape[0]} max | |v| - r | = {err / h:.4f} h, bound "
          f"{C.sphere_error_bound(r, h) / h:.4f} h")
    assert err <= C.sphere_error_bound(r, h)


def test_extract_eager_order_is_the_contract():
    """Vertices ascend in 7 v(owner) + class and faces in (cell, tetrahedron, triangle): re-derived here from the
    positions alone."""
    tsdf, weight, origin, h, _ = C.sphere_field(12, 3.1)
    V, _, F = M.mesh_extract_eager(tsdf, weight, None, origin, h)
    n = 12
    o = np.asarray(origin, np.float64)
    lower = np.floor((V.double().numpy() - o) / h + 1e-4).astype(np.int64)  # the owner: the edge's lower corner
    frac = (V.double().numpy() - o) / h - lower
    moved = frac > 1e-4
    cls = np.array([M.EDGE_CLASSES.index(tuple(int(b) for b in m)) for m in moved])
    key = 7 * ((lower[:, 2] * n + lower[:, 1]) * n + lower[:, 0]) + cls
    assert (np.diff(key) > 0).all()
    # a face's cell: the componentwise minimum of its vertices' owners
    cell = lower[F.numpy().astype(np.int64)].min(axis=1)
    lin = (cell[:, 2] * n + cell[:, 1]) * n + cell[:, 0]
    assert (np.diff(lin) >= 0).all()


def test_extract_eager_random_field_and_zero_weights():
    tsdf, weight, color, origin, h = C.random_field()
    V, colors, F = M.mesh_extract_eager(tsdf, weight, color, origin, h)
    assert F.shape[0] > 0 and int(F.max()) < V.shape[0] and int(F.min()) >= 0
    assert colors.shape == V.shape and float(colors.min()) >= 0.0 and float(colors.max()) <= 1.0
    assert np.unique(F.numpy()).shape[0] == V.shape[0]
    # no vertex lies on an edge with a weight-0 end: each vertex's edge is recovered from its position
    o = np.asarray(origin, np.float64)
    g = (V.double().numpy() - o) / h
    lo, hi = np.floor(g + 1e-6).astype(int), np.ceil(g - 1e-6).astype(int)
    w = weight.numpy()
    assert (w[lo[:, 2], lo[:, 1], lo[:, 0]] > 0).all() and (w[hi[:, 2], hi[:, 1], hi[:, 0]] > 0).all()
    # and no face touches a weight-0 corner: with the weights all 1 the same field gives strictly more faces, and
    # every face of the masked run is one of them (same cell, tetrahedron and triangle => same three positions)
    V1, _, F1 = M.mesh_extract_eager(tsdf, torch.ones_like(weight), None, origin, h)
    tri = lambda V, F: {tuple(map(tuple, V[f.long()].numpy().round(6))) for f in F}  # noqa: E731
    assert tri(V, F) < tri(V1, F1)


def test_extract_eager_empty_fields():
    z = torch.zeros((6, 5, 4))
    for tsdf, weight in ((torch.full_like(z, 0.5), torch.ones_like(z)), (torch.rand(z.shape) - 0.5, z)):
        V, colors, F = M.mesh_extract_eager(tsdf, weight, torch.zeros((3, 6, 5, 4)), (0.0, 0.0, 0.0), 0.1)
        assert V.shape == (0, 3) and F.shape == (0, 3) and colors.shape == (0, 3)
        assert F.dtype == torch.int32


# ---------------------------------------------------------------------------------------- integration twin
def _integrate(views, renders, state=None, color=True):
    G = C.GRID
    nx, ny, nz = G["dims"]
    if state is None:
        z = torch.zeros((nz, ny, nx))
        state = (z, z.clone(), torch.zeros((3, nz, ny, nx)) if color else None)
    return M.tsdf_integrate_eager(*state, G["origin"], G["h"], views, renders, G["sdf_trunc"], G["alpha_min"],
                                  G["depth_trunc"], G["near_z"])


def test_integrate_eager_views_one_at_a_time():
    pairs = C.synthetic_views()[:8]
    views, renders = [p[0] for p in pairs], [p[1] for p in pairs]
    together = _integrate(views, renders)
    state = None
    for v, r in pairs:
        state = _integrate([v], [r], state)
    for a, b in zip(together, state):
        assert torch.equal(a, b)
    tsdf, weight, color = together
    reached = torch.zeros_like(weight, dtype=torch.bool)
    G = C.GRID
    for v, r in pairs:
        cls = M.classify_eager(G["origin"], G["h"], G["dims"], v, r, G["sdf_trunc"], G["alpha_min"],
                               G["depth_trunc"], G["near_z"])
        reached |= cls["ramp"] | cls["clamped"]
    assert int((~reached).sum()) > 0 and int(reached.sum()) > 0
    assert bool((weight[~reached] == 0).all()) and bool((tsdf[~reached] == 0).all())
    assert bool((color[:, ~reached] == 0).all())
    assert bool((weight[reached] >= 1).all()) and float(weight.max()) <= 8
    assert float(tsdf.max()) <= 1.0 and float(tsdf.min()) >= -1.0


def test_integrate_eager_single_voxel_by_hand():
    """One voxel on the optical axis of an identity camera, in python floats rounded per operation."""
    f = np.float32
    view = C.View(torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]), torch.eye(4), 20.0, 20.0, 4.0, 4.0, 8, 8)
    depth, alpha = torch.full((8, 8), 1.17), torch.full((8, 8), 0.9)
    rgb = torch.full((8, 8, 3), 0.25)
    z = torch.zeros((2, 2, 2))
    tsdf, weight, color = M.tsdf_integrate_eager(z, z.clone(), torch.zeros((3, 2, 2, 2)), (0.01, 0.02, 1.0), 0.25,
                                                 [view, view], [dict(depth=depth, alpha=alpha, rgb=rgb)] * 2, 0.5)
    d = f(1.17) / f(0.9)
    for k, zv in enumerate((f(1.0), f(1.0) + f(0.25) * f(1.0))):
        t = min(f(1.0), (d - zv) / f(0.5))
        once = (f(0.0) * f(0.0) + t) / f(1.0)
        twice = (once * f(1.0) + t) / f(2.0)
        assert float(tsdf[k, 0, 0]) == float(twice) and float(weight[k, 0, 0]) == 2.0
        assert float(color[0, k, 0, 0]) == 0.25


# ---------------------------------------------------------------------------------------- PLY and components
def test_write_mesh_ply(tmp_path):
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], np.float32)
    F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3]], np.int32)
    colors = np.array([[0.0, 1.0, 0.5], [-0.2, 1.7, 0.999], [1 / 255, 0.9999 / 255, 254.5 / 255], [0.25, 0.75, 1.0]],
                      np.float32)
    path = tmp_path / "mesh.ply"
    write_mesh_ply(path, V, F, colors)
    raw = path.read_bytes()
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 3\n"
            "property list uchar int vertex_indices\nend_header\n").encode()
    assert raw.startswith(head)
    assert len(raw) == len(head) + 4 * 15 + 3 * 13
    cols = read_ply(path)
    assert list(cols) == ["x", "y", "z", "red", "green", "blue"]
    np.testing.assert_array_equal(np.stack([cols["x"], cols["y"], cols["z"]], 1), V)
    want = np.array([[0, 255, 127], [0, 255, 254], [1, 0, 254], [63, 191, 255]], np.uint8)  # truncated, not rounded
    np.testing.assert_array_equal(np.stack([cols["red"], cols["green"], cols["blue"]], 1), want)
    faces = np.frombuffer(raw[len(head) + 60:], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert (faces["n"] == 3).all()
    np.testing.assert_array_equal(faces["i"], F)
    # without colours: 12 bytes per vertex; an empty mesh is a valid file
    write_mesh_ply(path, V, F)
    assert list(read_ply(path)) == ["x", "y", "z"] and b"red" not in path.read_bytes()
    write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert read_ply(path)["x"].shape == (0,)
    from gstex_amd.ply import PlyError

    with pytest.raises(PlyError):
        write_mesh_ply(path, V, np.array([[0, 1, 4]], np.int32))


def test_largest_components():
    tet = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    faces = np.concatenate([tet + 3, [[0, 1, 2]], tet + 7, [[11, 12, 13]]])  # stray triangle, tet, tet, (3-face) fan
    faces = np.concatenate([faces, [[11, 13, 14], [11, 14, 12]]])
    f, kept = M.largest_components(faces, 15, 2)
    np.testing.assert_array_equal(kept, np.arange(3, 11))
    np.testing.assert_array_equal(f, np.concatenate([tet, tet + 4]).astype(np.int32))
    f, kept = M.largest_components(faces, 15, 1)  # a tie: the component holding the lowest vertex
    np.testing.assert_array_equal(kept, np.arange(3, 7))
    f, kept = M.largest_components(faces, 15, 3)
    np.testing.assert_array_equal(kept, np.arange(3, 15))
    f, kept = M.largest_components(faces, 15, 10)
    assert f.shape == faces.shape and kept.shape == (15,) and f.dtype == np.int32
    f, kept = M.largest_components(np.zeros((0, 3), np.int32), 0, 1)
    assert f.shape == (0, 3) and kept.shape == (0,)
    with pytest.raises(ValueError):
        M.largest_components(faces, 14, 1)


def test_mesh_grid_formula():
    origin, h, dims, trunc, (lo, hi) = M.mesh_grid((-1, -1, -0.5), (1, 1, 0.5), None, 48, None)
    assert abs(h - 2.0 / 36) < 1e-12 and abs(trunc - 5 * h) < 1e-12
    assert abs((hi - lo).max() / h - 48) < 1e-9 and dims == (49, 49, 31)
    assert np.allclose(origin, [-1 - 6 * h, -1 - 6 * h, -0.5 - 6 * h])
    origin, h, dims, trunc, (lo, hi) = M.mesh_grid((-1, -1, -1), (1, 1, 1), None, 50, 0.2)
    assert abs(h - 2.4 / 48) < 1e-12 and trunc == 0.2 and abs((hi - lo).max() / h - 50) < 1e-9
    _, h, dims, trunc, _ = M.mesh_grid((0, 0, 0), (1, 1, 1), 0.1, 999, None)
    assert h == 0.1 and abs(trunc - 0.5) < 1e-12 and dims == (23, 23, 23)


# ---------------------------------------------------------------------------------------- the pipeline on the oracle
def test_pipeline_on_oracle_renders_stays_within_half_a_cell_diagonal():
    """TSDFVolume fed by oracle/raster.py renders of the tangent-splat sphere (mesh_cases.E2E at 32 x 32 and 4 views):
    every vertex within HALF of the end-to-end test's bound sqrt(3) h of the sphere.  Measured: 0.22 h at this size,
    0.17 h at the device test's 64 x 64 and 8 views (the bound is 1.73 h, half of it 0.87 h)."""
    E = C.E2E
    scene = C.sphere_splat_scene(E["n"], E["R"])
    views = C.e2e_views(32, 32, 4)
    renders = [C.oracle_mesh_render(scene, v) for v in views]
    assert all(float(r["alpha"].min()) > 0.9 for r in renders)  # no silhouette in any view
    lo, hi = scene.means.min(0).values.numpy(), scene.means.max(0).values.numpy()
    origin, h, dims, trunc, (lo_p, hi_p) = M.mesh_grid(lo, hi, None, E["mesh_res"], None)
    assert (4.0311 - E["R"]) / views[0].fx < h  # the pixel footprint at the surface is below a voxel
    vol = M.TSDFVolume("cpu", origin, h, dims, trunc, color=True)
    vol.integrate(views, renders)
    V, colors, F = vol.extract()
    assert F.shape[0] > 0 and colors.shape == V.shape
    assert bool((V >= torch.tensor(lo_p, dtype=torch.float32)).all())
    assert bool((V <= torch.tensor(hi_p, dtype=torch.float32)).all())
    err = float((V.double().norm(dim=1) - E["R"]).abs().max())
    print(f"oracle pipeline: V {V.shape[0]} F {F.shape[0]} max | |v| - R | = {err / h:.3f} h")
    assert err <= 0.5 * math.sqrt(3) * h
    vol.reset()
    assert float(vol.weight.abs().max()) == 0.0 and vol.extract()[2].shape[0] == 0
