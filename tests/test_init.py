"""gstex_amd.init: the reference's initialisation routes as Scene builders, against what the reference's own loaders
return for the committed inputs (tests/golden/make_init_golden.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from gstex_amd.charts import RGB2SH, SH2RGB
from gstex_amd.init import (matrix_to_quat, quat_to_matrix, scene_from_2dgs_ply, scene_from_init_npz,
                            scene_from_point_cloud)
from gstex_amd.ply import read_ply, write_ply

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLY_2DGS = os.path.join(GOLDEN, "init_2dgs.ply")
PLY_LOD = os.path.join(GOLDEN, "init_lod.ply")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "init_golden.npz"), allow_pickle=False) as z:
        return {k: torch.from_numpy(np.array(z[k])) for k in z.files}


def _check_one_texel_form(sc):
    n = sc.n
    assert sc.texture_dims.dtype == torch.int32
    assert sc.texture_dims.tolist() == [[1, 1, k] for k in range(n)]
    assert torch.equal(sc.texture, SH2RGB(sc.features_dc))
    assert torch.equal(sc.mappings, 1.0 / (2.0 * 3.0 * torch.exp(sc.log_scales[:, :2])))
    assert torch.equal(sc.rgbs, torch.zeros(n, 3))
    assert sc.pixel_scale != sc.pixel_scale  # nan
    for t in (sc.means, sc.log_scales, sc.quats, sc.opacity_logits, sc.features_dc, sc.features_rest):
        assert t.dtype == torch.float32 and t.shape[0] == n
    assert sc.log_scales.shape == (n, 3) and sc.quats.shape == (n, 4) and sc.opacity_logits.shape == (n, 1)


def _rotmat64(q):
    """Rotation matrix of a wxyz quaternion, float64, written independently of gstex_amd.init (via the axis-angle
    free form R = (w^2 - v.v) I + 2 v v^T + 2 w [v]x on the unit quaternion)."""
    q = q.double()
    q = q / q.norm(dim=-1, keepdim=True)
    w, v = q[:, 0], q[:, 1:]
    eye = torch.eye(3, dtype=torch.float64)[None]
    cross = torch.zeros(q.shape[0], 3, 3, dtype=torch.float64)
    cross[:, 0, 1], cross[:, 0, 2] = -v[:, 2], v[:, 1]
    cross[:, 1, 0], cross[:, 1, 2] = v[:, 2], -v[:, 0]
    cross[:, 2, 0], cross[:, 2, 1] = -v[:, 1], v[:, 0]
    return ((w * w - (v * v).sum(-1))[:, None, None] * eye + 2 * v[:, :, None] * v[:, None, :]
            + 2 * w[:, None, None] * cross)


@pytest.mark.parametrize("fix", [False, True])
def test_2dgs_ply_against_the_reference_loader(golden, fix):
    tag = "fix" if fix else "raw"
    sc = scene_from_2dgs_ply(PLY_2DGS, sh_degree=3, fix_init=fix)
    assert sc.n == 16
    assert torch.equal(sc.means, golden[f"ply_{tag}_xyz"])
    assert torch.equal(sc.opacity_logits, golden[f"ply_{tag}_opacity"])
    assert torch.equal(sc.features_dc, golden[f"ply_{tag}_features_dc"][:, 0, :])  # (gstex.py:312)
    assert sc.features_rest.shape == (16, 15, 3) and sc.features_rest.is_contiguous()
    assert torch.equal(sc.features_rest, golden[f"ply_{tag}_features_rest"])
    assert torch.equal(sc.log_scales[:, :2], golden[f"ply_{tag}_scaling"])
    assert torch.equal(sc.log_scales[:, 2], torch.ones(16))  # (gstex.py:257)
    gq = golden[f"ply_{tag}_rotation"]
    if not fix:
        assert torch.equal(sc.quats, gq)
        norms = sc.quats.norm(dim=-1)
        assert float(norms.min()) < 0.9 and float(norms.max()) > 1.1  # as stored: not normalised
    else:
        assert torch.allclose(sc.quats.norm(dim=-1), torch.ones(16), atol=1e-6)
        err = (_rotmat64(sc.quats) - _rotmat64(gq)).abs().max()
        print(f"fix_init rotation matrices: max abs difference {float(err):.3e}")
        assert float(err) <= 1e-6
        # and the fix is the stated one: rows (r0, r2, -r1) of the raw file's rotations, means (x, z, -y)
        raw = scene_from_2dgs_ply(PLY_2DGS, sh_degree=3)
        r = _rotmat64(raw.quats)
        want = torch.stack([r[:, 0], r[:, 2], -r[:, 1]], 1)
        assert float((_rotmat64(sc.quats) - want).abs().max()) <= 1e-6
        assert torch.equal(sc.means, torch.stack([raw.means[:, 0], raw.means[:, 2], -raw.means[:, 1]], 1))
    _check_one_texel_form(sc)


def test_quaternion_matrix_pair_round_trips_every_branch():
    # one quaternion led by each component (the four branches of matrix_to_quat), plus random ones, at odd norms
    g = torch.Generator().manual_seed(3)
    q = torch.cat([torch.eye(4, dtype=torch.float64) * 0.9 + 0.1 * torch.rand(4, 4, generator=g, dtype=torch.float64),
                   torch.randn(60, 4, generator=g, dtype=torch.float64)])
    m = quat_to_matrix(q * torch.linspace(0.5, 2.0, q.shape[0], dtype=torch.float64)[:, None])
    assert torch.allclose(m @ m.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand_as(m), atol=1e-12)
    assert torch.allclose(torch.linalg.det(m), torch.ones(q.shape[0], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(m, _rotmat64(q), atol=1e-12)
    back = matrix_to_quat(m)
    unit = q / q.norm(dim=-1, keepdim=True)
    unit = torch.where(unit[:, :1] < 0, -unit, unit)
    assert torch.allclose(back, unit, atol=1e-12)


def _2dgs_columns(n, degree, seed=0):
    g = np.random.default_rng(seed)
    cols = {k: g.normal(0, 1, n).astype(np.float32) for k in ("x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2",
                                                               "scale_0", "scale_1", "rot_0", "rot_1", "rot_2",
                                                               "rot_3")}
    for i in range(3 * (degree + 1) ** 2 - 3):
        cols[f"f_rest_{i}"] = np.full(n, float(i), np.float32) + np.arange(n, dtype=np.float32) / 100
    return cols


def test_f_rest_is_ordered_by_numeric_suffix(tmp_path):
    cols = _2dgs_columns(5, 3)
    lexi = {k: cols[k] for k in sorted(cols)}  # f_rest_10 before f_rest_2, rot/scale after
    assert list(lexi).index("f_rest_10") < list(lexi).index("f_rest_2")
    path = tmp_path / "lexi.ply"
    write_ply(path, lexi)
    sc = scene_from_2dgs_ply(path, sh_degree=3)
    # column i of the file is channel i // 15, coefficient i % 15 (gstex.py:629, 645)
    for i in range(45):
        assert torch.equal(sc.features_rest[:, i % 15, i // 15], torch.from_numpy(cols[f"f_rest_{i}"])), i
    assert torch.equal(sc.quats, torch.from_numpy(np.stack([cols[f"rot_{i}"] for i in range(4)], 1)))


def test_wrong_f_rest_count_for_the_degree_raises(tmp_path):
    path = tmp_path / "deg2.ply"
    write_ply(path, _2dgs_columns(5, 2))
    assert scene_from_2dgs_ply(path, sh_degree=2).features_rest.shape == (5, 8, 3)
    with pytest.raises(ValueError, match="f_rest"):
        scene_from_2dgs_ply(path, sh_degree=3)
    with pytest.raises(ValueError, match="sh_degree"):
        scene_from_2dgs_ply(path, sh_degree=0)
    cols = _2dgs_columns(5, 2)
    del cols["opacity"]
    write_ply(path, cols)
    with pytest.raises(ValueError, match="opacity"):
        scene_from_2dgs_ply(path, sh_degree=2)


@pytest.mark.parametrize("fix", [False, True])
def test_point_cloud_against_the_reference_loader(golden, fix):
    tag = "fix" if fix else "raw"
    sc = scene_from_point_cloud(PLY_LOD, fix_lod_init=fix, sh_degree=3, seed=42)
    assert sc.n == 64
    assert read_ply(PLY_LOD)["x"].dtype == np.float64 and read_ply(PLY_LOD)["red"].dtype == np.uint8
    assert torch.equal(sc.means, golden[f"lod_{tag}_xyz"])
    assert torch.equal(sc.features_dc, RGB2SH(golden[f"lod_{tag}_rgbs"] / 255))  # (gstex.py:322)
    assert torch.equal(sc.features_rest, torch.zeros(64, 15, 3))
    want = torch.log(golden[f"lod_{tag}_knn_dist"].mean(dim=-1, keepdim=True).repeat(1, 3))  # (gstex.py:288, 300)
    assert torch.allclose(sc.log_scales, want, rtol=1e-6, atol=0.0)
    assert torch.equal(sc.opacity_logits, torch.logit(0.1 * torch.ones(64, 1)))
    assert torch.allclose(sc.quats.norm(dim=-1), torch.ones(64), atol=1e-6)
    again = scene_from_point_cloud(PLY_LOD, fix_lod_init=fix, seed=42)
    other = scene_from_point_cloud(PLY_LOD, fix_lod_init=fix, seed=43)
    assert torch.equal(sc.quats, again.quats) and not torch.equal(sc.quats, other.quats)
    _check_one_texel_form(sc)
    with pytest.raises(ValueError, match="sh_degree"):
        scene_from_point_cloud(PLY_LOD, sh_degree=0)


def _init_npz(path, n=6, drop=None, dtype=np.float32):
    g = np.random.default_rng(1)
    colors = g.uniform(0.1, 0.9, (n, 3)).astype(dtype)
    colors[0] = [0.0, 0.5 / 255, 0.99 / 255]       # below the lower clamp
    colors[1] = [1.0, 254.5 / 255, 254.01 / 255]   # above the upper clamp
    d = dict(xyz=g.normal(0, 1, (n, 3)).astype(np.float32), colors=colors,
             opacity=g.normal(0, 1, (n, 1)).astype(np.float32), scaling=g.normal(-3, 0.3, (n, 3)).astype(np.float32),
             rotation=g.normal(0, 1, (n, 4)).astype(np.float32))
    if drop:
        del d[drop]
    np.savez(path, **d)
    return d


def test_init_npz_clamps_the_colours(tmp_path):
    path = tmp_path / "init.npz"
    d = _init_npz(path)
    sc = scene_from_init_npz(path, sh_degree=3)
    lo, hi = RGB2SH(torch.tensor(1.0) / 255), RGB2SH(torch.tensor(254.0) / 255)
    assert torch.equal(sc.features_dc[0], torch.stack([lo, lo, lo]))
    assert torch.equal(sc.features_dc[1], torch.stack([hi, hi, hi]))
    inner = torch.from_numpy(d["colors"][2:])
    assert torch.equal(sc.features_dc[2:], RGB2SH(255.0 * inner / 255))  # (gstex.py:264, 322)
    for got, key in ((sc.means, "xyz"), (sc.opacity_logits, "opacity"), (sc.log_scales, "scaling"),
                     (sc.quats, "rotation")):
        assert torch.equal(got, torch.from_numpy(d[key])), key
    assert torch.equal(sc.features_rest, torch.zeros(6, 15, 3))
    _check_one_texel_form(sc)
    with pytest.raises(ValueError, match="sh_degree"):
        scene_from_init_npz(path, sh_degree=0)


@pytest.mark.parametrize("key", ["xyz", "colors", "opacity", "scaling", "rotation"])
def test_init_npz_missing_key(tmp_path, key):
    path = tmp_path / "init.npz"
    _init_npz(path, drop=key)
    with pytest.raises(KeyError, match=key):
        scene_from_init_npz(path)


def test_init_npz_refuses_pickled_arrays(tmp_path):
    path = tmp_path / "init.npz"
    d = _init_npz(path)
    d["colors"] = np.array([{"a": 1}], dtype=object)
    np.savez(path, **d)
    with pytest.raises(ValueError):
        scene_from_init_npz(path)
