"""The reference's initialisation routes as Scene builders (gstex.py:253-342, 377, 608-694).

Every preset of the reference starts from a file: a 2DGS PLY (`init_ply`, the NVS presets), a coloured point cloud
(`init_lod_ply`, scripts/blender_lod.py:10-14, scripts/dtu_lod.py) or an NPZ of activated-free parameters (`init_npz`).
Each builder here returns the `Scene` populate_modules leaves behind, in stored (pre-activation) form: one texel per
splat (`texture_dims[k] = (1, 1, k)`, gstex.py:333-339) holding the splat's DC colour (`texture = SH2RGB(features_dc)`,
gstex.py:341-342), `mappings = 1 / (2 * 3 * exp(scale))` (what build_charts writes, gstex.py:841-888), `rgbs` zero and
`pixel_scale` nan.  `trainer_from_scene` then does what populate_modules ends with (build_charts -> init_from_dims,
gstex.py:377): one rechart from the 1x1 charts onto the texel budget.

SH colour only (`sh_degree >= 1`): the sigmoid colour mode of gstex.py:325-326 is not built.
"""
from __future__ import annotations

import math
import re

import numpy as np
import torch

from .charts import RGB2SH, SH2RGB, random_quat_tensor
from .ply import read_ply
from .scene import Scene, knn_mean_dist


def _check_degree(sh_degree: int) -> int:
    if int(sh_degree) < 1:
        raise ValueError(f"sh_degree must be >= 1 (got {sh_degree}): the sigmoid colour mode is not supported")
    return int(sh_degree)


def _column(cols: dict, name: str, path) -> torch.Tensor:
    if name not in cols:
        raise ValueError(f"{path}: no property {name!r} (has {', '.join(cols) or 'none'})")
    return torch.tensor(cols[name], dtype=torch.float32)


def _columns(cols: dict, names, path) -> torch.Tensor:
    return torch.stack([_column(cols, n, path) for n in names], dim=1)


def _by_suffix(cols: dict, prefix: str):
    """The property names `prefix<int>` ordered by that integer (f_rest_10 after f_rest_9), as load_ply sorts them."""
    pat = re.compile(re.escape(prefix) + r"(\d+)$")
    found = [(int(m.group(1)), name) for name in cols for m in [pat.match(name)] if m]
    return [name for _, name in sorted(found)]


def axis_fix_points(xyz: torch.Tensor) -> torch.Tensor:
    """(x, y, z) -> (x, z, -y): fix_init / fix_lod_init (gstex.py:650-654, 683-687)."""
    return torch.stack([xyz[:, 0], xyz[:, 2], -xyz[:, 1]], dim=1)


def quat_to_matrix(q: torch.Tensor) -> torch.Tensor:
    """Rotation matrices (N, 3, 3) of wxyz quaternions of any non-zero norm: with s = 2 / |q|^2,
    R = I + s * (w [v]x + [v]x^2) for q = (w, v), written out per entry."""
    w, x, y, z = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    rows = [1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y),
            s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x),
            s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def matrix_to_quat(m: torch.Tensor) -> torch.Tensor:
    """Unit wxyz quaternions (w >= 0) of rotation matrices (N, 3, 3).  From the diagonal, 4 c^2 = 1 +- m00 +- m11
    +- m22 for each component c; the off-diagonal sums and differences give 4 c c' for every pair.  The largest
    component is taken from its square (the best conditioned root) and the other three from their products with it."""
    m00, m01, m02 = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2]
    m10, m11, m12 = m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    m20, m21, m22 = m[:, 2, 0], m[:, 2, 1], m[:, 2, 2]
    four_sq = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1)
    wx, wy, wz = m21 - m12, m02 - m20, m10 - m01  # 4 w x, 4 w y, 4 w z
    xy, xz, yz = m01 + m10, m02 + m20, m12 + m21  # 4 x y, 4 x z, 4 y z
    pick = four_sq.argmax(-1)
    lead = four_sq.gather(-1, pick[:, None])[:, 0]  # 4 c^2 of the leading component, >= 1 for a rotation
    # row c of the symmetric table 4 q q^T
    table = torch.stack([torch.stack([lead, wx, wy, wz], -1), torch.stack([wx, lead, xy, xz], -1),
                         torch.stack([wy, xy, lead, yz], -1), torch.stack([wz, xz, yz, lead], -1)], 1)
    row = table.gather(1, pick[:, None, None].expand(-1, 1, 4))[:, 0]
    q = row / (2.0 * torch.sqrt(lead))[:, None]
    return torch.where(q[:, :1] < 0, -q, q)


def axis_fix_quats(q: torch.Tensor) -> torch.Tensor:
    """fix_init's rotation (gstex.py:656-661): the matrix of each quaternion with its rows reordered to
    (r0, r2, -r1), as a unit wxyz quaternion.  Computed in float64 and rounded once."""
    r = quat_to_matrix(q.double())
    fixed = torch.stack([r[:, 0, :], r[:, 2, :], -r[:, 1, :]], dim=1)
    return matrix_to_quat(fixed).to(q.dtype)


def _one_texel_scene(means, log_scales, quats, opacity_logits, features_dc, features_rest) -> Scene:
    n = means.shape[0]
    dims = torch.ones((n, 3), dtype=torch.int32)
    dims[:, 2] = torch.arange(n, dtype=torch.int32)
    mappings = 1.0 / (2.0 * 3.0 * torch.exp(log_scales[:, :2]))
    return Scene(means=means, log_scales=log_scales, quats=quats, opacity_logits=opacity_logits,
                 features_dc=features_dc, features_rest=features_rest, rgbs=torch.zeros((n, 3)), texture_dims=dims,
                 mappings=mappings, texture=SH2RGB(features_dc), pixel_scale=float("nan"))


def scene_from_2dgs_ply(path, sh_degree: int = 3, fix_init: bool = False) -> Scene:
    """`init_ply` (load_ply, gstex.py:608-665; populate_modules, gstex.py:253-260, 294-296, 311-313): a 2DGS
    checkpoint PLY.  x y z; opacity as stored (logits); f_dc_0..2; f_rest_* by numeric suffix, channel-major in the
    file ((N, 3, K-1), returned as (N, K-1, 3)); scale_* by suffix with a column of ones appended to 2DGS's two;
    rot_* by suffix, wxyz, NOT normalised (the step's activation normalises).  Other columns (nx ny nz) are ignored.
    fix_init: the DTU presets' axis change of the means and rotations."""
    deg = _check_degree(sh_degree)
    cols = read_ply(path)
    means = _columns(cols, ("x", "y", "z"), path)
    n = means.shape[0]
    opacity = _column(cols, "opacity", path)[:, None]
    features_dc = _columns(cols, ("f_dc_0", "f_dc_1", "f_dc_2"), path)
    rest_names = _by_suffix(cols, "f_rest_")
    k = (deg + 1) ** 2
    if len(rest_names) != 3 * k - 3:
        raise ValueError(f"{path}: {len(rest_names)} f_rest_* properties; sh_degree {deg} needs {3 * k - 3}")
    features_rest = _columns(cols, rest_names, path).reshape(n, 3, k - 1).transpose(1, 2).contiguous()
    scale_names, rot_names = _by_suffix(cols, "scale_"), _by_suffix(cols, "rot_")
    if not 2 <= len(scale_names) <= 3:
        raise ValueError(f"{path}: {len(scale_names)} scale_* properties; expected 2 (2DGS) or 3")
    if len(rot_names) != 4:
        raise ValueError(f"{path}: {len(rot_names)} rot_* properties; expected 4")
    scales = _columns(cols, scale_names, path)
    if scales.shape[1] == 2:  # (gstex.py:257)
        scales = torch.cat([scales, torch.ones_like(scales[:, :1])], dim=-1)
    quats = _columns(cols, rot_names, path)
    if fix_init:
        means, quats = axis_fix_points(means), axis_fix_quats(quats)
    return _one_texel_scene(means, scales, quats, opacity, features_dc, features_rest)


def _seeded_scene(means, features_dc, sh_degree, log_scales=None, quats=None, opacity=None, seed=42,
                  knn_device=None) -> Scene:
    n = means.shape[0]
    features_rest = torch.zeros((n, (sh_degree + 1) ** 2 - 1, 3))
    if log_scales is None:  # the seeded-points branch (gstex.py:285-301)
        if n <= 3:
            raise ValueError(f"{n} points: the scale of a point is the mean distance to its 3 nearest neighbours")
        d = torch.from_numpy(knn_mean_dist(means.numpy(), 3, device=knn_device))
        log_scales = torch.log(d[:, None].repeat(1, 3))
        quats = random_quat_tensor(n, generator=torch.Generator().manual_seed(int(seed)))
        opacity = torch.logit(0.1 * torch.ones(n, 1))
    return _one_texel_scene(means, log_scales, quats, opacity, features_dc, features_rest)


def scene_from_point_cloud(path, fix_lod_init: bool = False, sh_degree: int = 3, seed: int = 42,
                           knn_device=None) -> Scene:
    """`init_lod_ply` (load_from_lod_ply, gstex.py:672-694; the seeded-points branch, gstex.py:278-301, 314-328): a
    point cloud with x y z and red green blue in 0..255.  features_dc = RGB2SH(colour / 255), features_rest zero,
    log-scales the log of the mean distance to the 3 nearest neighbours (x3), uniform random unit quaternions from a
    CPU generator seeded with `seed` (the reference draws them from the global generator), opacity logit(0.1).
    knn_device: where the neighbour distances are computed; None (the default) is cKDTree on the host, a HIP device
    the grid kernels of gstex_amd.neighbors (scene.knn_mean_dist)."""
    deg = _check_degree(sh_degree)
    cols = read_ply(path)
    means = _columns(cols, ("x", "y", "z"), path)
    colors = _columns(cols, ("red", "green", "blue"), path)
    if fix_lod_init:
        means = axis_fix_points(means)
    return _seeded_scene(means, RGB2SH(colors / 255), deg, seed=seed, knn_device=knn_device)


INIT_NPZ_KEYS = ("xyz", "colors", "opacity", "scaling", "rotation")


def scene_from_init_npz(path, sh_degree: int = 3) -> Scene:
    """`init_npz` (gstex.py:261-270, 294-296, 320-322): xyz, colors in [0, 1] (clamped to [1, 254] / 255 before
    RGB2SH), and opacity / scaling / rotation in stored form.  Read with allow_pickle=False."""
    deg = _check_degree(sh_degree)
    with np.load(path, allow_pickle=False) as z:
        for key in INIT_NPZ_KEYS:
            if key not in z.files:
                raise KeyError(f"{path}: not an init NPZ, missing {key!r}")
        d = {k: torch.from_numpy(np.array(z[k])) for k in INIT_NPZ_KEYS}
    colors = torch.clamp(255.0 * d["colors"], min=1.0, max=254.0)  # (in the file's dtype, as the reference)
    return _seeded_scene(d["xyz"].float(), RGB2SH(colors / 255).float(), deg, d["scaling"].float(),
                         d["rotation"].float(), d["opacity"].float())


def trainer_from_scene(scene: Scene, device, pixel_num: float, **trainer_kwargs):
    """The trainer populate_modules constructs (gstex.py:333-342, 377): built on the scene's 1x1 charts with
    texture_dc = features_dc (copied: SH2RGB -> RGB2SH does not round-trip exactly), then recharted once onto
    `pixel_num` texels (build_charts ending in init_from_dims, which resamples each 1x1 chart).  The step counter
    stays at start_step.  sh_degree defaults to the degree of the scene's features_rest."""
    from .model import GStexTrainer

    trainer_kwargs.setdefault("sh_degree", math.isqrt(int(scene.features_rest.shape[1]) + 1) - 1)
    tr = GStexTrainer(scene, device, pixel_num=float(pixel_num), **trainer_kwargs)
    with torch.no_grad():
        tr.texture_dc.copy_(scene.features_dc.to(tr.device))
    tr.recharge()
    return tr
