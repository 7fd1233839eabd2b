"""Shared inputs and checks of tests/test_mesh.py and tests/test_gpu_mesh.py (no test in here): analytic volumes, the
synthetic views of the integrate test, the tangent-splat sphere of the end-to-end test and the mesh properties."""
import functools
import math

import numpy as np
import torch

from gstex_amd.scene import View, look_at, sphere_view

OFFSET = (0.013, 0.007, -0.004)  # a non-lattice shift of the grid: no sample is exactly 0


def sphere_field(n: int, r_over_h: float):
    """tsdf = clamp((|p| - r) / (5 h), -1, 1) on an n^3 grid centred near the origin, all weights 1.
    -> (tsdf (n, n, n), weight, origin, h, r)."""
    h = float(np.float32(1.0 / n))
    origin = tuple(float(np.float32(-0.5 + o)) for o in OFFSET)
    ax = [torch.tensor(origin[c], dtype=torch.float32) + torch.tensor(h) * torch.arange(n, dtype=torch.float32)
          for c in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    r = r_over_h * h
    dist = torch.sqrt(x.double() ** 2 + y.double() ** 2 + z.double() ** 2)
    tsdf = torch.clamp((dist - r) / (5 * h), -1.0, 1.0).float()
    assert not bool((tsdf == 0).any())
    return tsdf, torch.ones_like(tsdf), origin, h, r


def random_field(seed: int = 3, n: int = 8):
    """Random signs on an n^3 grid with 10 % of the weights zero, and a colour volume."""
    g = torch.Generator().manual_seed(seed)
    tsdf = torch.rand((n, n, n), generator=g) * 2 - 1
    weight = (torch.rand((n, n, n), generator=g) >= 0.1).float() * torch.randint(1, 4, (n, n, n), generator=g).float()
    color = torch.rand((3, n, n, n), generator=g)
    assert int((weight == 0).sum()) > 0 and not bool((tsdf == 0).any())
    return tsdf, weight, color, (-0.31, 0.12, 0.05), 0.0625


def mesh_properties(vertices, faces, centre=(0.0, 0.0, 0.0)) -> dict:
    """closed (every directed edge once and its reverse once), chi = V - E + F, outward (fraction of the faces whose
    normal points away from `centre`), referenced (every vertex is used) and degenerate (faces of zero area)."""
    V = vertices.detach().cpu().double().numpy()
    F = faces.detach().cpu().numpy().astype(np.int64)
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    code = a * (V.shape[0] + 1) + b
    uniq, counts = np.unique(code, return_counts=True)
    closed = bool((counts == 1).all()) and bool(np.isin(b * (V.shape[0] + 1) + a, uniq).all())
    n_edges = np.unique(np.minimum(a, b) * (V.shape[0] + 1) + np.maximum(a, b)).shape[0]
    nrm = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    cen = V[F].mean(1) - np.asarray(centre)
    return dict(closed=closed, chi=V.shape[0] - n_edges + F.shape[0], outward=float(((nrm * cen).sum(1) > 0).mean()),
                referenced=np.unique(F).shape[0] == V.shape[0],
                degenerate=int((np.linalg.norm(nrm, axis=1) == 0).sum()))


def sphere_error_bound(r: float, h: float) -> float:
    """3 h^2 / (8 (r - sqrt(3) h)): linear interpolation of a distance function along an edge of length at most
    sqrt(3) h, plus 4 fp32 ulps of r."""
    return 3 * h * h / (8 * (r - math.sqrt(3) * h)) + 4 * float(np.spacing(np.float32(r)))


# ------------------------------------------------------------------------------------------ the integrate test's views
GRID = dict(origin=(-1.6, -0.8, -0.4), h=0.1, dims=(33, 17, 9), sdf_trunc=0.3, alpha_min=0.5, depth_trunc=1.6,
            near_z=0.2)
VIEW_W, VIEW_H = 48, 40
_CAMS = [((-1.0, 0.0, 0.0), (1.0, 0.05, 0.02)), ((-0.4, -0.3, 0.1), (1.2, 0.4, -0.1)), ((2.4, 0.2, 0.3), (0.0, 0.0, 0.0)),
         ((0.0, -1.9, 0.2), (0.1, 0.0, 0.0)), ((0.3, 0.1, 1.6), (0.0, 0.0, 0.0)), ((-2.2, 0.9, -0.5), (0.0, 0.0, 0.0)),
         ((1.0, 1.5, 0.4), (-0.5, 0.0, 0.0)), ((-0.2, 0.1, -1.4), (0.2, 0.0, 0.1)), ((1.4, -0.6, 0.0), (-1.0, 0.2, 0.0))]


@functools.lru_cache(maxsize=None)
def synthetic_views():
    """Nine (view, render) pairs on the CPU: 48 x 40 images with fx != fy and an off-centre principal point; depth and
    alpha are smooth synthetic images (no raster), alpha with a patch below alpha_min, rgb random.  The first camera
    sits inside the grid, so the grid has voxels behind it, nearer than near_z and outside every image border."""
    g = torch.Generator().manual_seed(11)
    r, c = torch.meshgrid(torch.arange(VIEW_H, dtype=torch.float32), torch.arange(VIEW_W, dtype=torch.float32),
                          indexing="ij")
    out = []
    for q, (pos, target) in enumerate(_CAMS):
        vm, c2w = look_at(pos, target)
        view = View(vm, c2w, 60.0, 50.0, 22.3, 21.1, VIEW_H, VIEW_W)
        expected = 1.2 + 0.3 * torch.sin(0.2 * c + q) + 0.2 * torch.cos(0.3 * r - q)  # in [0.7, 1.7]
        alpha = 0.7 + 0.25 * torch.rand((VIEW_H, VIEW_W), generator=g)
        alpha[5:12, 8 + 3 * q % 20:16 + 3 * q % 20] = 0.3
        out.append((view, dict(depth=(expected * alpha).contiguous(), alpha=alpha.contiguous(),
                               rgb=torch.rand((VIEW_H, VIEW_W, 3), generator=g))))
    return tuple(out)


# ------------------------------------------------------------------------------------------ the end-to-end sphere
def sphere_splat_scene(n: int, R: float, sigma_over_spacing: float = 1.0, opacity: float = 0.99, seed: int = 5):
    """Opaque one-texel splats tangent to the sphere of radius R: means on a Fibonacci sphere, radial normals, scale
    about the spacing sqrt(4 pi R^2 / n)."""
    from gstex_amd.init import _one_texel_scene, matrix_to_quat

    i = torch.arange(n, dtype=torch.float64) + 0.5
    zc = 1 - 2 * i / n
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    rxy = torch.sqrt(1 - zc * zc)
    nrm = torch.stack([rxy * torch.cos(phi), rxy * torch.sin(phi), zc], -1)
    ref = torch.where((nrm[:, 2].abs() < 0.9)[:, None], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64),
                      torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    tu = torch.linalg.cross(ref, nrm)
    tu = tu / tu.norm(dim=1, keepdim=True)
    tv = torch.linalg.cross(nrm, tu)
    quats = matrix_to_quat(torch.stack([tu, tv, nrm], -1)).float()
    spacing = math.sqrt(4 * math.pi * R * R / n)
    g = torch.Generator().manual_seed(seed)
    log_scales = torch.full((n, 3), math.log(sigma_over_spacing * spacing))
    return _one_texel_scene((R * nrm).float(), log_scales, quats, torch.full((n, 1), math.log(opacity / (1 - opacity))),
                            torch.rand((n, 3), generator=g) * 2 - 1, torch.zeros((n, 15, 3)))


def oracle_mesh_render(scene, view, background=(1.0, 1.0, 1.0)) -> dict:
    """What GStexTrainer._mesh_render gives extract_mesh, from the CPU oracle (oracle/raster.py) in fp32."""
    from gstex_amd.charts import SH2RGB, get_uv_mapping
    from gstex_amd.model import DEFAULT_SETTINGS
    from oracle import raster as O

    means, scales, quats, opac = scene.activated()
    uv0, umap, vmap = get_uv_mapping(quats, scene.mappings)
    campos = view.c2w[:3, 3]
    cam = O.Camera(view.viewmat, view.fx, view.fy, view.cx, view.cy, view.H, view.W, 16, campos)
    centers, extents = O.aabb_2d(means, scales, 1.0, quats, cam)
    _, depths = O.project_points(means, cam)
    rgbs = torch.zeros((means.shape[0], 3))  # SH colour with the DC zeroed and features_rest zero
    inp = O.RasterInputs(scene.texture_dims, centers, extents, depths, rgbs, opac, means, scales, 1.0, quats, uv0, umap,
                         vmap, scene.texture[:, :3].contiguous(), cam, DEFAULT_SETTINGS, None)
    out, _, _ = O.rasterize(inp)
    bg = torch.tensor(background, dtype=torch.float32)
    rgb = torch.clamp(out["img"] + out["tex"][:, :, 0:3] + (1 - out["alpha"][:, :, None]) * bg, 0.0, 1.0)
    return dict(depth=out["depth"].contiguous(), alpha=out["alpha"].contiguous(), rgb=rgb.contiguous())


# The end-to-end case: R, splat count, image size, view count and mesh_res (tests/test_gpu_mesh.py on the device, and
# the same pipeline on oracle renders in tests/test_mesh.py at 32 x 32 and 4 views).  Spacing = sigma = 0.156, voxel
# h = 2 R / (mesh_res - 12) = 0.122, pixel footprint at the surface (4.03 - R) / fx = 0.021 = 0.17 h.  R = 2.2 keeps the
# sphere's silhouette outside every image, corners included (it enters at R < 1.83): a silhouette pixel's depth is
# applied to every voxel that projects into it, and those next to the limb ray lie outside the sphere, so a fin of
# negative voxels up to sdf_trunc long trails each limb.  Measured on oracle renders at R = 1.0 .. 1.6 with 1200 to
# 60000 splats, opacity 0.99 and 0.999: |r - R| up to 2.2 .. 2.6 h, whatever the opacity and density (it is the
# nearest-pixel lookup at grazing incidence, not the splats); with 100 views the other views' free-space votes
# outweigh a fin, with 8 they do not.  At R = 2.2 the same pipeline measures 0.17 h (64 x 64, 8 views).
E2E = dict(R=2.2, n=2500, H=64, W=64, n_views=8, mesh_res=48)


def e2e_views(H=None, W=None, n_views=None):
    H, W, n_views = H or E2E["H"], W or E2E["W"], n_views or E2E["n_views"]
    return [sphere_view(i, H, W, n_views) for i in range(n_views)]
