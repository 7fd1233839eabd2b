"""GStex parameter export/import in the reference's NPZ wire format.

``export_npz`` writes exactly the arrays of ``ExportGStexNpz`` (nerfstudio/scripts/exporter.py:78-105):
xyz, features_rest, opacity, scaling, rotation, texture_dc, texture_dims, mappings (parameters in
their stored, pre-activation form; texture_dc holds SH-DC values, gstex.py:1119).  ``trainer_from_npz``
rebuilds a ``GStexTrainer`` from such a file bit-exactly (features_dc, which the exporter omits, is zero:
under SH colour the DC term is replaced by the texture, gstex.py:1100).  ``average_colors`` is
``GStexModel.get_average_colors`` (gstex.py:714-726), used by the reference's PLY export, which ``export_ply``
restates (``ExportGStexPly``, exporter.py:52-76) on gstex_amd.ply's writer.
"""
from __future__ import annotations

import numpy as np
import torch

from .charts import SH2RGB

NPZ_KEYS = ("xyz", "features_rest", "opacity", "scaling", "rotation", "texture_dc", "texture_dims", "mappings")


def export_npz(trainer, path) -> None:
    if hasattr(trainer, "wait_texture"):  # defer_texture: the pending texel update must run before the read
        trainer.wait_texture()
    params = {
        "xyz": trainer.means,
        "features_rest": trainer.features_rest,
        "opacity": trainer.opacities,
        "scaling": trainer.scales,
        "rotation": trainer.quats,
        "texture_dc": trainer.texture_dc,
        "texture_dims": trainer.texture_dims,
        "mappings": trainer.mappings,
    }
    np.savez(path, **{k: v.detach().cpu().numpy() for k, v in params.items()})


def load_npz(path) -> dict:
    """The NPZ arrays as CPU tensors (no pickle: allow_pickle=False)."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in NPZ_KEYS if k not in z.files]
        if missing:
            raise KeyError(f"{path}: not a GStex NPZ export, missing {missing}")
        return {k: torch.from_numpy(np.array(z[k])) for k in NPZ_KEYS}


def average_colors(texture_dc: torch.Tensor, texture_dims: torch.Tensor, sh_degree: int = 3) -> torch.Tensor:
    """Per-splat mean texel colour (gstex.py:714-726): SH2RGB (sigmoid without SH) of each splat's
    h*w texels, averaged."""
    n = texture_dims.shape[0]
    hws = (texture_dims[:, 0] * texture_dims[:, 1]).long()
    ids = torch.repeat_interleave(torch.arange(n, device=texture_dims.device), hws)
    tex = texture_dc[: ids.numel()]
    tex = SH2RGB(tex) if sh_degree > 0 else torch.sigmoid(tex)
    avg = torch.zeros((n, tex.shape[-1]), device=tex.device, dtype=torch.float32)
    return torch.index_add(avg, 0, ids, tex) / hws.float()[:, None]


def export_ply(trainer, path) -> None:
    """ExportGStexPly (scripts/exporter.py:52-76): a point cloud of the splat centres coloured by each splat's mean
    texel colour, clamp(average_colors, 0, 1).  Little-endian binary, `double x y z` then `uchar red green blue`
    (the colour times 255, rounded to nearest).  The reference writes the file with open3d's write_point_cloud;
    these column types and the rounding follow that writer from memory, which cannot be checked here (open3d is
    absent).  What is checked: the file is a valid `init_lod_ply` (gstex_amd.init.scene_from_point_cloud), the
    format the reference's own LOD inits use."""
    from .ply import write_ply

    with torch.no_grad():
        xyz = trainer.means.detach().cpu().numpy().astype(np.float64)
        colors = torch.clamp(average_colors(trainer.texels(), trainer.texture_dims, trainer.sh_degree), 0.0, 1.0)
        rgb = torch.round(colors * 255.0).to(torch.uint8).cpu().numpy()
    write_ply(path, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2],
                     "red": rgb[:, 0], "green": rgb[:, 1], "blue": rgb[:, 2]}, binary=True)


def export_2dgs_ply(trainer, path) -> None:
    """A one-texel trainer (the geometry stage's result, gstex_amd.density) as the 2DGS checkpoint PLY that
    gstex_amd.init.scene_from_2dgs_ply reads: float columns x y z, nx ny nz (zeros), f_dc_0..2 (each splat's texel, the
    SH-DC colour; under SH colour the features_dc parameter is replaced by the texture), f_rest_* channel-major,
    opacity (logit), scale_0 scale_1 (log; the unused third column is not part of the format, the reader appends
    ones) and rot_0..3 (raw, wxyz).  Anything but one texel per splat raises ValueError."""
    from .ply import write_ply

    n = int(trainer.means.shape[0])
    dims = trainer.texture_dims.detach().cpu()
    want = torch.ones((n, 3), dtype=dims.dtype)
    want[:, 2] = torch.arange(n, dtype=dims.dtype)
    if trainer.n_texels != n or tuple(dims.shape) != (n, 3) or not torch.equal(dims, want):
        raise ValueError("export_2dgs_ply: a 2DGS checkpoint has one colour per splat; this trainer's charts hold "
                         f"{trainer.n_texels} texels for {n} splats")
    c = lambda t: t.detach().cpu().numpy().astype(np.float32)  # noqa: E731
    xyz, dc, op = c(trainer.means), c(trainer.texels()[:n]), c(trainer.opacities).reshape(n)
    rest = c(trainer.features_rest.detach().transpose(1, 2).reshape(n, -1)) if trainer.features_rest.numel() else \
        np.zeros((n, 0), np.float32)
    ls, q = c(trainer.scales), c(trainer.quats)
    zeros = np.zeros(n, np.float32)
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "nx": zeros, "ny": zeros, "nz": zeros}
    cols.update({f"f_dc_{k}": dc[:, k] for k in range(3)})
    cols.update({f"f_rest_{k}": rest[:, k] for k in range(rest.shape[1])})
    cols["opacity"] = op
    cols.update({f"scale_{k}": ls[:, k] for k in range(2)})
    cols.update({f"rot_{k}": q[:, k] for k in range(4)})
    write_ply(path, {k: np.ascontiguousarray(v) for k, v in cols.items()}, binary=True)


def export_mesh_ply(trainer, views, path, **kw):
    """GStexTrainer.extract_mesh(views, **kw) written as a triangle-mesh PLY (gstex_amd.ply.write_mesh_ply): the
    lineage's second deliverable next to the checkpoint PLY.  -> (vertices, colors, faces) as extract_mesh returns
    them."""
    from .ply import write_mesh_ply

    vertices, colors, faces = trainer.extract_mesh(views, **kw)
    write_mesh_ply(path, vertices.cpu().numpy(), faces.cpu().numpy(),
                   None if colors is None else colors.cpu().numpy())
    return vertices, colors, faces


def score_mesh_ply(trainer, views, reference_ply, **kw) -> dict:
    """GStexTrainer.score_mesh(views, reference, **kw) with the reference point cloud read from a PLY (its x y z
    columns, gstex_amd.ply.read_ply)."""
    from .ply import read_ply

    cols = read_ply(reference_ply)
    missing = [c for c in ("x", "y", "z") if c not in cols]
    if missing:
        raise ValueError(f"{reference_ply}: no property {missing[0]!r} (has {', '.join(cols) or 'none'})")
    ref = np.stack([np.asarray(cols[c], np.float32) for c in ("x", "y", "z")], axis=1)
    return trainer.score_mesh(views, torch.from_numpy(ref), **kw)


def cluster_ply(ply_in, ply_out, eps, min_pts, sh_degree: int = 3, fix_init: bool = False, report=None,
                device=None):
    """The reference's demo_ballquery_dbscan.py as a function: read a 2DGS checkpoint PLY
    (gstex_amd.init.scene_from_2dgs_ply), cluster its splats (gstex_amd.cluster.dbscan on the scene's activation; on
    `device`, default the HIP device when there is one), and write a point PLY of the centres: float x y z, int
    `label` (1..K, -1 noise) and uchar red green blue from cluster.label_colors' fixed hash.  report: a path for
    cluster.cluster_report's text (opacities activated, the two in-plane scales).  -> the ClusterResult."""
    from .cluster import cluster_report, dbscan, label_colors
    from .init import scene_from_2dgs_ply
    from .ply import write_ply

    scene = scene_from_2dgs_ply(ply_in, sh_degree=sh_degree, fix_init=fix_init)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    with torch.no_grad():
        means, scales, quats, opacities = (t.to(device) for t in scene.activated())
        res = dbscan(means, scales[:, :2], quats, eps, min_pts)
        if report is not None:
            cluster_report(report, res, means, opacities, scales[:, :2])
    xyz = means.cpu().numpy().astype(np.float32)
    rgb = label_colors(res.labels)
    write_ply(ply_out, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "label": res.labels.cpu().numpy().astype(np.int32),
                        "red": rgb[:, 0], "green": rgb[:, 1], "blue": rgb[:, 2]}, binary=True)
    return res


def trainer_from_npz(path, device, **trainer_kwargs):
    """A GStexTrainer holding exactly the exported parameters (fresh optimizer state)."""
    from .model import GStexTrainer
    from .scene import Scene

    d = load_npz(path)
    n = d["xyz"].shape[0]
    zeros = torch.zeros((n, 3), dtype=torch.float32)
    scene = Scene(means=d["xyz"], log_scales=d["scaling"], quats=d["rotation"], opacity_logits=d["opacity"],
                  features_dc=zeros, features_rest=d["features_rest"], rgbs=zeros,
                  texture_dims=d["texture_dims"].to(torch.int32), mappings=d["mappings"],
                  texture=SH2RGB(d["texture_dc"]), pixel_scale=float("nan"))
    tr = GStexTrainer(scene, device, pixel_num=float(d["texture_dc"].shape[0]), **trainer_kwargs)
    with torch.no_grad():  # the raster-space round trip SH2RGB -> (x - 0.5) / C0 is not exact: copy the DC
        tr.texture_dc.copy_(d["texture_dc"].to(tr.device))
    return tr
