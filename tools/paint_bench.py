#!/usr/bin/env python3
"""Microbenchmark of painting (EXPERIMENTS.md, "Paint").

At cfg3 (200k splats, 1e7 texels, 800x800, pose 0) two strokes -- a thin polyline over about 1 % of the pixels and a
full-coverage one, as uint8 canvases -- each painted two ways:

  reference   GStexModel.draw_from_view's call sequence through gstex_cuda (gstex.py:489-606): torch activations,
              project_points / get_aabb_2d / get_num_tiles_hit_2d, texture_gaussians, depth -+ 1e-2, texture_edit, the
              three-line blend.  Needs nothing of this script's commit but gstex_cuda: `--only reference` runs on
              older checkouts.
  paint       GStexTrainer.paint.

and a replay of 8 edits (the polyline from poses 0..7): the reference's update_edit_texture loop against
GStexTrainer.edit_texture.  Timing events on the launch stream around each call, the two ways taking turns call by
call so neither runs on an idle device; warm-up, then the median of --reps repetitions with the p10-p90 spread.
paint_launch_ms: the median device time of each launch inside GStexTrainer.paint, from a separate loop.  Prints one
JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SH_C0 = 0.28209479177387814


def polyline_canvas(H, W, width=5.0, colour=(255, 0, 255)):
    """A uint8 RGBA canvas with a zig-zag polyline of the given width (opaque on transparent)."""
    pts = torch.tensor([[0.10, 0.15], [0.85, 0.30], [0.20, 0.55], [0.90, 0.80]]) * torch.tensor([W, H])
    yy, xx = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    p = torch.stack([xx, yy], -1)
    dist = torch.full((H, W), float("inf"))
    for a, b in zip(pts[:-1], pts[1:]):
        ab = b - a
        t = (((p - a) * ab).sum(-1) / (ab * ab).sum()).clamp(0, 1)
        dist = torch.minimum(dist, (p - (a + t[..., None] * ab)).norm(dim=-1))
    canvas = torch.zeros(H, W, 4, dtype=torch.uint8)
    canvas[dist <= width / 2] = torch.tensor([*colour, 255], dtype=torch.uint8)
    return canvas


def full_canvas(H, W, colour=(0, 255, 0)):
    canvas = torch.zeros(H, W, 4, dtype=torch.uint8)
    canvas[...] = torch.tensor([*colour, 255], dtype=torch.uint8)
    return canvas


@torch.no_grad()
def draw_from_view(tr, view, cur_texture, canvas):
    """gstex.py:427-437 + 489-606 for one edit, on the trainer's parameters."""
    import gstex_cuda
    from gstex_amd.charts import get_uv_mapping

    change_img = canvas.float() / 255.0
    means = tr.means.detach()
    quats = tr.quats / tr.quats.norm(dim=-1, keepdim=True)
    scales = torch.zeros_like(tr.scales)
    scales[:, :-1] = torch.clamp(torch.exp(tr.scales[:, :-1]), min=1e-9)
    scales[:, -1] = 1e-5 * torch.mean(scales[:, :-1], dim=-1)
    opacities = torch.sigmoid(tr.opacities)
    uv0, umap, vmap = get_uv_mapping(quats, tr.mappings)
    intr = (view.fx, view.fy, view.cx, view.cy)
    H, W = view.H, view.W
    _, depths = gstex_cuda.project_points(means, view.viewmat, intr)
    centers, extents = gstex_cuda.get_aabb_2d(means, scales, 1, quats, view.viewmat, intr)
    nth = gstex_cuda.get_num_tiles_hit_2d(centers, extents, H, W, 16)
    n = means.shape[0]
    cam = (view.viewmat, view.c2w, view.fx, view.fy, view.cx, view.cy, H, W, 16)
    bg = torch.zeros(3, device=means.device)
    outputs = gstex_cuda.texture_gaussians((n, 1, 3), tr.texture_dims, centers, extents, depths, nth,
                                           torch.sigmoid(means), opacities, means, scales, 1, quats, uv0, umap, vmap,
                                           cur_texture, *cam, tr.settings, background=bg)
    depth_output = outputs[1]
    depth_lower = depth_output - 1e-2
    depth_upper = depth_output + 1e-2
    updated = gstex_cuda.texture_edit((n, 1, 5), tr.texture_dims, change_img[:, :, :3], change_img[:, :, 3:],
                                      depth_lower, depth_upper, centers, extents, depths, nth, opacities, means, scales,
                                      1, quats, uv0, umap, vmap, *cam, 1 << 13, background=bg)
    weight = updated[:, 3:4] / (updated[:, 4:] + 1e-6)
    edit_rgb_texture = updated[:, :3] / (updated[:, 3:4] + 1e-6)
    return edit_rgb_texture * weight + cur_texture * (1 - weight)


def timed(fns, warmup, reps, dev):
    from gstex_amd._lib import TimingEvent

    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in fns}
    for _ in range(reps):  # the ways take turns; one synchronisation at the end
        for name, fn in fns.items():
            a, b = TimingEvent(), TimingEvent()
            a.record(dev)
            fn()
            b.record(dev)
            events[name].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for name, ev in events.items():
        v = sorted(a.elapsed_time(b) for a, b in ev)
        out[name] = {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
                     "p90_ms": round(v[(9 * len(v)) // 10], 4), "min_ms": round(v[0], 4)}
    return out


def launch_split(tr, view, canvas, reps):
    """Median device time of each timed launch inside GStexTrainer.paint (event pairs around the C calls)."""
    from gstex_amd import ops

    ops.set_kernel_timing(True, ("gstex_bin_sort", "gstex_raster_setup", "gstex_raster_fwd", "gstex_paint_scatter",
                                 "gstex_paint_blend"))
    for _ in range(reps):
        tr.paint(view, canvas)
    times = ops.kernel_times()
    ops.set_kernel_timing(False)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=200_000)
    ap.add_argument("--texels", type=float, default=1e7)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--edits", type=int, default=8)
    ap.add_argument("--only", choices=["reference", "paint"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("paint_bench.py needs a HIP device")
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    dev = torch.device("cuda", 0)
    H = W = args.size
    tr = GStexTrainer(make_scene(args.splats, args.texels, seed=args.seed), dev, start_step=3000)
    views = [sphere_view(i, H, W, n_views=8).to(dev) for i in range(8)]
    thin, full = polyline_canvas(H, W).to(dev), full_canvas(H, W).to(dev)
    edits = [(views[i % 8], thin) for i in range(args.edits)]

    def base():
        return tr.texture_dc.detach()[:tr.n_texels] * SH_C0 + 0.5

    def replay_reference():
        tex = base()
        for view, canvas in edits:
            tex = draw_from_view(tr, view, tex, canvas)
        return tex

    def ways(ref, new):
        return {k: f for k, f in (("reference", ref), ("paint", new)) if args.only in (None, k)}

    res = {"splats": args.splats, "texels": int(tr.n_texels), "H": H, "W": W, "warmup": args.warmup, "reps": args.reps,
           "edits": args.edits, "thin_stroke_pixel_share": round(float((thin[..., 3] > 0).float().mean()), 5)}
    res["thin_stroke"] = timed(ways(lambda: draw_from_view(tr, views[0], base(), thin),
                                    lambda: tr.paint(views[0], thin)), args.warmup, args.reps, dev)
    res["full_stroke"] = timed(ways(lambda: draw_from_view(tr, views[0], base(), full),
                                    lambda: tr.paint(views[0], full)), args.warmup, args.reps, dev)
    res["replay"] = timed(ways(replay_reference, lambda: tr.edit_texture(edits)), args.warmup, args.reps, dev)
    if args.only is None:  # the two ways paint the same texels to the same colours (float atomics: last bits)
        a, b = draw_from_view(tr, views[0], base(), thin), tr.paint(views[0], thin)
        res["thin_stroke_max_abs_difference"] = float((a - b).abs().max())
        res["paint_launch_ms"] = {"thin_stroke": launch_split(tr, views[0], thin, args.reps),
                                  "full_stroke": launch_split(tr, views[0], full, args.reps)}
        res["thin_stroke_texels_changed"] = [int((a != base()).any(-1).sum()), int((b != base()).any(-1).sum())]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
