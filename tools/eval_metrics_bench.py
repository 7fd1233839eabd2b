#!/usr/bin/env python3
"""Microbenchmark of the evaluation metrics (EXPERIMENTS.md, "evaluation metrics").

  --mode metrics   gstex_eval_metrics on a uint8 RGBA target (raw C-ABI call, preallocated buffers) next to
                   gstex_loss_target_fwd on the same inputs, then the Python routes: image_metrics against the eager
                   twin (the composite with torch ops, then image_metrics_eager).
  --mode render    the evaluation's render (one raster call: GStexTrainer.render under no_grad, no geometry outputs)
                   against eval_render's three, and GStexTrainer.evaluate as a whole.

Timing events (gstex_amd._lib.TimingEvent); warm-up, then the median over --reps timed windows of --inner calls
each, the measured functions taking turns window by window.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, warmup, reps, inner, dev):
    from gstex_amd._lib import TimingEvent

    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = TimingEvent(), TimingEvent()
            a.record(dev)
            for _ in range(inner):
                fn()
            b.record(dev)
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / inner)
    out = {}
    for name, v in ms.items():
        v.sort()
        out[name] = {"median_us": round(1e3 * statistics.median(v), 2), "p10_us": round(1e3 * v[len(v) // 10], 2),
                     "p90_us": round(1e3 * v[(9 * len(v)) // 10], 2)}
    return out


def inputs(H, W, C, dev):
    g = torch.Generator().manual_seed(1)
    img = (torch.rand(H, W, 3, generator=g) * 1.2 - 0.1).to(dev)
    tex = (torch.rand(H, W, C, generator=g) * 0.3).to(dev)
    alpha = torch.rand(H, W, generator=g).to(dev)
    bg = torch.rand(3, generator=g).to(dev)
    rgba = torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8).to(dev)
    return img, tex, alpha, bg, rgba


def metric_calls(H, W, C, dev):
    from gstex_amd import _lib
    from gstex_amd.loss import _cwin, image_metrics, image_metrics_eager

    lib = _lib.load()
    img, tex, alpha, bg, rgba = inputs(H, W, C, dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    st = _lib.stream_of(dev)
    win = _cwin()
    out = torch.empty(4, device=dev)
    rgb, gto = torch.empty(H, W, 3, device=dev), torch.empty(H, W, 3, device=dev)
    u8 = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    ws_m = torch.empty(int(lib.gstex_eval_metrics_workspace_size(H, W)), dtype=torch.uint8, device=dev)
    ws_t = torch.empty(int(lib.gstex_loss_target_workspace_size(H, W)), dtype=torch.uint8, device=dev)
    target = _lib.GstexLossTarget(p(rgba), None, _lib.GT_U8, 4, _lib.MASK_F32, 0)

    def kernel_metrics():
        _lib.call("gstex_eval_metrics", H, W, C, p(img), p(tex), p(alpha), p(bg), ctypes.byref(target), win, p(rgb),
                  p(u8), p(gto), p(out), p(ws_m), ws_m.numel(), st)

    def kernel_metrics_no_images():
        _lib.call("gstex_eval_metrics", H, W, C, p(img), p(tex), p(alpha), p(bg), ctypes.byref(target), win, None,
                  None, None, p(out), p(ws_m), ws_m.numel(), st)

    def kernel_loss_target_fwd():
        _lib.call("gstex_loss_target_fwd", H, W, C, p(img), p(tex), p(alpha), p(bg), ctypes.byref(target), win, 0.2,
                  p(rgb), p(gto), p(out), p(ws_t), ws_t.numel(), st)

    def py_image_metrics():
        image_metrics(img, tex, alpha, bg, rgba)

    def py_eager():
        comp = torch.clamp(img + tex[:, :, 0:3] + (1 - alpha[:, :, None]) * bg[None, None, :], 0.0, 1.0)
        image_metrics_eager(comp, bg, rgba)

    return {"gstex_eval_metrics": kernel_metrics, "gstex_eval_metrics_no_images": kernel_metrics_no_images,
            "gstex_loss_target_fwd": kernel_loss_target_fwd, "image_metrics": py_image_metrics,
            "composite_then_image_metrics_eager": py_eager}


def render_calls(H, W, n, texels, dev):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    tr = GStexTrainer(make_scene(n, texels, seed=9), dev, start_step=3000, background="random")
    view = sphere_view(1, H, W).to(dev)
    rgba = inputs(H, W, 3, dev)[4]

    def plain_render():
        with torch.no_grad():
            tr.render(view, composite=False, geometry=False)

    return {"evaluate_render_one_raster_call": plain_render, "eval_render_three_raster_calls":
            lambda: tr.eval_render(view), "evaluate": lambda: tr.evaluate(view, rgba)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["metrics", "render"], default="metrics")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--splats", type=int, default=100_000)
    ap.add_argument("--texels", type=float, default=2_000_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_metrics_bench.py needs a HIP device")
    dev = torch.device("cuda", 0)
    H = W = args.size
    res = {"mode": args.mode, "H": H, "W": W, "C": args.channels, "warmup": args.warmup, "reps": args.reps,
           "inner": args.inner}
    if args.mode == "metrics":
        res.update(timed(metric_calls(H, W, args.channels, dev), args.warmup, args.reps, args.inner, dev))
    else:
        res.update(splats=args.splats, texels=args.texels)
        res.update(timed(render_calls(H, W, args.splats, args.texels, dev), args.warmup, args.reps, args.inner, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
