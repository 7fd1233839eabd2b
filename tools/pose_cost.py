#!/usr/bin/env python3
"""What the camera pose gradient costs (EXPERIMENTS.md, "Camera pose gradient").

At cfg3 size (200k splats, 1e7 texels, 800x800, pose 0), on one HIP device:

  kernels   gstex_raster_viewmat_bwd (raster mode with the folded centre chain, on the accumulator rows of a real
            backward; and the centre-only mode) and gstex_sh_dirs_bwd (degree 3, the DC-less rest layout): each call
            repeated in place inside a real per-op backward (its buffers alive), timing events on the launch stream
            around each repetition, warm-up, then the median of --reps repetitions with the p10-p90 spread.  gstex_raster_setup_bwd on the same buffers is timed alongside as the yardstick (the chain the new
            kernel repeats part of).
  step      a per-op training step (zero_grad, forward_backward, optimizer_step; fused_step=False) on a constant view
            and on a PoseRefiner view with the regulariser and refiner.step(), taking turns step by step; events around
            each step, warm-up, median and spread.

Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, warmup, reps, dev):
    """{name: fn} taking turns call by call -> {name: median / p10 / p90 / min in ms} from device events."""
    from gstex_amd._lib import TimingEvent

    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = TimingEvent(), TimingEvent()
            a.record(dev)
            fn()
            b.record(dev)
            events[name].append((a, b))
    torch.cuda.synchronize()
    return {name: _stats(ev) for name, ev in events.items()}


def _stats(events):
    v = sorted(a.elapsed_time(b) for a, b in events)
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
            "p90_ms": round(v[(9 * len(v)) // 10], 4), "min_ms": round(v[0], 4)}


def time_kernels(tr, view, gt, warmup, reps):
    """One real per-op pose step; each of the three C calls is repeated in place -- inside the backward that issues it,
    while every buffer its arguments point at is alive -- with an event pair around each repetition.  The calls only
    read their inputs and overwrite their outputs (accumulator mode), so a repetition computes the same values."""
    from gstex_amd import _lib, ops
    from gstex_amd._lib import TimingEvent
    from gstex_amd.pose import PoseRefiner

    dev = tr.device
    events = {}
    orig = ops._launch

    def repeat(label, name, *args):
        for _ in range(warmup):
            _lib.call(name, *args)
        ev = events.setdefault(label, [])
        for _ in range(reps):
            a, b = TimingEvent(), TimingEvent()
            a.record(dev)
            _lib.call(name, *args)
            b.record(dev)
            ev.append((a, b))

    def timed_launch(name, *args):
        orig(name, *args)
        if name in ("gstex_raster_setup_bwd", "gstex_raster_viewmat_bwd", "gstex_sh_dirs_bwd"):
            repeat(name, name, *args)
        if name == "gstex_raster_viewmat_bwd":
            # centre-only mode on the same splats: a seeded centre gradient, outputs into the same workspace / result
            n = tr.means.shape[0]
            v_centers = torch.randn((n, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            real = args[0]._obj
            result = torch.empty((3, 4), device=dev, dtype=torch.float32)
            centre = _lib.GstexRasterViewmatBwdArgs.from_buffer_copy(real)
            centre.partials, centre.row_flags = None, None
            centre.v_centers, centre.v_viewmat = v_centers.data_ptr(), result.data_ptr()
            repeat("gstex_raster_viewmat_bwd_centre_only", name, ctypes.byref(centre), args[1])
            torch.cuda.synchronize()  # (v_centers / result are released when this returns)

    ops._launch = timed_launch
    try:
        r = PoseRefiner(1, dev, accumulate=1)
        tr.zero_grad()
        tr.forward_backward(r.view(0, view), gt)
        torch.cuda.synchronize()
    finally:
        ops._launch = orig
    assert len(events) == 4, sorted(events)
    return {k: _stats(v) for k, v in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=200_000)
    ap.add_argument("--texels", type=float, default=1e7)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_cost.py needs a HIP device: its numbers are device times")

    from gstex_amd.model import GStexTrainer
    from gstex_amd.pose import PoseRefiner
    from gstex_amd.scene import make_scene, sphere_view

    dev = torch.device("cuda", 0)
    sc = make_scene(a.splats, a.texels, seed=42)
    view = sphere_view(0, a.size, a.size).to(dev)
    gt = torch.rand((a.size, a.size, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    tr = GStexTrainer(sc, dev, start_step=3000, fused_step=False)
    res = {"splats": a.splats, "texels": a.texels, "size": a.size, "reps": a.reps,
           "kernels": time_kernels(tr, view, gt, a.warmup, a.reps)}

    refiner = PoseRefiner(1, dev, accumulate=1)

    def step_const():
        tr.zero_grad()
        tr.forward_backward(view, gt)
        tr.optimizer_step()

    def step_pose():
        tr.zero_grad()
        tr.forward_backward(refiner.view(0, view), gt, extra_loss=refiner.regulariser())
        tr.optimizer_step()
        refiner.step()

    res["step"] = timed({"per_op_step": step_const, "per_op_step_with_pose": step_pose}, a.warmup, a.reps, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
