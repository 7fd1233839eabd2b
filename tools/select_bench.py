#!/usr/bin/env python3
"""Microbenchmark of the splat selection (EXPERIMENTS.md, "Selecting splats").

--splats charts with h, w uniform in [1, 13] (about 49 texels each, so 200 000 splats hold about 1e7 texels) laid out
in splat order, three (T, 3) float32 texel tensors (a parameter and its two Adam moments), keep every other splat.
Prints the steps' times by timing events (the plan with its two scans and the read-back, the dims, the jagged gather of
the three tensors in one launch, alone and as the mean of --burst launches back to back), the wall-clock total of gstex_amd.select.select_texture and of its eager twin
(select_texture_eager) on the same device tensors, each the median over --reps, the gather's byte floor (every kept
texel of three tensors read once and written once, 2 x 3 x 12 T_new bytes, at 6.3 TB/s) and whether kernels and twin
agree.  Prints one JSON line (progress goes to stderr)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12  # achievable on an MI355X


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return round(statistics.median(out), 3), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=20, help="back-to-back launches of the gather per timed window")
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("select_bench.py needs a HIP device")
    from gstex_amd import _lib
    from gstex_amd import select as sel

    dev = torch.device("cuda", 0)
    n = args.splats
    g = torch.Generator().manual_seed(args.seed)
    hw = torch.randint(1, 14, (n, 2), generator=g)
    size = hw[:, 0] * hw[:, 1]
    dims = torch.cat([hw, (torch.cumsum(size, 0) - size)[:, None]], 1).to(torch.int32).to(dev)
    T = int(size.sum())
    keep = (torch.arange(n) % 2 == 0).to(dev)
    tensors = [torch.randn((T, 3), generator=g).to(dev) for _ in range(3)]
    print(f"{n} splats, {T} texels", file=sys.stderr, flush=True)

    run = lambda: sel.select_texture(dims, T, keep, tensors)  # noqa: E731
    twin = lambda: sel.select_texture_eager(dims, T, keep, tensors)  # noqa: E731
    run(), twin()  # warm-up: library load, allocator
    steps = []
    for _ in range(args.reps):
        ev = [_lib.TimingEvent() for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record(dev)
        plan = sel.plan_selection(dims, T, keep)
        ev[1].record(dev)
        new_dims, src_off = sel.select_dims(dims, plan)
        ev[2].record(dev)
        sel.select_texels(new_dims, src_off, T, plan.n_texels_new, tensors)
        ev[3].record(dev)
        torch.cuda.synchronize()
        steps.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
    plan_ms, dims_ms, single_ms = (round(statistics.median(s[k] for s in steps), 4) for k in range(3))
    # one launch between two events also counts the time the device waits for the host to reach the launch; the
    # kernel's own time: --burst launches back to back into the same destinations, so that the queue stays full
    outs = [torch.empty((plan.n_texels_new, 3), device=dev) for _ in tensors]
    bursts = []
    for _ in range(args.reps):
        e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
        torch.cuda.synchronize()
        e0.record(dev)
        for _ in range(args.burst):
            sel.select_texels(new_dims, src_off, T, plan.n_texels_new, tensors, lambda k, shape: outs[k])
        e1.record(dev)
        torch.cuda.synchronize()
        bursts.append(e0.elapsed_time(e1) / args.burst)
    texels_ms = round(statistics.median(bursts), 4)
    kernels_ms, got = wall(run, args.reps)
    twin_ms, want = wall(twin, args.reps)
    t_new = got[2]
    moved = 2 * 3 * 12 * t_new
    floor_ms = 1e3 * moved / HBM_BYTES_PER_S
    res = {"splats": n, "texels": T, "kept_splats": int(got[0].shape[0]), "kept_texels": t_new, "reps": args.reps,
           "burst": args.burst, "plan_scans_readback_ms": plan_ms, "dims_ms": dims_ms,
           "texels_single_launch_ms": single_ms, "texels_ms": texels_ms,
           "texels_tb_per_s": round(moved / (1e-3 * texels_ms) / 1e12, 3), "byte_floor_ms": round(floor_ms, 4),
           "texels_over_floor": round(texels_ms / floor_ms, 2), "select_texture_ms": kernels_ms,
           "eager_twin_ms": twin_ms, "ratio_twin_over_kernels": round(twin_ms / kernels_ms, 2),
           "equal": bool(torch.equal(got[0], want[0]) and got[2] == want[2]
                         and all(torch.equal(a, b) for a, b in zip(got[1], want[1])))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
