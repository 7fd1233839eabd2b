#!/usr/bin/env python3
"""Microbenchmark of the grid nearest-neighbour search (EXPERIMENTS.md, "Nearest neighbours").

Times, on points sampled near a surface (a bumpy sphere with 0.2 % noise, the shape of a scan or of mesh samples):
  * PointGrid(points): the build (bounds read-back, count, scan, place);
  * PointGrid.query(queries, k) for --k neighbours: the queries ordered by cell (count, scan, place on them) and
    gstex_nn_query; and the gstex_nn_query launch alone on ordered and on unordered queries;
  * knn_mean_dist_device at --knn-points uniform points in a cube (the initialisation's case);
against scipy's cKDTree on this machine's host (build, and query with workers=16), which is what users have without
it.  --cell-scales sweeps the cell size around the default.  Wall-clock around a device synchronisation for the
Python routes, timing events for the single launch; the median over --reps.  The device's distances are checked against
the host tree's.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface_points(n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn((n, 3), generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    r = 1.0 + 0.15 * torch.sin(5 * d[:, 0]) * torch.cos(4 * d[:, 1]) + 0.1 * torch.sin(7 * d[:, 2])
    p = d * r[:, None] + 0.002 * torch.randn((n, 3), generator=g, dtype=torch.float64)
    return p.float().contiguous()


def wall(fn, reps, sync=True):
    out = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        if sync:
            torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return round(statistics.median(out), 3), r


def event_ms(fn, reps, dev):
    from gstex_amd._lib import TimingEvent

    out = []
    for _ in range(reps):
        a, b = TimingEvent(), TimingEvent()
        a.record(dev)
        fn()
        b.record(dev)
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--knn-points", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=1, help="neighbours per query (1..8)")
    ap.add_argument("--cell-scales", type=str, default="1")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nn_bench.py needs a HIP device")
    from gstex_amd import neighbors as N

    dev = torch.device("cuda", 0)
    P, Q = surface_points(args.points, 1), surface_points(args.queries, 2)
    Pd, Qd = P.to(dev), Q.to(dev)
    res = {"points": args.points, "queries": args.queries, "k": args.k, "knn_points": args.knn_points,
           "reps": args.reps, "workers": args.workers}
    N.PointGrid(Pd).query(Qd[:1000])  # warm-up: library load, allocator
    base = N.PointGrid(Pd)
    sweep = []
    d2_dev = None
    for scale in [float(s) for s in args.cell_scales.split(",")]:
        h = base.cell_size * scale
        build_ms, grid = wall(lambda: N.PointGrid(Pd, cell_size=h), args.reps)
        query_ms, (d2, _) = wall(lambda: grid.query(Qd, k=args.k), args.reps)
        _, qrec = N.grid_build(Qd, grid.origin, grid.cell_size, grid.dims)
        plain = torch.cat([Qd, torch.arange(Qd.shape[0], device=dev, dtype=torch.int32).view(torch.float32)[:, None]],
                          1).contiguous()
        launch = lambda q: N.nn_query(grid.origin, grid.cell_size, grid.dims, grid.cell_start, grid.records, q,  # noqa: E731
                                      k=args.k)
        cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
        occupied = int((grid.cell_start[1:] > grid.cell_start[:-1]).sum())
        sweep.append({"cell_scale": scale, "cell_size": grid.cell_size, "dims": grid.dims, "cells": cells,
                      "points_per_occupied_cell": round(args.points / max(occupied, 1), 2), "build_ms": build_ms,
                      "query_ms": query_ms, "query_kernel_ordered_ms": event_ms(lambda: launch(qrec), args.reps, dev),
                      "query_kernel_unordered_ms": event_ms(lambda: launch(plain), args.reps, dev)})
        if scale == 1.0:
            d2_dev = d2
    res["device"] = sweep
    Kd = (torch.rand((args.knn_points, 3), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    res["knn_mean_dist_device_ms"], knn_dev = wall(lambda: N.knn_mean_dist_device(Kd, 3), args.reps)
    if not args.skip_host:
        from scipy.spatial import cKDTree

        p64, q64 = P.double().numpy(), Q.double().numpy()
        host_build, tree = wall(lambda: cKDTree(p64), 1, sync=False)
        host_query, (dd, _) = wall(lambda: tree.query(q64, k=1, workers=args.workers), 1, sync=False)
        k64 = Kd.cpu().double().numpy()
        host_knn, hk = wall(lambda: cKDTree(k64).query(k64, k=4, workers=args.workers)[0][:, 1:].mean(-1), 1, sync=False)
        res["host"] = {"build_ms": host_build, "query_ms": host_query, "knn_mean_dist_ms": host_knn}
        one = next((s for s in sweep if s["cell_scale"] == 1.0), sweep[0])
        res["ratio_host_over_device"] = {
            "build": round(host_build / one["build_ms"], 2), "query": round(host_query / one["query_ms"], 2),
            "build_and_query": round((host_build + host_query) / (one["build_ms"] + one["query_ms"]), 2),
            "knn_mean_dist": round(host_knn / res["knn_mean_dist_device_ms"], 2)}
        if d2_dev is not None:
            got = np.sqrt(d2_dev[:, 0].double().cpu().numpy())
            res["max_rel_distance_error_vs_host"] = float(np.abs(got / np.maximum(dd, 1e-300) - 1)[dd > 0].max())
        res["max_rel_knn_error_vs_host"] = float(np.abs(knn_dev.double().cpu().numpy() / hk - 1).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
