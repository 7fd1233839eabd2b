#!/usr/bin/env python3
"""Microbenchmark of the splat clustering (EXPERIMENTS.md, "Clustering the splats").

N splats on a sphere shell with a random rotation in the surface (tests/cluster_cases.sphere_shell_splats), a radius of
--radius mean spacings and --min-pts.  Prints, per --points value, each step's time by timing events (the grid build
with its bounds read-back, shapes, degree, link, roots, the scan of the root flags, assign) and the wall-clock total of
gstex_amd.cluster.dbscan, the median over --reps; and, at --twin-points, the brute-force twin (dbscan_eager) on the same
device next to the kernels, with the two results compared.  --cell-scales also times the whole call at multiples of
the default cell.  Prints one JSON line (progress goes to stderr)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--points", type=str, default="200000,1000000")
    ap.add_argument("--twin-points", type=int, default=50_000)
    ap.add_argument("--radius", type=float, default=1.4, help="sqrt(eps) in mean spacings")
    ap.add_argument("--min-pts", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cell-scales", type=str, default="", help="also time dbscan at these multiples of the default cell")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_bench.py needs a HIP device")
    from cluster_cases import sphere_shell_splats

    from gstex_amd import cluster as C

    dev = torch.device("cuda", 0)

    def splats(n):
        eps = (args.radius * math.sqrt(4 * math.pi / n)) ** 2
        return [t.to(dev) for t in sphere_shell_splats(n, 7)], eps

    s, eps = splats(10_000)
    C.dbscan(*s, eps, args.min_pts)  # warm-up: library load, allocator
    res = {"radius_spacings": args.radius, "min_pts": args.min_pts, "reps": args.reps, "sizes": []}
    for n in [int(v) for v in args.points.split(",")]:
        s, eps = splats(n)
        total_ms, r = wall(lambda: C.dbscan(*s, eps, args.min_pts), args.reps)
        steps = []
        for _ in range(args.reps):
            t = {}
            C.dbscan_device(*C._splats(*s), C._f32(eps), args.min_pts, timings=t)
            steps.append(t)
        row = {k: round(statistics.median(t[k] for t in steps), 3) for k in steps[0] if k.endswith("_ms")}
        row.update(points=n, eps=eps, cell_size=steps[0]["cell_size"], dims=steps[0]["dims"], total_ms=total_ms,
                   n_clusters=r.n_clusters, cores=int(r.core.sum()), noise=int((r.labels == -1).sum()),
                   mean_degree=round(float(r.degree.float().mean()), 2))
        for scale in [float(v) for v in args.cell_scales.split(",") if v]:
            h = steps[0]["cell_size"] * scale
            ms, rs = wall(lambda: C.dbscan(*s, eps, args.min_pts, cell_size=h), args.reps)
            row[f"total_ms_cell_x{scale:g}"] = ms
            assert torch.equal(rs.labels, r.labels)
        res["sizes"].append(row)
        print(f"{n} splats: {row}", file=sys.stderr, flush=True)
    if args.twin_points > 0:
        s, eps = splats(args.twin_points)
        print(f"the twin at {args.twin_points} splats ...", file=sys.stderr, flush=True)
        twin_ms, want = wall(lambda: C.dbscan_eager(*s, eps, args.min_pts), 1)
        dev_ms, got = wall(lambda: C.dbscan(*s, eps, args.min_pts), args.reps)
        res["twin"] = {"points": args.twin_points, "twin_ms": twin_ms, "kernels_ms": dev_ms,
                       "ratio_twin_over_kernels": round(twin_ms / dev_ms, 1),
                       "equal": bool(torch.equal(got.labels, want.labels) and torch.equal(got.degree, want.degree)
                                     and got.n_clusters == want.n_clusters)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
