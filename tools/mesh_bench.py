"""EXPERIMENTS.md "Mesh extraction": gstex_tsdf_integrate at 256^3 with colour for K = 1 and K = 8 views per launch,
tsdf_integrate_eager on the device for the same inputs, and the extraction at 256^3 on the analytic sphere.
    python tools/mesh_bench.py [N = 256] [record.json]      one JSON line"""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gstex_amd import _lib, mesh as M  # noqa: E402
from gstex_amd.scene import sphere_view  # noqa: E402

DEV = "cuda"
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
HW = 512
out = {"n": N}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = _lib.TimingEvent(), _lib.TimingEvent()
    a.record(DEV)
    for _ in range(reps):
        fn()
    b.record(DEV)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


# views of a sphere of radius 0.8 rendered analytically (depth of the front hit, alpha 1 inside the silhouette)
R = 0.8
views, renders = [], []
for q in range(8):
    v = sphere_view(q, HW, HW)
    ys, xs = torch.meshgrid(torch.arange(HW) + 0.5, torch.arange(HW) + 0.5, indexing="ij")
    d = torch.stack([(xs - v.cx) / v.fx, (ys - v.cy) / v.fy, torch.ones_like(xs)], -1)
    c = v.viewmat[:, 3]
    A, B, Cq = (d * d).sum(-1), -2 * (d * c).sum(-1), (c * c).sum() - R * R
    disc = B * B - 4 * A * Cq
    t = (-B - torch.sqrt(disc.clamp(min=0))) / (2 * A)
    alpha = (disc > 0).float()
    views.append(v.to(DEV))
    renders.append(dict(depth=(t * alpha).contiguous().to(DEV), alpha=alpha.contiguous().to(DEV),
                        rgb=torch.rand((HW, HW, 3)).to(DEV)))
h = 2.0 / (N - 1)
origin = (-1.0, -1.0, -1.0)
vol = M.TSDFVolume(DEV, origin, h, (N, N, N), 5 * h, color=True)
n_vox = N ** 3
floor_ms = 40.0 * n_vox / 8e12 * 1e3  # 20 B read + 20 B written per voxel at 8 TB/s
out["bytes_floor_ms_40B"] = floor_ms
def integrate(lo, hi):
    M.tsdf_integrate(vol.tsdf, vol.weight, vol.color, origin, h, views[lo:hi], renders[lo:hi], 5 * h)


# three alternated blocks: one view, eight views in one launch, eight launches of one view (device events)
out["integrate_K1_ms"], out["integrate_K8_ms"], out["integrate_8x_K1_ms"] = [], [], []
for _ in range(3):
    out["integrate_K1_ms"].append(timed(lambda: integrate(0, 1), 400))
    out["integrate_K8_ms"].append(timed(lambda: integrate(0, 8), 200))
    out["integrate_8x_K1_ms"].append(timed(lambda: [integrate(q, q + 1) for q in range(8)], 50))
touched = float((vol.weight > 0).float().mean())
out["fraction_of_voxels_some_view_reaches"] = touched
# the eager twin on the device, same inputs (it returns new tensors)
for K in (1, 8):
    fn = lambda: M.tsdf_integrate_eager(vol.tsdf, vol.weight, vol.color, origin, h, views[:K], renders[:K], 5 * h)  # noqa: E731
    out[f"eager_K{K}_ms"] = timed(fn, 20)
    torch.cuda.empty_cache()
# agreement at this size: kernel against the twin on the device, from a fresh volume
vol.reset()
ref = M.tsdf_integrate_eager(vol.tsdf, vol.weight, vol.color, origin, h, views, renders, 5 * h)
M.tsdf_integrate(vol.tsdf, vol.weight, vol.color, origin, h, views, renders, 5 * h)
out["kernel_vs_device_twin_mismatches"] = [int((a.view(torch.int32) != b.view(torch.int32)).sum())
                                           for a, b in zip((vol.tsdf, vol.weight, vol.color), ref)]
del ref
torch.cuda.empty_cache()

# extraction at N^3 on the analytic sphere r = 0.33 N h (no colour), whole call (mark, scans, read-back, emit)
ax = [torch.tensor(origin[c] + o, device=DEV) + h * torch.arange(N, device=DEV, dtype=torch.float32)
      for c, o in enumerate((0.0013, 0.0007, -0.0004))]
z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
r = 0.33 * N * h
tsdf = torch.clamp((torch.sqrt(x * x + y * y + z * z) - r) / (5 * h), -1.0, 1.0).contiguous()
weight = torch.ones_like(tsdf)
del x, y, z
Vx, _, Fx = M.mesh_extract(tsdf, weight, None, origin, h)
out["extract_V"], out["extract_F"] = int(Vx.shape[0]), int(Fx.shape[0])
out["extract_euler"] = int(Vx.shape[0]) - 3 * int(Fx.shape[0]) // 2 + int(Fx.shape[0])
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    M.mesh_extract(tsdf, weight, None, origin, h)
torch.cuda.synchronize()
out["extract_whole_call_ms_host_clock"] = (time.perf_counter() - t0) / 200 * 1e3
plan = M.mesh_extract_mark(tsdf, weight, None, origin, h)
a = plan.args
import ctypes  # noqa: E402
st = _lib.stream_of(torch.device(DEV))
out["extract_mark_ms"] = timed(lambda: _lib.call("gstex_mesh_extract_mark", ctypes.byref(a), st), 200)
Vb = torch.empty((plan.n_vertices, 3), device=DEV)
Fb = torch.empty((plan.n_faces, 3), device=DEV, dtype=torch.int32)
out["extract_emit_ms"] = timed(lambda: M.mesh_extract_emit(plan, Vb, None, Fb), 200)
print(json.dumps(out))
if len(sys.argv) > 2:  # also keep the record in a file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
