"""Density control at the flagship size (EXPERIMENTS.md "Density control"): 200k one-texel splats, 800x800.

  --mode step    the training step with DensityController.accumulate on and off, alternated block by block in one call
  --mode event   one clone / split / prune event (plan, scan, read-back, apply, trainer rebuild) with its byte count
  --mode kernel  a loop of accumulate launches alone, for `rocprofv3 --kernel-trace --stats -- python tools/...`
                 (kernel name: density_accum_kernel)

Prints one JSON line per measurement.  Needs a HIP device; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(n, H, W, seed):
    from gstex_amd import density as dn
    from gstex_amd.init import _one_texel_scene
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    dev = torch.device("cuda", 0)
    sc = make_scene(n, 0, seed=seed)
    one = _one_texel_scene(sc.means, sc.log_scales, sc.quats, sc.opacity_logits, sc.features_dc, sc.features_rest)
    tr = GStexTrainer(one, dev, defer_texture=True, start_step=3000)
    views = [sphere_view(i, H, W, n_views=8).to(dev) for i in range(8)]
    g = torch.Generator().manual_seed(seed)
    gts = [torch.rand((H, W, 3), generator=g).to(dev) for _ in range(2)]
    ctl = dn.DensityController(n, dev, dn.scene_extent(views))
    return tr, views, gts, ctl


def steps(tr, views, gts, ctl, k, accumulate):
    for i in range(k):
        v = views[i % len(views)]
        tr.zero_grad()
        tr.forward_backward(v, gts[i % len(gts)])
        if accumulate:
            ctl.accumulate(tr, v)
        tr.optimizer_step()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("step", "event", "kernel"), default="step")
    p.add_argument("--n-splats", type=int, default=200_000)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=800)
    p.add_argument("--steps", type=int, default=50, help="steps per timed block")
    p.add_argument("--blocks", type=int, default=6, help="timed blocks per setting, alternated")
    p.add_argument("--warmup", type=int, default=30)
    p.add_argument("--seed", type=int, default=42)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_bench: no HIP device")
    n = a.n_splats
    tr, views, gts, ctl = build(n, a.height, a.width, a.seed)
    sync = torch.cuda.synchronize
    steps(tr, views, gts, ctl, a.warmup, True)
    sync()
    if a.mode == "step":
        ms = {False: [], True: []}
        for _ in range(a.blocks):
            for on in (False, True):
                sync()
                t0 = time.perf_counter()
                steps(tr, views, gts, ctl, a.steps, on)
                sync()
                ms[on].append(1e3 * (time.perf_counter() - t0) / a.steps)
        med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
        print(json.dumps({"measure": "train step ms, accumulate off / on (alternated blocks)", "n": n,
                          "H": a.height, "W": a.width, "steps_per_block": a.steps, "off_ms": ms[False],
                          "on_ms": ms[True], "off_median_ms": med(ms[False]), "on_median_ms": med(ms[True]),
                          "skipped_steps": len(tr.skipped_steps)}))
    elif a.mode == "kernel":
        tr.zero_grad()
        tr.forward_backward(views[0], gts[0])
        for _ in range(200):
            ctl.accumulate(tr, views[0])
        sync()
        # per splat: means 12 + gradient 12 + num_tiles_hit 4 + extents 8 + the three statistics 12 read, 12 written
        print(json.dumps({"measure": "accumulate launches for a kernel trace", "n": n, "launches": 200,
                          "bytes_read_per_splat": 48, "bytes_written_per_splat": 12}))
        tr.optimizer_step()
    else:
        from gstex_amd import density as dn

        g = torch.Generator().manual_seed(a.seed)
        out = []
        for rep in range(3):
            m = tr.means.shape[0]
            count = torch.full((m,), 4.0)
            grad_sum = torch.where(torch.rand(m, generator=g) < 0.3, torch.ones(m), torch.zeros(m))  # 30 % hot
            noise = torch.randn((m, 2, 2), generator=g).to(tr.device)
            th = dn.density_thresholds(
                100.0 * float(torch.exp(tr.scales.detach()[:, :2].max(dim=1).values).median()))
            stats = [grad_sum.to(tr.device), count.to(tr.device), torch.zeros(m, device=tr.device)]
            floats = sum(t.numel() // t.shape[0] * (3 if tr.optimizer.state.get(t) else 1) for t in tr.parameters())
            sync()
            t0 = time.perf_counter()
            plan = tr.apply_density(*stats, noise, th, size_prune=False)
            sync()
            out.append({"n_before": m, "n_after": plan.n_new, "cloned": plan.cloned, "split": plan.split,
                        "pruned": plan.pruned, "event_ms": 1e3 * (time.perf_counter() - t0),
                        "floats_per_row": floats, "bytes_read": 4 * floats * (plan.kept + plan.cloned + plan.split)
                        + 12 * m, "bytes_written": 4 * floats * plan.n_new})
            steps(tr, views, gts, ctl.__class__(plan.n_new, tr.device, ctl.extent), 3, False)
        print(json.dumps({"measure": "density event (plan, scan, read-back, apply, rebuild), wall clock",
                          "events": out}))
    tr.wait_texture()
    sync()


if __name__ == "__main__":
    main()
