#!/usr/bin/env python3
"""Microbenchmark of the fused loss kernels (EXPERIMENTS.md, "dataset targets").

  --mode kernels [--lib PATH]   gstex_loss_fwd + gstex_loss_bwd through raw ctypes calls on any libgstex_hip.so
                                (default: the in-tree one), so two builds can be compared in alternating runs; where
                                the library exports gstex_loss_target_fwd / _bwd, also those on a uint8 RGBA target
                                with a bool mask.
  --mode routes                 image_loss (uint8 RGBA + bool mask) against the only route without it: eager
                                conversion, alpha composite and mask multiplies, then photometric_loss.
  --mode once                   each forward kernel a few times, for a counter-only profiling run.

Device events; warm-up, then the median over --reps timed windows of --inner forward + backward pairs each, the
measured functions taking turns window by window.  Prints
one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, warmup, reps, inner):
    """{name: percentiles of the per-call time}: each repetition times a window of `inner` calls of every function in
    turn (device events), so a drift of the machine over the run reaches all of them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
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
    mask = (torch.rand(H, W, generator=g) >= 0.3).to(dev)
    return img, tex, alpha, bg, rgba, mask


class Target(ctypes.Structure):
    _fields_ = [("gt", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("gt_dtype", ctypes.c_int32),
                ("gt_channels", ctypes.c_int32), ("mask_dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def kernel_calls(lib_path, H, W, C, dev):
    """{name: callable} of forward + backward pairs through the C ABI of `lib_path`."""
    from gstex_amd.loss import gaussian_window

    lib = ctypes.CDLL(lib_path)
    P, I, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    win = (F * 11)(*(float(x) for x in gaussian_window().numpy()))
    lib.gstex_loss_workspace_size.restype = ctypes.c_size_t
    lib.gstex_loss_workspace_size.argtypes = [I, I]
    lib.gstex_loss_fwd.argtypes = [I, I, I, P, P, P, P, P, ctypes.POINTER(F), F, P, P, P, ctypes.c_size_t, P]
    lib.gstex_loss_bwd.argtypes = [I, I, I, P, P, P, P, P, ctypes.POINTER(F), F, P, P, P, P, P, ctypes.c_size_t, P]
    img, tex, alpha, bg, rgba, mask = inputs(H, W, C, dev)
    gt = (rgba[..., :3].float() / 255).contiguous()
    out = torch.empty(4, device=dev)
    rgb, gto = torch.empty(H, W, 3, device=dev), torch.empty(H, W, 3, device=dev)
    one = torch.ones((), device=dev)
    d_img, d_tex, d_alpha = torch.empty_like(img), torch.empty_like(tex), torch.empty_like(alpha)
    st = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(int(lib.gstex_loss_workspace_size(H, W)), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"loss call failed with status {rc}")

    def base_fwd():
        check(lib.gstex_loss_fwd(H, W, C, p(img), p(tex), p(alpha), p(bg), p(gt), win, 0.2, p(rgb), p(out), p(ws),
                                 ws.numel(), st))

    def base():
        base_fwd()
        check(lib.gstex_loss_bwd(H, W, C, p(img), p(tex), p(alpha), p(bg), p(gt), win, 0.2, p(one), p(d_img), p(d_tex),
                                 p(d_alpha), p(ws), ws.numel(), st))

    calls, fwds, keep = {"loss_f32": base}, {"loss_f32": base_fwd}, [img, tex, alpha, bg, gt, ws]
    if hasattr(lib, "gstex_loss_target_fwd"):
        TP = ctypes.POINTER(Target)
        lib.gstex_loss_target_workspace_size.restype = ctypes.c_size_t
        lib.gstex_loss_target_workspace_size.argtypes = [I, I]
        lib.gstex_loss_target_fwd.argtypes = [I, I, I, P, P, P, P, TP, ctypes.POINTER(F), F, P, P, P, P,
                                              ctypes.c_size_t, P]
        lib.gstex_loss_target_bwd.argtypes = [I, I, I, P, P, P, P, TP, ctypes.POINTER(F), F, P, P, P, P, P,
                                              ctypes.c_size_t, P]
        ws3 = torch.empty(int(lib.gstex_loss_target_workspace_size(H, W)), dtype=torch.uint8, device=dev)
        keep += [ws3, rgba, mask]

        def target_pair(t):
            def fwd():
                check(lib.gstex_loss_target_fwd(H, W, C, p(img), p(tex), p(alpha), p(bg), ctypes.byref(t), win, 0.2,
                                                p(rgb), p(gto), p(out), p(ws3), ws3.numel(), st))

            def both():
                fwd()
                check(lib.gstex_loss_target_bwd(H, W, C, p(img), p(tex), p(alpha), p(bg), ctypes.byref(t), win, 0.2,
                                                p(one), p(d_img), p(d_tex), p(d_alpha), p(ws3), ws3.numel(), st))
            return fwd, both

        fwds["target_f32"], calls["target_f32"] = target_pair(Target(p(gt), None, 0, 3, 0, 0))
        fwds["target_u8_rgba_bool"], calls["target_u8_rgba_bool"] = target_pair(Target(p(rgba), p(mask), 1, 4, 1, 0))
    return calls, fwds, keep


def route_calls(H, W, C, dev):
    from gstex_amd.loss import image_loss, photometric_loss

    img, tex, alpha, bg, rgba, mask = inputs(H, W, C, dev)
    leaves = [t.requires_grad_(True) for t in (img, tex, alpha)]

    def fused():
        for t in leaves:
            t.grad = None
        image_loss(leaves[0], leaves[1], leaves[2], bg, rgba, mask).loss.backward()

    def eager_then_fused():
        # the target prepared with torch ops (gstex.py:1244-1245, 1256-1258).  The mask is not applied: it cannot be
        # prepared outside the loss without composing rgb in autograd, so this route computes less than `fused`
        for t in leaves:
            t.grad = None
        f = rgba.float() / 255.0
        a = f[..., -1].unsqueeze(-1).repeat((1, 1, 3))
        gt = a * f[..., :3] + (1 - a) * bg
        photometric_loss(leaves[0], leaves[1], leaves[2], bg, gt)[0].backward()

    def eager_masked():
        # the same loss as `fused`: eager composite of rgb and both mask multiplies, then the fused loss on a zero
        # background with alpha 1 (rgb enters as img), the gradient flowing back through the eager composite
        for t in leaves:
            t.grad = None
        f = rgba.float() / 255.0
        a = f[..., -1].unsqueeze(-1).repeat((1, 1, 3))
        gt = (a * f[..., :3] + (1 - a) * bg) * mask[..., None]
        rgb = torch.clamp(leaves[0] + leaves[1][..., :3] + (1 - leaves[2][..., None]) * bg, 0.0, 1.0) * mask[..., None]
        zeros = torch.zeros_like(leaves[1])
        photometric_loss(rgb, zeros, torch.ones_like(leaves[2]), bg, gt)[0].backward()

    return {"image_loss": fused, "eager_target_then_photometric_loss_unmasked": eager_then_fused,
            "eager_target_and_mask_then_photometric_loss": eager_masked}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "routes", "once"], default="kernels")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gstex_amd", "libgstex_hip.so"))
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_target_bench.py needs a HIP device")
    dev = torch.device("cuda", 0)
    H = W = args.size
    res = {"mode": args.mode, "tag": args.tag, "H": H, "W": W, "C": args.channels, "warmup": args.warmup,
           "reps": args.reps, "inner": args.inner}
    if args.mode == "kernels":
        res["lib"] = args.lib
        calls, _, _keep = kernel_calls(args.lib, H, W, args.channels, dev)
        res.update(timed(calls, args.warmup, args.reps, args.inner))
    elif args.mode == "routes":
        res.update(timed(route_calls(H, W, args.channels, dev), args.warmup, args.reps, args.inner))
    else:
        _, fwds, _keep = kernel_calls(args.lib, H, W, args.channels, dev)
        for fn in fwds.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
