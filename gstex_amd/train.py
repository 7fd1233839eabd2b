"""The reference presets' training loop around GStexTrainer: learning-rate schedule, view order, rechart cadence.

* exponential_decay  <- engine/schedulers.py:122-138 (warmup_steps = 0), the means' schedule of every preset
* PRESETS            <- configs/gstex_configs.py (the six gstex-* entries)
* fit                <- the train iteration with the model's callbacks (gstex.py:901-914: retexture_after after
                        every iteration whose step is a multiple of build_chart_every, step 0 included)

Single GPU.  The loop reads nothing back from the device: the losses go into one preallocated device tensor.
"""
from __future__ import annotations

import math

import torch

# configs/gstex_configs.py.  lrs: the optimizers' lr per group; xyz_lr_final / xyz_max_steps: the means'
# ExponentialDecaySchedulerConfig (the only scheduled group besides camera_opt: gstex_amd.pose.PoseRefiner); max_steps:
# max_num_iterations.  Every preset has sh_degree 3, build_chart_every 100 and sigma_factor 3.
_COMMON_LRS = {"features_dc": 0.0025, "features_rest": 0.0025 / 20, "opacity": 0.05, "scaling": 0.005,
               "rotation": 0.001, "texture_dc": 1e-3}


def _preset(pixel_num, background, fix_init, fix_lod_init, max_steps, xyz_lr, xyz_lr_final, xyz_max_steps):
    return dict(pixel_num=pixel_num, background=background, fix_init=fix_init, fix_lod_init=fix_lod_init,
                max_steps=max_steps, lrs={"xyz": xyz_lr, **_COMMON_LRS}, xyz_lr_final=xyz_lr_final,
                xyz_max_steps=xyz_max_steps, build_chart_every=100, sh_degree=3)


PRESETS = {
    # gstex_configs.py:39-105 (model :55-62, xyz :65-72, the other groups :73-96)
    "blender-init": _preset(1e6, "white", False, False, 1, 5 * 1.6e-5, 5 * 1.6e-6, 15000),
    # gstex_configs.py:107-180 (model :130-137, xyz :140-147, the other groups :148-171)
    "colmap-init": _preset(1e7, "black", True, False, 1, 2 * 1.6e-5, 2 * 1.6e-6, 15000),
    # gstex_configs.py:182-249 (model :198-205, xyz :208-215, the other groups :216-239)
    "blender-nvs": _preset(1e6, "white", False, False, 15000, 5 * 1.6e-5, 5 * 1.6e-6, 15000),
    # gstex_configs.py:251-325 (model :274-281, xyz :284-291, the other groups :292-315)
    "dtu-nvs": _preset(1e6, "black", True, False, 15000, 2 * 1.6e-5, 2 * 1.6e-6, 15000),
    # gstex_configs.py:327-394 (model :343-350, xyz :353-360, the other groups :361-384)
    "blender-lod": _preset(1e6, "white", False, False, 7000, 5 * 1.6e-4, 5 * 1.6e-6, 30000),
    # gstex_configs.py:396-471 (model :419-427, xyz :430-437, the other groups :438-461)
    "dtu-lod": _preset(1e6, "black", True, True, 7000, 2 * 1.6e-4, 2 * 1.6e-6, 30000),
}


def exponential_decay(lr_init: float, lr_final: float, max_steps: int):
    """f(step) = exp(log(lr_init) (1 - t) + log(lr_final) t), t = clip(step / max_steps, 0, 1): the learning rate
    used AT step `step` (LambdaLR steps after the optimizer, so step 0 runs at lr_init)."""
    a, b = math.log(lr_init), math.log(lr_final)

    def f(step):
        t = min(max(step / max_steps, 0.0), 1.0)
        return math.exp(a * (1.0 - t) + b * t)

    return f


def _to_device(pair, device):
    view, image = pair[0].to(device), pair[1].to(device)
    mask = pair[2].to(device) if len(pair) > 2 and pair[2] is not None else None
    return view, image, mask


def fit(trainer, pairs, steps: int, *, xyz_lr_final: float | None = None, max_steps: int = 15000,
        build_chart_every: int = 100, seed: int = 0, on_step=None, pose_refiner=None, density=None) -> dict:
    """Run `steps` training steps from trainer.step on.  pairs: a sequence of (View, image[, mask]) as
    gstex_amd.data.load_blender yields them, moved to the trainer's device once.  Per step s = trainer.step:

    1. the xyz group's lr is exponential_decay(trainer.lrs["xyz"], xyz_lr_final, max_steps)(s) (None: left alone);
    2. the next view of a permutation drawn from a CPU torch.Generator(seed), reshuffled when exhausted (each view
       once per epoch; the reference draws from Python's global `random`, whose sequence is not reproduced);
    3. zero_grad(), forward_backward(), optimizer_step();
    4. recharge() when s % build_chart_every == 0 (gstex.py:907-914; 0 or None: never);
    5. on_step(s, out) with forward_backward's StepOutput.

    pose_refiner (a gstex_amd.pose.PoseRefiner over these pairs; the presets' camera_opt group): step 3 renders
    pose_refiner.view(k, view) for the chosen pair k, adds pose_refiner.regulariser() to the loss and calls
    pose_refiner.step() after optimizer_step().  None: the loop above, unchanged.

    density (a gstex_amd.density.DensityController over a one-texel trainer; the geometry stage): step 3 becomes
    zero_grad(), forward_backward(), density.accumulate(trainer, view), optimizer_step(), density.update(trainer) --
    the statistics read the step's gradient before Adam consumes it, an event (clone / split / prune, opacity reset)
    runs after the update.  build_chart_every must then be 0 or None (ValueError): density control is defined on
    one-texel charts.  The returned dict gains density, the list of the events' records.  None: the loop above,
    unchanged.

    Returns loss (a (steps,) device tensor, filled without a read-back), views (the chosen indices) and recharts
    (the steps s after which a rechart ran).  The only host synchronisation is inside a rechart (build_charts'
    bisection reads its score back)."""
    if density is not None and build_chart_every:
        raise ValueError(f"fit: density control needs build_chart_every = 0 or None (got {build_chart_every}): it is "
                         "defined on one-texel charts, which a rechart replaces")
    pairs = [_to_device(p, trainer.device) for p in pairs]
    if not pairs:
        raise ValueError("fit: no (view, image) pairs")
    group = next(g for g in trainer.optimizer.param_groups if g["name"] == "xyz")
    schedule = None if xyz_lr_final is None else exponential_decay(trainer.lrs["xyz"], xyz_lr_final, max_steps)
    gen = torch.Generator().manual_seed(int(seed))
    losses = torch.zeros(int(steps), device=trainer.device, dtype=torch.float32)
    order, views, recharts, events = [], [], [], []
    for i in range(int(steps)):
        s = trainer.step
        if schedule is not None:
            group["lr"] = schedule(s)
        if not order:
            order = torch.randperm(len(pairs), generator=gen).tolist()[::-1]
        k = order.pop()
        view, image, mask = pairs[k]
        trainer.zero_grad()
        if pose_refiner is None:
            out = trainer.forward_backward(view, image, mask)
        else:
            view = pose_refiner.view(k, view)
            out = trainer.forward_backward(view, image, mask, extra_loss=pose_refiner.regulariser())
        if density is not None:
            density.accumulate(trainer, view)
        trainer.optimizer_step()
        if pose_refiner is not None:
            pose_refiner.step()
        if density is not None:
            event = density.update(trainer)
            if event is not None:
                events.append(event)
        losses[i].copy_(out.loss)
        views.append(k)
        if build_chart_every and s % build_chart_every == 0:
            trainer.recharge()
            recharts.append(s)
        if on_step is not None:
            on_step(s, out)
    res = dict(loss=losses, views=views, recharts=recharts)
    if density is not None:
        res["density"] = events
    return res
