"""Camera pose refinement: the reference presets' `camera_opt` group (configs/gstex_configs.py:48, 97-100) on this
project's views.

* exp_so3xr3 / exp_se3  <- the tangent parametrisations of cameras/camera_optimizers.py (modes "SO3xR3" and "SE3"):
                           6-vectors (translation, rotation) -> [R|t] corrections, written from the definitions
                           (Rodrigues' formula and the SE(3) left Jacobian)
* PoseRefiner.view      <- apply_to_camera (camera_optimizers.py:154-162: the OpenGL camera_to_worlds right-multiplied
                           by the correction) followed by get_outputs' y/z flip and analytic inverse
                           (gstex.py:1031-1042), expressed on the post-flip viewmat / c2w a View holds
* PoseRefiner.regulariser <- get_loss_dict (camera_optimizers.py:164-170)
* PoseRefiner.step      <- Adam(lr 1e-3, eps 1e-15) with the exponential decay to 5e-5 over 30000 steps, applied once per
                           `accumulate` (100) calls (gstex_configs.py:97-100 and :48, gradient_accumulation_steps)

The gradient reaches the adjustments through View.viewmat (ops.texture_gaussians' viewmat gradient,
gstex_raster_viewmat_bwd) and View.c2w (the SH view directions, gstex_sh_dirs_bwd); both matrices are built in torch from
the same adjustment, so they stay consistent.  Single GPU: the adjustments are not exchanged between ranks.
"""
from __future__ import annotations

import copy

import torch

from .scene import View
from .train import exponential_decay

MODES = ("SO3xR3", "SE3")
_SMALL = 1e-2  # below this angle the SE(3) coefficients are evaluated by their Taylor series


def _skew(w: torch.Tensor) -> torch.Tensor:
    """(B, 3) -> (B, 3, 3) cross-product matrices [w]x."""
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def exp_so3xr3(tangent: torch.Tensor) -> torch.Tensor:
    """(B, 6) (translation, rotation vector) -> (B, 3, 4) [exp([w]x) | t] of the direct product SO(3) x R^3.
    Rodrigues: R = I + (sin a / a) K + ((1 - cos a) / a^2) K^2 with K = [w]x.  The angle is floored at 1e-2
    (a^2 = max(|w|^2, 1e-4)), the reference's guard against 0 / 0: below it R = I + c1 K + c2 K^2 with the
    coefficients of the angle 1e-2, which differ from the exact ones by less than 2e-5 relative."""
    t, w = tangent[:, :3], tangent[:, 3:]
    a = torch.clamp((w * w).sum(1), min=1e-4).sqrt()
    K = _skew(w)
    c1 = (torch.sin(a) / a)[:, None, None]
    c2 = ((1.0 - torch.cos(a)) / (a * a))[:, None, None]
    R = c1 * K + c2 * (K @ K) + torch.eye(3, dtype=tangent.dtype, device=tangent.device)
    return torch.cat([R, t[:, :, None]], -1)


def exp_se3(tangent: torch.Tensor) -> torch.Tensor:
    """(B, 6) (v, w) in se(3) -> (B, 3, 4) [R | J v]: R = I + A K + B K^2, J = I + B K + C K^2 (the left Jacobian),
    A = sin a / a, B = (1 - cos a) / a^2, C = (a - sin a) / a^3, a = |w|; for a < 1e-2 by their Taylor series
    (1 - a^2/6, 1/2 - a^2/24, 1/6 - a^2/120: the next terms are below 1e-9, under fp32 rounding)."""
    v, w = tangent[:, :3], tangent[:, 3:]
    a2 = (w * w).sum(1)
    small = a2 < _SMALL * _SMALL
    # (1 in the small branch, which does not use it: a safe divisor, and no sqrt'(0) in the backward)
    an = torch.where(small, torch.ones_like(a2), a2).sqrt()
    A = torch.where(small, 1.0 - a2 / 6.0, torch.sin(an) / an)
    B = torch.where(small, 0.5 - a2 / 24.0, (1.0 - torch.cos(an)) / (an * an))
    C = torch.where(small, 1.0 / 6.0 - a2 / 120.0, (an - torch.sin(an)) / (an * an * an))
    K = _skew(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)
    R = eye + A[:, None, None] * K + B[:, None, None] * K2
    J = eye + B[:, None, None] * K + C[:, None, None] * K2
    return torch.cat([R, J @ v[:, :, None]], -1)


def corrected_matrices(viewmat: torch.Tensor, c2w: torch.Tensor, corr: torch.Tensor):
    """A View's (viewmat (3,4), c2w (4,4)) with the reference's correction `corr` = [Ra | ta] (3,4) applied.

    The reference multiplies the OpenGL camera_to_worlds C = [R_gl | T] by the correction on the right, C' = C [Ra|ta],
    and get_outputs then flips y and z (R = R_gl F, F = diag(1, -1, -1)) and inverts.  A View holds the post-flip
    matrices c2w = [R | T] (R = R_gl F) and viewmat = [R^T | -R^T T] = [Rv | tv], on which that reads
        c2w'     = [R (F Ra F) | T + R F ta]
        viewmat' = [(F Ra F)^T Rv | (F Ra F)^T (tv - F ta)].
    """
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=corr.dtype, device=corr.device)
    Ra = flip[:, None] * corr[:, :3] * flip[None, :]  # F Ra F
    ta = flip * corr[:, 3]  # F ta
    R, T = c2w[:3, :3], c2w[:3, 3]
    Rv, tv = viewmat[:3, :3], viewmat[:3, 3]
    top = torch.cat([R @ Ra, (T + R @ ta)[:, None]], 1)
    c2w_new = torch.cat([top, c2w[3:4, :].to(top.dtype)], 0)
    vm_new = torch.cat([Ra.T @ Rv, (Ra.T @ (tv - ta))[:, None]], 1)
    return vm_new, c2w_new


class PoseRefiner:
    """Per-view SO3xR3 / SE3 pose corrections, their regulariser and their optimizer (see the module docstring).

        refiner = PoseRefiner(len(pairs), trainer.device)
        out = trainer.forward_backward(refiner.view(i, view), image, extra_loss=refiner.regulariser())
        trainer.optimizer_step(); refiner.step()
    or  train.fit(trainer, pairs, steps, pose_refiner=refiner).
    """

    def __init__(self, n_views: int, device, mode: str = "SO3xR3", lr: float = 1e-3, lr_final: float = 5e-5,
                 max_steps: int = 30000, eps: float = 1e-15, accumulate: int = 100, trans_l2_penalty: float = 1e-2,
                 rot_l2_penalty: float = 1e-3):
        if mode not in MODES:
            raise ValueError(f"PoseRefiner: mode must be one of {MODES} (got {mode!r})")
        if int(n_views) < 1 or int(accumulate) < 1:
            raise ValueError("PoseRefiner: n_views and accumulate must be >= 1")
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            raise RuntimeError("PoseRefiner: pose refinement is single-GPU (the adjustments are not exchanged between "
                               "ranks); world size is %d" % torch.distributed.get_world_size())
        self.mode = mode
        self.device = torch.device(device)
        self.pose_adjustment = torch.nn.Parameter(torch.zeros((int(n_views), 6), device=self.device))
        self.lr, self.lr_final, self.max_steps = float(lr), float(lr_final), int(max_steps)
        self.accumulate = int(accumulate)
        self.trans_l2_penalty, self.rot_l2_penalty = float(trans_l2_penalty), float(rot_l2_penalty)
        self.optimizer = torch.optim.Adam([self.pose_adjustment], lr=self.lr, eps=float(eps))
        self._schedule = exponential_decay(self.lr, self.lr_final, self.max_steps)
        self.steps = 0  # step() calls so far: the training step the schedule and the accumulation count

    # ------------------------------------------------------------------ the corrected camera
    def correction(self, index: int) -> torch.Tensor:
        """The (3, 4) correction [Ra | ta] of view `index` (identity at a zero adjustment)."""
        t = self.pose_adjustment[int(index)][None]
        return (exp_so3xr3(t) if self.mode == "SO3xR3" else exp_se3(t))[0]

    def view(self, index: int, base_view: View) -> View:
        """The camera the reference would render for view `index`: base_view with its correction applied, viewmat and
        c2w both differentiable functions of pose_adjustment[index]."""
        vm, c2w = corrected_matrices(base_view.viewmat.detach(), base_view.c2w.detach(), self.correction(index))
        return View(vm, c2w, base_view.fx, base_view.fy, base_view.cx, base_view.cy, base_view.H, base_view.W)

    def regulariser(self) -> torch.Tensor:
        """mean |translation part| * trans_l2_penalty + mean |rotation part| * rot_l2_penalty over the views."""
        p = self.pose_adjustment
        return (p[:, :3].norm(dim=-1).mean() * self.trans_l2_penalty
                + p[:, 3:].norm(dim=-1).mean() * self.rot_l2_penalty)

    # ------------------------------------------------------------------ the optimizer
    def current_lr(self) -> float:
        """The learning rate at the current step: exponential_decay(lr, lr_final, max_steps)(steps so far) -- the
        reference's scheduler advances every training step, whatever the accumulation."""
        return self._schedule(self.steps)

    def step(self) -> bool:
        """Count one training step s; when s % accumulate == accumulate - 1, apply Adam at the step's learning rate to
        the gradients summed since the last update and clear them (engine/trainer.py:451-465: zeroed where
        s % accumulate == 0, stepped where s % accumulate == accumulate - 1).  -> whether the parameters moved."""
        due = self.steps % self.accumulate == self.accumulate - 1
        moved = False
        if due:
            if self.pose_adjustment.grad is not None:
                self.optimizer.param_groups[0]["lr"] = self.current_lr()
                self.optimizer.step()
                moved = True
            self.optimizer.zero_grad(set_to_none=True)
        self.steps += 1
        return moved

    def state_dict(self) -> dict:
        return dict(mode=self.mode, pose_adjustment=self.pose_adjustment.detach().clone(),
                    grad=None if self.pose_adjustment.grad is None else self.pose_adjustment.grad.detach().clone(),
                    optimizer=copy.deepcopy(self.optimizer.state_dict()), steps=self.steps)

    def load_state_dict(self, state: dict) -> None:
        if state["mode"] != self.mode:
            raise ValueError(f"PoseRefiner: state is for mode {state['mode']!r}, this refiner is {self.mode!r}")
        p = state["pose_adjustment"]
        if tuple(p.shape) != tuple(self.pose_adjustment.shape):
            raise ValueError(f"PoseRefiner: state has {tuple(p.shape)} adjustments, this refiner "
                             f"{tuple(self.pose_adjustment.shape)}")
        with torch.no_grad():
            self.pose_adjustment.copy_(p.to(self.device))
        g = state.get("grad")
        self.pose_adjustment.grad = None if g is None else g.detach().clone().to(self.device)
        self.optimizer.load_state_dict(copy.deepcopy(state["optimizer"]))  # (the moments are not shared)
        self.steps = int(state["steps"])
