"""Camera pose refinement without a GPU: the two new C-ABI entry points' bindings and argument checks, and
gstex_amd.pose.PoseRefiner (exponential maps and view() against the reference's own code through
tests/golden/pose_golden.npz, the regulariser, the accumulation and the learning-rate schedule)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gstex_amd import _lib
from gstex_amd.pose import PoseRefiner, corrected_matrices, exp_se3, exp_so3xr3
from gstex_amd.scene import View

HERE = os.path.dirname(os.path.abspath(__file__))
EPS32 = 2.0 ** -24  # the unit roundoff of fp32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pose_golden.npz"))


# ---------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_bound(lib):
    for name in ("gstex_raster_viewmat_bwd", "gstex_raster_viewmat_bwd_workspace", "gstex_sh_dirs_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19  # added within ABI 19
    # ceil(n / 256) * 12 doubles
    for n, rows in ((0, 0), (1, 1), (256, 1), (257, 2), (70001, 274)):
        assert lib.gstex_raster_viewmat_bwd_workspace(n) == rows * 12 * 8
    assert lib.gstex_raster_viewmat_bwd_workspace(-3) == 0


def _vm_args(**kw):
    one = ctypes.c_void_p(16)  # a non-NULL placeholder: every rejected call returns before any pointer is read
    base = dict(n=4, glob_scale=1.0, row_floats=32, fold_aabb=0, n_rows=-1,
                cam=_lib.GstexCamera(one, None, 100.0, 100.0, 16.0, 16.0, 32, 32, 16), means=one, scales=one,
                quats=one, num_tiles_hit=one, offsets=one, partials=one, row_flags=None, v_centers=None,
                workspace=one, v_viewmat=one)
    base.update(kw)
    return _lib.GstexRasterViewmatBwdArgs(**base)


def test_viewmat_bwd_rejects_invalid_arguments(lib):
    def status(args):
        rc = lib.gstex_raster_viewmat_bwd(None if args is None else ctypes.byref(args), None)
        return rc, _lib.last_error()

    rc, msg = status(None)
    assert rc == 1 and "gstex_raster_viewmat_bwd" in msg and "invalid arguments" in msg
    rc, msg = status(_vm_args(n=-1))
    assert rc == 1 and "invalid arguments" in msg
    for field in ("v_viewmat", "means", "scales", "quats", "workspace", "num_tiles_hit", "offsets"):
        rc, msg = status(_vm_args(**{field: None}))
        assert rc == 1 and "null pointer" in msg, (field, rc, msg)
    rc, msg = status(_vm_args(row_floats=16))
    assert rc == 1 and "row_floats must be 24 or 32" in msg
    rc, msg = status(_vm_args(partials=None, v_centers=None))  # neither mode's input
    assert rc == 1 and "neither partials nor v_centers" in msg
    rc, msg = status(_vm_args(v_centers=ctypes.c_void_p(16)))  # both modes' inputs
    assert rc == 1 and "v_centers" in msg


def test_sh_dirs_bwd_rejects_invalid_arguments(lib):
    one = ctypes.c_void_p(16)

    def status(*a):
        rc = lib.gstex_sh_dirs_bwd(*a)
        return rc, _lib.last_error()

    rc, msg = status(-1, 3, 0, 16, one, one, one, one, None)
    assert rc == 1 and "gstex_sh_dirs_bwd" in msg
    rc, msg = status(4, 5, 0, 36, one, one, one, one, None)
    assert rc == 1 and "degree" in msg
    rc, msg = status(4, 3, 2, 16, one, one, one, one, None)
    assert rc == 1 and "k0 must be 0" in msg
    rc, msg = status(4, 3, 0, 15, one, one, one, one, None)  # the full layout needs 16 at degree 3 ...
    assert rc == 1 and "coefficients" in msg
    rc, msg = status(4, 3, 1, 14, one, one, one, one, None)  # ... the rest layout 15
    assert rc == 1 and "coefficients" in msg
    for k in range(4):
        a = [one, one, one, one]
        a[k] = None
        rc, msg = status(4, 3, 0, 16, *a, None)
        assert rc == 1 and "null pointer" in msg, k
    assert lib.gstex_sh_dirs_bwd(0, 3, 0, 16, None, None, None, None, None) == 0  # nothing to do


# ---------------------------------------------------------------------------------------------- the maps and view()
def test_exponential_maps_match_the_reference(golden):
    """Bound: both sides evaluate, in fp32, sums of at most three products of quantities <= s = max(1, |entry|) with
    coefficients (sin a / a, (1 - cos a) / a^2, ...) that each carry a few roundings; (1 - cos a) / a^2 at the floor
    angle 1e-2 amplifies cos's half-ulp by 1 / a^2 = 1e4 relative to 1 - cos a = 5e-5, i.e. an absolute 6e-8 * 1e4 *
    |K^2| <= 6e-4 |w|^2.  So: 32 roundings of s, plus 1e4 * eps32 * |w|^2 where the floor applies."""
    tan = torch.from_numpy(golden["tangents"])
    w2 = (tan[:, 3:] ** 2).sum(1)
    for mode, fn in (("SO3xR3", exp_so3xr3), ("SE3", exp_se3)):
        ref = torch.from_numpy(golden[f"exp_{mode}"])
        got = fn(tan)
        assert got.dtype == torch.float32 and got.shape == ref.shape == (12, 3, 4)
        scale = ref.abs().clamp(min=1.0)
        bound = 32 * EPS32 * scale + (1e4 * EPS32 * torch.where(w2 < 1e-4, w2, torch.zeros_like(w2)))[:, None, None]
        err = (got - ref).abs()
        print(mode, "max err", float(err.max()), "min slack", float((bound - err).min()))
        assert bool((err <= bound).all()), (mode, float((err - bound).max()))
    # both are rigid: R^T R = I to fp32 rounding, also through the small-angle branches
    for fn in (exp_so3xr3, exp_se3):
        R = fn(tan.double())[:, :, :3]
        big = w2 >= 1e-4  # (the SO3xR3 floor makes R slightly non-orthonormal below it, as the reference's is)
        assert float((R[big].transpose(1, 2) @ R[big] - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_view_matches_the_reference_camera(golden, mode):
    """viewmat: two 3x3 products of entries <= |T| ~ 4.1 on each side -> 64 roundings of max(1, |entry|).  c2w: the
    reference inverts its fp32 viewmat numerically, whose forward error is bounded by ~ n eps cond(viewmat) |c2w|
    (n = 4, a factor 2 for the two sides): computed from the golden's own viewmat."""
    base = View(torch.from_numpy(golden["base_viewmat"]), torch.from_numpy(golden["base_c2w"]), 100.0, 100.0, 40.0,
                32.0, 64, 80)
    tan = torch.from_numpy(golden["tangents"])
    ref_vm, ref_c2w = golden[f"viewmat_{mode}"], golden[f"c2w_{mode}"]
    r = PoseRefiner(tan.shape[0], "cpu", mode=mode)
    with torch.no_grad():
        r.pose_adjustment.copy_(tan)
    for i in range(tan.shape[0]):
        v = r.view(i, base)
        assert (v.fx, v.fy, v.cx, v.cy, v.H, v.W) == (100.0, 100.0, 40.0, 32.0, 64, 80)
        assert tuple(v.viewmat.shape) == (3, 4) and tuple(v.c2w.shape) == (4, 4)
        assert v.viewmat.requires_grad and v.c2w.requires_grad
        vm_b = 64 * EPS32 * np.maximum(np.abs(ref_vm[i][:3]), 1.0)
        cond = np.linalg.cond(ref_vm[i].astype(np.float64))
        c2w_b = 8 * EPS32 * cond * np.abs(ref_c2w[i]).max() + 64 * EPS32
        e_vm = np.abs(v.viewmat.detach().numpy() - ref_vm[i][:3])
        e_cw = np.abs(v.c2w.detach().numpy() - ref_c2w[i])
        assert (e_vm <= vm_b).all(), (i, e_vm.max())
        assert (e_cw <= c2w_b).all(), (i, e_cw.max(), c2w_b)
        # consistent: viewmat @ c2w = I (what a viewmat / c2w mismatch in the trainer would break)
        vm4 = torch.cat([v.viewmat.detach().double(), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0)
        assert float((vm4 @ v.c2w.detach().double() - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-5


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_zero_adjustment_is_the_base_view(golden, mode):
    base = View(torch.from_numpy(golden["base_viewmat"]), torch.from_numpy(golden["base_c2w"]), 100.0, 90.0, 40.0,
                32.0, 64, 80)
    r = PoseRefiner(3, "cpu", mode=mode)
    v = r.view(1, base)
    assert torch.equal(v.viewmat.detach(), base.viewmat) and torch.equal(v.c2w.detach(), base.c2w)
    # and it is differentiable there: finite gradients to the six parameters from both matrices
    (v.viewmat.sum() + v.c2w.sum()).backward()
    g = r.pose_adjustment.grad
    assert bool(torch.isfinite(g).all()) and float(g[1].abs().min()) > 0 and float(g[0].abs().max()) == 0.0


def test_view_gradient_matches_finite_differences():
    torch.manual_seed(0)
    from gstex_amd.scene import sphere_view

    base = sphere_view(2, 64, 80)
    base = View(base.viewmat.double(), base.c2w.double(), base.fx, base.fy, base.cx, base.cy, 64, 80)
    wv, wc = torch.randn(3, 4, dtype=torch.float64), torch.randn(4, 4, dtype=torch.float64)
    for fn in (exp_so3xr3, exp_se3):
        t = (0.1 * torch.randn(1, 6, dtype=torch.float64)).requires_grad_(True)

        def f(t):
            vm, c2w = corrected_matrices(base.viewmat, base.c2w, fn(t)[0])
            return (vm * wv).sum() + (c2w * wc).sum()

        assert torch.autograd.gradcheck(f, (t,), eps=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------- regulariser, optimizer
def test_regulariser_value():
    r = PoseRefiner(3, "cpu", trans_l2_penalty=1e-2, rot_l2_penalty=1e-3)
    assert float(r.regulariser().detach()) == 0.0
    with torch.no_grad():
        r.pose_adjustment.copy_(torch.tensor([[3.0, 4.0, 0.0, 0.0, 0.0, 2.0], [0.0, 0.0, 0.0, 1.0, 2.0, 2.0],
                                              [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]))
    # translations' norms (5, 0, 0) -> mean 5/3; rotations' norms (2, 3, 0) -> mean 5/3
    want = (5.0 / 3.0) * 1e-2 + (5.0 / 3.0) * 1e-3
    assert abs(float(r.regulariser().detach()) - want) <= 4 * EPS32 * want
    r.regulariser().backward()  # the zero row's norm has a zero (not NaN) gradient
    assert bool(torch.isfinite(r.pose_adjustment.grad).all())


def test_accumulation_99_calls_leave_the_parameters_the_100th_moves_them():
    r = PoseRefiner(2, "cpu")  # accumulate = 100
    assert r.accumulate == 100
    g = torch.tensor([[1.0, -2.0, 0.5, 0.125, 0.0, -0.25], [0.0] * 6])  # (dyadic: the sums below are exact)
    for k in range(99):
        r.pose_adjustment.grad = g.clone() if r.pose_adjustment.grad is None else r.pose_adjustment.grad + g
        assert r.step() is False
        assert float(r.pose_adjustment.detach().abs().max()) == 0.0, k
    assert torch.equal(r.pose_adjustment.grad, 99 * g)  # summed, not cleared
    r.pose_adjustment.grad += g
    assert r.step() is True
    p = r.pose_adjustment.detach()
    # Adam's first update: -lr * sign(g) where g != 0 (eps 1e-15), at the learning rate of step 99
    lr = r._schedule(99)
    assert torch.allclose(p[0], -lr * torch.sign(g[0]), rtol=1e-5, atol=0) and float(p[1].abs().max()) == 0.0
    assert r.pose_adjustment.grad is None and r.steps == 100
    # a cycle without any gradient moves nothing
    for _ in range(100):
        assert r.step() is False
    assert torch.equal(r.pose_adjustment.detach(), p)


def test_learning_rate_schedule_endpoints():
    r = PoseRefiner(1, "cpu", accumulate=1)
    assert r.current_lr() == pytest.approx(1e-3, rel=1e-12)
    r.steps = 30000
    assert r.current_lr() == pytest.approx(5e-5, rel=1e-12)
    r.steps = 10 ** 6
    assert r.current_lr() == pytest.approx(5e-5, rel=1e-12)  # held at the final value
    r.steps = 15000
    assert r.current_lr() == pytest.approx(math.sqrt(1e-3 * 5e-5), rel=1e-12)  # log-linear
    # the optimizer runs at the schedule's value
    r.steps = 30000
    r.pose_adjustment.grad = torch.ones(1, 6)
    assert r.step() is True
    assert r.optimizer.param_groups[0]["lr"] == pytest.approx(5e-5, rel=1e-12)
    assert torch.allclose(r.pose_adjustment.detach(), torch.full((1, 6), -5e-5), rtol=1e-5, atol=0)


def test_state_dict_round_trip():
    a = PoseRefiner(2, "cpu", accumulate=2)
    for k in range(3):
        a.pose_adjustment.grad = torch.full((2, 6), 0.1 * (k + 1))
        a.step()
    a.pose_adjustment.grad = torch.full((2, 6), 0.7)  # a pending, not yet applied gradient
    b = PoseRefiner(2, "cpu", accumulate=2)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.pose_adjustment.detach(), b.pose_adjustment.detach()) and b.steps == a.steps == 3
    assert a.step() is True and b.step() is True
    assert torch.equal(a.pose_adjustment.detach(), b.pose_adjustment.detach())
    with pytest.raises(ValueError):
        PoseRefiner(2, "cpu", mode="SE3").load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        PoseRefiner(3, "cpu").load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        PoseRefiner(2, "cpu", mode="so3")


def test_refiner_refuses_a_multi_rank_process_group(monkeypatch):
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="single-GPU"):
        PoseRefiner(4, "cpu")
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    PoseRefiner(4, "cpu")  # a one-rank group is fine
