"""gstex_amd.density without a GPU: the C-ABI of the three density-control entry points, the eager twins' decisions and
layout on a hand-written table, fit()'s call order with a controller, the 2DGS checkpoint round trip and
GStexTrainer.apply_density on a CPU trainer (through the twins)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gstex_amd import _lib
from gstex_amd import density as dn

KEEP, CLONE, SPLIT, PRUNE = dn.KEEP, dn.CLONE, dn.SPLIT, dn.PRUNE
NEW = ("gstex_density_accum", "gstex_density_plan", "gstex_density_apply")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _status(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, _lib.last_error()


# ---------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "gstex_hip.h")).read()
    for s in NEW:
        assert f"int {s}(" in header and hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert "#define GSTEX_ABI_VERSION 19" in header
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19
    assert (_lib.DENSITY_KEEP, _lib.DENSITY_CLONE, _lib.DENSITY_SPLIT, _lib.DENSITY_PRUNE) == (0, 1, 2, 3)


def test_struct_layouts_match_header(tmp_path):
    import subprocess

    structs = {"gstex_density_plan_args": _lib.GstexDensityPlanArgs, "gstex_density_tensor": _lib.GstexDensityTensor,
               "gstex_density_apply_args": _lib.GstexDensityApplyArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append('printf("max %d\\n", GSTEX_DENSITY_MAX_TENSORS);')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    assert int(got["max"]) == _lib.DENSITY_MAX_TENSORS
    for cname, cls in structs.items():
        assert int(got[f"{cname} size"]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got[f"{cname} {f[0]}"]) == getattr(cls, f[0]).offset, f"{cname}.{f[0]}"


def _cam(fx=100.0, fy=100.0, H=32, W=32, viewmat=None):
    return _lib.GstexCamera(viewmat, None, fx, fy, 16.0, 16.0, H, W, 16)


def _buf():
    """A host word array's address: compared, null- and alignment-checked only (rejected before any launch)."""
    keep = (ctypes.c_float * 64)()
    return keep, ctypes.addressof(keep)


def test_accum_rejects_bad_arguments(lib):
    keep, b = _buf()
    cam = _cam(viewmat=b)
    ok = [b] * 2 + [ctypes.byref(cam)] + [b, b, None, b, b, b, None]
    rc, msg = _status(lib, "gstex_density_accum", -1, *ok)
    assert rc == 1 and "n < 0" in msg
    rc, msg = _status(lib, "gstex_density_accum", 4, b, b, None, b, b, None, b, b, b, None)
    assert rc == 1 and "null camera" in msg
    for bad in (dict(fx=float("nan")), dict(fy=float("inf")), dict(fx=0.0), dict(fy=-1.0)):
        c = _cam(viewmat=b, **bad)
        rc, msg = _status(lib, "gstex_density_accum", 4, b, b, ctypes.byref(c), b, b, None, b, b, b, None)
        assert rc == 1 and "fx, fy must be finite" in msg, bad
    c = _cam(viewmat=b, H=0)
    rc, msg = _status(lib, "gstex_density_accum", 4, b, b, ctypes.byref(c), b, b, None, b, b, b, None)
    assert rc == 1 and "image size" in msg
    for hole in (0, 1, 3, 4, 6, 7, 8):  # each required pointer in turn
        args = list(ok)
        args[hole] = None
        rc, msg = _status(lib, "gstex_density_accum", 4, *args)
        assert rc == 1 and "null pointer" in msg, hole
    c = _cam(viewmat=None)
    rc, msg = _status(lib, "gstex_density_accum", 4, b, b, ctypes.byref(c), b, b, None, b, b, b, None)
    assert rc == 1 and "null pointer" in msg
    for hole in (0, 1, 3, 4, 5, 6, 7, 8):
        args = list(ok)
        args[hole] = b + 2
        rc, msg = _status(lib, "gstex_density_accum", 4, *args)
        assert rc == 1 and "misaligned" in msg, hole
    # n = 0: a successful no-op, before any pointer is looked at
    assert lib.gstex_density_accum(0, None, None, ctypes.byref(_cam()), None, None, None, None, None, None, None) == 0
    del keep


def _plan_args(b, **kw):
    a = dict(n=4, size_prune=0, prune_only=0, grad_threshold=2e-4, log_big=-2.0, logit_faint=-5.0,
             max_screen_px=20.0, log_world=0.0, log_split=0.47, log_scales=b, opac_logits=b, grad_sum=b, count=b,
             max_extent=b, rows=b, kind=b)
    a.update(kw)
    return _lib.GstexDensityPlanArgs(**a)


def test_plan_rejects_bad_arguments(lib):
    keep, b = _buf()
    rc, msg = _status(lib, "gstex_density_plan", None, None)
    assert rc == 1 and "null args" in msg
    rc, msg = _status(lib, "gstex_density_plan", ctypes.byref(_plan_args(b, n=-3)), None)
    assert rc == 1 and "n < 0" in msg
    for name in ("grad_threshold", "log_big", "logit_faint", "max_screen_px", "log_world", "log_split"):
        for v in (float("nan"), float("inf"), -float("inf")):
            rc, msg = _status(lib, "gstex_density_plan", ctypes.byref(_plan_args(b, **{name: v})), None)
            assert rc == 1 and "non-finite threshold" in msg, (name, v)
    rc, msg = _status(lib, "gstex_density_plan", ctypes.byref(_plan_args(b, grad_threshold=-1.0)), None)
    assert rc == 1 and "grad_threshold < 0" in msg
    for name in ("log_scales", "opac_logits", "grad_sum", "count", "max_extent", "rows", "kind"):
        rc, msg = _status(lib, "gstex_density_plan", ctypes.byref(_plan_args(b, **{name: None})), None)
        assert rc == 1 and "null pointer" in msg, name
        rc, msg = _status(lib, "gstex_density_plan", ctypes.byref(_plan_args(b, **{name: b + 1})), None)
        assert rc == 1 and "misaligned" in msg, name
    empty = _plan_args(None, n=0)
    assert lib.gstex_density_plan(ctypes.byref(empty), None) == 0
    del keep


def _apply_args(b, tensors, **kw):
    arr = (_lib.GstexDensityTensor * max(len(tensors), 1))(*tensors)
    a = dict(n=4, n_tensors=len(tensors), n_new=6, log_split=0.47, rows=b, kind=b, offsets=b, scales=b, quats_n=b,
             noise=b, tensors=arr)
    a.update(kw)
    return _lib.GstexDensityApplyArgs(**a), arr


def test_apply_rejects_bad_arguments(lib):
    keep, b = _buf()
    keep2, b2 = _buf()
    T = _lib.GstexDensityTensor
    good = [T(b, b2, 3, _lib.DENSITY_ROLE_COPY)]

    def status(tensors=good, **kw):
        a, arr = _apply_args(b, tensors, **kw)
        return _status(lib, "gstex_density_apply", ctypes.byref(a), None)

    rc, msg = _status(lib, "gstex_density_apply", None, None)
    assert rc == 1 and "null args" in msg
    for kw in (dict(n=-1), dict(n_new=-1), dict(n_new=9), dict(n=1 << 30, n_new=1 << 31)):
        rc, msg = status(**kw)
        assert rc == 1 and "invalid sizes" in msg, kw
    rc, msg = status(n_tensors=_lib.DENSITY_MAX_TENSORS + 1)
    assert rc == 1 and "n_tensors" in msg
    rc, msg = status(log_split=float("nan"))
    assert rc == 1 and "non-finite log_split" in msg
    a, arr = _apply_args(b, good)
    a.tensors = ctypes.POINTER(T)()
    rc, msg = _status(lib, "gstex_density_apply", ctypes.byref(a), None)
    assert rc == 1 and "null tensor table" in msg
    for name in ("rows", "kind", "offsets"):
        rc, msg = status(**{name: None})
        assert rc == 1 and "null pointer" in msg, name
    for name in ("rows", "kind", "offsets", "scales", "quats_n", "noise"):
        rc, msg = status(**{name: b + 2})
        assert rc == 1 and "misaligned" in msg, name
    for bad, what in ((T(b, b2, -1, 0), "width < 0"), (T(b, b2, 3, 7), "unknown role"), (T(None, b2, 3, 0), "null"),
                      (T(b, None, 3, 0), "null"), (T(b + 1, b2, 3, 0), "misaligned"), (T(b, b2 + 2, 3, 0), "misaligned"),
                      (T(b, b, 3, 0), "must differ"), (T(b, b2, 4, _lib.DENSITY_ROLE_MEANS), "width 3"),
                      (T(b, b2, 1, _lib.DENSITY_ROLE_LOG_SCALES), "width >= 2")):
        rc, msg = status(tensors=[bad])
        assert rc == 1 and what in msg, what
    rc, msg = status(tensors=[T(b, b2, 3, _lib.DENSITY_ROLE_MEANS)], noise=None)
    assert rc == 1 and "scales, quats_n and noise" in msg
    # nothing to do: n = 0, n_new = 0, no tensors, only zero-width tensors -- all before any launch
    assert status(n=0, n_new=0, rows=None, kind=None, offsets=None)[0] == 0
    assert status(n_new=0)[0] == 0
    assert status(tensors=[])[0] == 0
    assert status(tensors=[T(None, None, 0, 0)])[0] == 0
    del keep, keep2


# ---------------------------------------------------------------------------------------- the twins
EXTENT = 10.0  # log_big = log(0.1), log_world = log(1) = 0
TH = dn.density_thresholds(EXTENT)

# one splat per decision branch: (max log-scale m, opacity logit, grad_sum, count, max_extent)
TABLE = [
    (-3.0, 0.0, 5e-4, 5.0, 5.0),    # 0 cool (5e-4 < 2e-4 * 5): keep
    (-3.0, 0.0, 1e-2, 5.0, 5.0),    # 1 hot, small: clone
    (0.3, 0.0, 1e-2, 5.0, 25.0),    # 2 hot, big; the children pass the world test (0.3 - log 1.6 < 0): split, always
    (-3.0, -6.0, 0.0, 5.0, 5.0),    # 3 faint: prune
    (-3.0, -6.0, 1e-2, 5.0, 5.0),   # 4 hot + faint: prune (the lineage clones it, then prunes both)
    (0.6, 0.0, 1e-2, 5.0, 5.0),     # 5 hot, big, child 0.6 - log 1.6 > 0 fails the world test: split / prune
    (-3.0, 0.0, 1.0, 0.0, 0.0),     # 6 never seen (count == 0) with a stale sum: keep
    (-3.0, 0.0, 0.0, 5.0, 25.0),    # 7 cool, screen extent 25 > 20: keep / prune
    (0.2, 0.0, 0.0, 5.0, 5.0),      # 8 cool, world size 0.2 > 0: keep / prune
    (-3.0, 0.0, 1e-2, 5.0, 30.0),   # 9 hot, small, screen extent 30 > 20: clone / prune
]


def _table():
    t = torch.tensor(TABLE, dtype=torch.float32)
    log_scales = torch.stack([t[:, 0], t[:, 0] - 0.5, torch.zeros(len(TABLE))], dim=1)
    log_scales[1] = torch.tensor([-3.5, -3.0, 0.0])  # (the maximum may sit in either column)
    return log_scales, t[:, 1:2].contiguous(), t[:, 2].contiguous(), t[:, 3].contiguous(), t[:, 4].contiguous()


def test_thresholds_are_fp32_roundings_of_the_double_values():
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert TH == dict(grad_threshold=f32(2e-4), log_big=f32(math.log(0.1)), logit_faint=f32(math.log(0.005 / 0.995)),
                      max_screen_px=20.0, log_world=0.0, log_split=f32(math.log(1.6)))
    for bad in (dict(extent=0.0), dict(extent=float("inf")), dict(extent=1.0, min_opacity=0.0),
                dict(extent=1.0, grad_threshold=-1.0)):
        with pytest.raises(ValueError):
            dn.density_thresholds(**bad)


def test_plan_twin_on_the_hand_written_table():
    ls, op, gs, cnt, me = _table()
    # before reset_every: no size pruning
    rows, kind, offsets = dn.density_plan_eager(ls, op, gs, cnt, me, TH, size_prune=False)
    assert kind.tolist() == [KEEP, CLONE, SPLIT, PRUNE, PRUNE, SPLIT, KEEP, KEEP, KEEP, CLONE]
    assert rows.tolist() == [1, 2, 2, 0, 0, 2, 1, 1, 1, 2]
    assert offsets.tolist() == [0, 1, 3, 5, 5, 5, 7, 8, 9, 10, 12]
    assert rows.dtype == kind.dtype == offsets.dtype == torch.int32
    # after: the failing child, both size candidates and the hot splat with a large screen record go
    rows, kind, offsets = dn.density_plan_eager(ls, op, gs, cnt, me, TH, size_prune=True)
    assert kind.tolist() == [KEEP, CLONE, SPLIT, PRUNE, PRUNE, PRUNE, KEEP, PRUNE, PRUNE, PRUNE]
    assert rows.tolist() == [1, 2, 2, 0, 0, 0, 1, 0, 0, 0]
    assert offsets.tolist() == [0, 1, 3, 5, 5, 5, 5, 6, 6, 6, 6]
    # the cap's prune-only plan: every hot splat is planned as if it were not hot
    rows, kind, offsets = dn.density_plan_eager(ls, op, gs, cnt, me, TH, size_prune=False, prune_only=True)
    assert kind.tolist() == [KEEP, KEEP, KEEP, PRUNE, PRUNE, KEEP, KEEP, KEEP, KEEP, KEEP]
    assert int(offsets[-1]) == 8
    # an exact tie counts as hot (>=): grad_sum == fp32(grad_threshold) * count
    tie = torch.tensor([TH["grad_threshold"]], dtype=torch.float32) * cnt[1:2]
    assert dn.density_plan_eager(ls[1:2], op[1:2], tie, cnt[1:2], me[1:2], TH, False)[1].tolist() == [CLONE]


def test_plan_event_applies_the_cap():
    ls, op, gs, cnt, me = _table()
    plan = dn.plan_event(ls, op, gs, cnt, me, TH, False)
    assert (plan.n_new, plan.kept, plan.cloned, plan.split, plan.pruned, plan.prune_only) == (12, 4, 2, 2, 2, False)
    assert dn.plan_event(ls, op, gs, cnt, me, TH, False, max_splats=12).n_new == 12
    capped = dn.plan_event(ls, op, gs, cnt, me, TH, False, max_splats=11)
    assert (capped.n_new, capped.kept, capped.cloned, capped.split, capped.pruned, capped.prune_only) == \
        (8, 8, 0, 0, 2, True)
    assert dn.plan_event(ls, op, gs, cnt, me, TH, False, check=torch.tensor(True)).flagged
    assert not plan.flagged


def _f(x):
    return np.float32(x)


def test_apply_twin_layout_moments_and_children():
    ls, op, gs, cnt, me = _table()
    n = ls.shape[0]
    rows, kind, offsets = dn.density_plan_eager(ls, op, gs, cnt, me, TH, size_prune=False)
    g = torch.Generator().manual_seed(11)
    means = torch.randn((n, 3), generator=g)
    quats = torch.randn((n, 4), generator=g)
    quats_n = quats / quats.norm(dim=-1, keepdim=True)
    scales = torch.cat([torch.exp(ls[:, :2]), torch.zeros(n, 1)], dim=1)
    noise = torch.randn((n, 2, 2), generator=g)
    ids = torch.arange(n, dtype=torch.float32)[:, None]
    rest = torch.randn((n, 15, 3), generator=g)
    m1, m2 = torch.rand((n, 3), generator=g) + 1.0, torch.rand((n, 3), generator=g) + 1.0
    named = {"ids": (ids, dn.ROLE_COPY), "means": (means, dn.ROLE_MEANS), "ls": (ls, dn.ROLE_LOG_SCALES),
             "rest": (rest, dn.ROLE_COPY), "m1": (m1, dn.ROLE_MOMENT), "m2": (m2, dn.ROLE_MOMENT),
             "empty": (torch.zeros((n, 0, 3)), dn.ROLE_COPY)}
    out = dn.density_apply_eager(rows, kind, offsets, named, scales, quats_n, noise, TH["log_split"])
    # source order: keep then clone, child 0 then child 1, pruned splats absent
    src = [0, 1, 1, 2, 2, 5, 5, 6, 7, 8, 9, 9]
    assert out["ids"][:, 0].tolist() == [float(i) for i in src]
    assert tuple(out["rest"].shape) == (12, 15, 3) and torch.equal(out["rest"], rest[src])
    assert tuple(out["empty"].shape) == (12, 0, 3)
    # kept rows carry their moments, clone rows and split children start at zero
    kept_rows = [0, 1, 7, 8, 9, 10]   # splats 0, 1 (first row), 6, 7, 8, 9 (first row)
    new_rows = [2, 3, 4, 5, 6, 11]    # the clone of 1, the children of 2 and 5, the clone of 9
    for name, m in (("m1", m1), ("m2", m2)):
        assert torch.equal(out[name][kept_rows], m[[0, 1, 6, 7, 8, 9]])
        assert torch.equal(out[name][new_rows], torch.zeros(6, 3))
    # log-scales: the children's first two columns shrink by fp32(log 1.6), one rounded subtraction; all else copied
    log16 = _f(math.log(1.6))
    for row, i in ((3, 2), (4, 2), (5, 5), (6, 5)):
        want = [float(_f(ls[i, 0]) - log16), float(_f(ls[i, 1]) - log16), float(ls[i, 2])]
        assert out["ls"][row].tolist() == want
    assert torch.equal(out["ls"][[0, 1, 2, 7, 8, 9, 10, 11]], ls[[0, 1, 1, 6, 7, 8, 9, 9]])
    # centres: clones sit on their source; child k of splat i by hand, every line one rounded fp32 operation
    assert torch.equal(out["means"][[0, 1, 2, 7, 8, 9, 10, 11]], means[[0, 1, 1, 6, 7, 8, 9, 9]])
    for row, i, k in ((3, 2, 0), (4, 2, 1), (5, 5, 0), (6, 5, 1)):
        w, x, y, z = (_f(v) for v in quats_n[i].tolist())
        nrm = np.sqrt(_f(_f(_f(w * w) + _f(x * x)) + _f(y * y)) + _f(z * z))
        w, x, y, z = _f(w / nrm), _f(x / nrm), _f(y / nrm), _f(z / nrm)
        one, two = _f(1), _f(2)
        col0 = [_f(one - _f(two * _f(_f(y * y) + _f(z * z)))), _f(two * _f(_f(x * y) + _f(w * z))),
                _f(two * _f(_f(x * z) - _f(w * y)))]
        col1 = [_f(two * _f(_f(x * y) - _f(w * z))), _f(one - _f(two * _f(_f(x * x) + _f(z * z)))),
                _f(two * _f(_f(y * z) + _f(w * x)))]
        a = _f(_f(scales[i, 0]) * _f(noise[i, k, 0]))
        b = _f(_f(scales[i, 1]) * _f(noise[i, k, 1]))
        want = [float(_f(_f(means[i, c]) + _f(_f(col0[c] * a) + _f(col1[c] * b)))) for c in range(3)]
        assert out["means"][row].tolist() == want, (row, i, k)
        assert not torch.equal(out["means"][row], means[i])


def test_accum_twin_by_hand_and_guard():
    from gstex_amd.scene import sphere_view

    view = sphere_view(1, 64, 80)
    g = torch.Generator().manual_seed(5)
    n = 6
    means, grad = torch.randn((n, 3), generator=g), 1e-3 * torch.randn((n, 3), generator=g)
    nth = torch.tensor([3, 0, 1, 0, 7, 2], dtype=torch.int32)
    extents = 10.0 * torch.rand((n, 2), generator=g)
    zeros = torch.zeros(n)
    gs, cnt, me = dn.density_accum_eager(means, grad, view.viewmat, view.fx, view.fy, 64, 80, nth, extents, zeros, zeros,
                                         zeros)
    V = view.viewmat.numpy()
    for i in range(n):
        if nth[i] == 0:
            assert (gs[i], cnt[i], me[i]) == (0.0, 0.0, 0.0)
            continue
        x, y, zw = (_f(v) for v in means[i].tolist())
        gx, gy, gz = (_f(v) for v in grad[i].tolist())
        z = _f(_f(_f(_f(V[2, 0] * x) + _f(V[2, 1] * y)) + _f(V[2, 2] * zw)) + V[2, 3])
        gcx = _f(_f(_f(V[0, 0] * gx) + _f(V[0, 1] * gy)) + _f(V[0, 2] * gz))
        gcy = _f(_f(_f(V[1, 0] * gx) + _f(V[1, 1] * gy)) + _f(V[1, 2] * gz))
        ax = _f(_f(_f(gcx * z) / _f(view.fx)) * _f(40.0))
        ay = _f(_f(_f(gcy * z) / _f(view.fy)) * _f(32.0))
        assert float(gs[i]) == float(np.sqrt(_f(_f(ax * ax) + _f(ay * ay))))
        assert float(cnt[i]) == 1.0 and float(me[i]) == float(extents[i].max())
    # a second call accumulates; a set guard flag changes nothing
    gs2, cnt2, me2 = dn.density_accum_eager(means, grad, view.viewmat, view.fx, view.fy, 64, 80, nth, extents, gs, cnt,
                                            me)
    assert torch.equal(gs2, gs + gs) and torch.equal(cnt2, 2 * cnt) and torch.equal(me2, me)
    held = dn.density_accum_eager(means, grad, view.viewmat, view.fx, view.fy, 64, 80, nth, extents, gs, cnt, me,
                                  skip=torch.ones(1))
    assert all(torch.equal(a, b) for a, b in zip(held, (gs, cnt, me)))


def test_scene_extent_and_stage_settings():
    from gstex_amd.scene import sphere_view
    from gstex_amd.train import _COMMON_LRS, PRESETS

    views = [sphere_view(i, 32, 32, n_views=6) for i in range(6)]
    centres = np.stack([v.c2w[:3, 3].double().numpy() for v in views])
    want = 1.1 * np.linalg.norm(centres - centres.mean(0), axis=1).max()
    assert dn.scene_extent(views) == pytest.approx(want, rel=1e-12)
    st = dn.GEOMETRY_STAGE
    assert st["max_steps"] == 30000 and st["lrs"] == _COMMON_LRS and st["lambda_normal"] == [0.0, 0.05, 7000]
    assert dn.geometry_stage_lrs(2.5) == {"xyz": 1.6e-4 * 2.5, **_COMMON_LRS}
    assert st["xyz_lr_final"] == 1.6e-6
    assert st["density"] == dict(grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_screen_px=20.0,
                                 start=500, stop=15000, every=100, reset_every=3000)
    assert "geometry" not in " ".join(PRESETS)  # the stage is not one of the reference's presets


# ---------------------------------------------------------------------------------------- fit
class _RecordingDensity:
    def accumulate(self, trainer, view):
        trainer.calls.append(("accumulate", trainer.step, view.tag))

    def update(self, trainer):
        trainer.calls.append(("update", trainer.step))
        return ("event", trainer.step) if trainer.step % 2 == 0 else None


def test_fit_with_a_controller_orders_the_step():
    from gstex_amd.model import LRS
    from gstex_amd.train import fit
    from test_train_loop import _RecordingTrainer, _View

    pairs = [(_View(k), torch.tensor([k])) for k in range(3)]
    tr = _RecordingTrainer(start_step=4)
    res = fit(tr, pairs, 5, build_chart_every=0, seed=3, density=_RecordingDensity())
    want = []
    for i, k in enumerate(res["views"]):
        s = 4 + i
        want += [("zero_grad", s), ("forward_backward", s, k, k, None), ("accumulate", s, k),
                 ("optimizer_step", s, LRS["xyz"], LRS["texture_dc"]), ("update", s + 1)]
    assert tr.calls == want
    assert res["density"] == [("event", 6), ("event", 8)] and res["recharts"] == []
    # a rechart cadence cannot be combined with density control
    for every in (100, 1):
        with pytest.raises(ValueError, match="build_chart_every"):
            fit(_RecordingTrainer(), pairs, 1, build_chart_every=every, density=_RecordingDensity())
    fit(_RecordingTrainer(), pairs, 1, build_chart_every=None, density=_RecordingDensity())
    # density=None: today's sequence, and no density key
    a, b = _RecordingTrainer(start_step=4), _RecordingTrainer(start_step=4)
    ra = fit(a, pairs, 5, build_chart_every=2, seed=3)
    rb = fit(b, pairs, 5, build_chart_every=2, seed=3, density=None)
    assert a.calls == b.calls and "density" not in ra and "density" not in rb
    assert [c[0] for c in a.calls[:4]] == ["zero_grad", "forward_backward", "optimizer_step", "recharge"]


# ---------------------------------------------------------------------------------------- trainer, export
def _one_texel_trainer(n=40, sh_degree=1, seed=3):
    from gstex_amd.init import _seeded_scene
    from gstex_amd.model import GStexTrainer

    g = torch.Generator().manual_seed(seed)
    means = torch.rand((n, 3), generator=g) - 0.5
    sc = _seeded_scene(means, torch.rand((n, 3), generator=g), sh_degree, seed=seed)
    sc.features_rest = 0.1 * torch.randn(sc.features_rest.shape, generator=g)
    sc.log_scales[:, 2] = 1.0  # (2DGS stores two scales; its reader supplies ones for the third column)
    tr = GStexTrainer(sc, "cpu", sh_degree=sh_degree, fused_adam=False)
    with torch.no_grad():
        tr.texture_dc.copy_(sc.features_dc)
    return tr, sc, g


def test_export_2dgs_ply_round_trip(tmp_path):
    from gstex_amd.export import export_2dgs_ply
    from gstex_amd.init import scene_from_2dgs_ply
    from gstex_amd.model import GStexTrainer
    from gstex_amd.ply import read_ply
    from gstex_amd.scene import make_scene

    tr, sc, _ = _one_texel_trainer(sh_degree=2)
    path = tmp_path / "stage.ply"
    export_2dgs_ply(tr, path)
    cols = read_ply(path)
    names = list(cols)
    assert names[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    assert names[9:33] == [f"f_rest_{k}" for k in range(24)]
    assert names[33:] == ["opacity", "scale_0", "scale_1", "rot_0", "rot_1", "rot_2", "rot_3"]
    assert all(v.dtype == np.float32 for v in cols.values()) and not cols["nx"].any()
    back = scene_from_2dgs_ply(path, sh_degree=2)
    for got, want in ((back.means, tr.means), (back.log_scales, tr.scales), (back.quats, tr.quats),
                      (back.opacity_logits, tr.opacities), (back.features_dc, tr.texture_dc),
                      (back.features_rest, tr.features_rest)):
        assert torch.equal(got, want.detach())
    assert torch.equal(back.texture_dims, tr.texture_dims) and torch.equal(back.mappings, tr.mappings)
    with pytest.raises(ValueError, match="one colour per splat"):
        export_2dgs_ply(GStexTrainer(make_scene(30, 300, seed=1), "cpu", fused_adam=False), tmp_path / "no.ply")


def _stats_for(tr, g):
    n = tr.means.shape[0]
    count = torch.full((n,), 4.0)
    grad_sum = torch.where(torch.rand(n, generator=g) < 0.5, torch.full((n,), 1.0), torch.zeros(n))  # half are hot
    return grad_sum, count, torch.zeros(n), torch.randn((n, 2, 2), generator=g)


def test_apply_density_on_a_cpu_trainer():
    tr, sc, g = _one_texel_trainer()
    n = 40
    for p in tr.parameters():  # one Adam step, so that the optimizer holds moments
        p.grad = torch.randn(p.shape, generator=g)
    tr.optimizer.step()
    with torch.no_grad():
        tr.opacities[:5] = -7.0  # faint
        tr.scales[5:20, :2] += 3.0  # big for this extent
    grad_sum, count, max_extent, noise = _stats_for(tr, g)
    th = dn.density_thresholds(float(torch.exp(tr.scales.detach()[:, :2]).median()) * 300)
    before = {k: ps[0].detach().clone() for k, ps in tr.param_groups().items()}
    moments = {k: (tr.optimizer.state[ps[0]]["exp_avg"].clone(), tr.optimizer.state[ps[0]]["exp_avg_sq"].clone(),
                   tr.optimizer.state[ps[0]]["step"]) for k, ps in tr.param_groups().items()}
    # the twins, called directly on the same inputs
    rows, kind, offsets = dn.density_plan_eager(before["scaling"], before["opacity"], grad_sum, count, max_extent, th,
                                                False)
    assert {KEEP, CLONE, SPLIT, PRUNE} == set(kind.tolist())
    quats_n = before["rotation"] / before["rotation"].norm(dim=-1, keepdim=True)
    s = torch.exp(before["scaling"][:, :2]).clamp(min=1e-9)
    scales = torch.cat([s, 1e-5 * s.mean(dim=-1, keepdim=True)], dim=-1)
    roles = {"xyz": dn.ROLE_MEANS, "scaling": dn.ROLE_LOG_SCALES}
    named = {k: (v, roles.get(k, dn.ROLE_COPY)) for k, v in before.items()}
    for k, (m, v, _) in moments.items():
        named[k + ".m"], named[k + ".v"] = (m, dn.ROLE_MOMENT), (v, dn.ROLE_MOMENT)
    want = dn.density_apply_eager(rows, kind, offsets, named, scales, quats_n, noise, th["log_split"])

    plan = tr.apply_density(grad_sum, count, max_extent, noise, th, size_prune=False)
    m = int(offsets[-1])
    assert plan.n_new == m != n and torch.equal(plan.kind, kind)
    assert (plan.kept, plan.cloned, plan.split, plan.pruned) == tuple(int((kind == k).sum()) for k in range(4))
    groups = tr.param_groups()
    for g_ in tr.optimizer.param_groups:
        p = groups[g_["name"]][0]
        assert g_["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert torch.equal(p.detach(), want[g_["name"]]), g_["name"]
        st = tr.optimizer.state[p]
        assert torch.equal(st["exp_avg"], want[g_["name"] + ".m"]) and torch.equal(st["exp_avg_sq"], want[g_["name"] + ".v"])
        assert st["step"] == moments[g_["name"]][2]
    assert len(tr.optimizer.state) == 7
    assert tr.n_texels == m and tr.texture_dims.tolist() == [[1, 1, i] for i in range(m)]
    assert torch.equal(tr.mappings, 1.0 / (2.0 * 3.0 * torch.exp(tr.scales.detach()[:, :2])))
    # the geometry parameters are views of the new flat allocation, segments 16-byte aligned
    base = tr.geometry_flat.data_ptr()
    for p in (tr.means, tr.scales, tr.quats, tr.opacities):
        assert (p.data_ptr() - base) % 16 == 0 and 0 <= p.data_ptr() - base < 4 * tr.geometry_flat.numel()
    # the trainer still steps
    for p in tr.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    tr.optimizer.step()
    # opacity reset: logits capped at logit(0.01), the opacity moments zeroed
    with torch.no_grad():
        tr.opacities[:3] = 2.0
        tr.opacities[3] = -8.0
    prev = tr.opacities.detach().clone()
    tr.reset_opacity(0.01)
    cap = math.log(0.01 / 0.99)
    assert torch.equal(tr.opacities.detach(), torch.clamp(prev, max=cap))
    assert float(tr.opacities.max()) == float(np.float32(cap)) and float(tr.opacities.min()) == -8.0
    st = tr.optimizer.state[tr.opacities]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert tr.opacities.data_ptr() - tr.geometry_flat.data_ptr() > 0  # (still a view of the flat allocation)


def test_apply_density_refuses_what_it_cannot_do():
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene

    tr, sc, g = _one_texel_trainer()
    n = 40
    grad_sum, count, max_extent, noise = _stats_for(tr, g)
    th = dn.density_thresholds(1.0)
    snapshot = {k: (ps[0], ps[0].detach().clone()) for k, ps in tr.param_groups().items()}
    flat = tr.geometry_flat
    # every splat faint: n_new == 0 raises and leaves the trainer untouched
    with torch.no_grad():
        tr.opacities.fill_(-9.0)
        snapshot["opacity"] = (tr.opacities, tr.opacities.detach().clone())
    with pytest.raises(RuntimeError, match="prune every splat"):
        tr.apply_density(grad_sum, count, max_extent, noise, th, size_prune=False)
    assert tr.geometry_flat is flat and tr.n_texels == n
    for k, ps in tr.param_groups().items():
        assert ps[0] is snapshot[k][0] and torch.equal(ps[0].detach(), snapshot[k][1]), k
    # an all-keep event changes no tensor
    with torch.no_grad():
        tr.opacities.fill_(0.0)
    plan = tr.apply_density(torch.zeros(n), count, max_extent, noise, th, size_prune=False)
    assert plan.n_new == n and plan.kept == n and tr.geometry_flat is flat
    assert all(ps[0] is snapshot[k][0] for k, ps in tr.param_groups().items())
    # charts with more than one texel per splat, a wrong chart order, wrong statistics
    multi = GStexTrainer(make_scene(30, 300, seed=1), "cpu", fused_adam=False)
    z = torch.zeros(30)
    with pytest.raises(ValueError, match="one-texel"):
        multi.apply_density(z, z, z, torch.zeros(30, 2, 2), th, size_prune=False)
    tr.texture_dims[3, 2] = 7
    with pytest.raises(ValueError, match="one-texel"):
        tr.apply_density(grad_sum, count, max_extent, noise, th, size_prune=False)
    tr.texture_dims[3, 2] = 3
    with pytest.raises(ValueError, match="grad_sum"):
        tr.apply_density(grad_sum[:5], count, max_extent, noise, th, size_prune=False)
    # a trainer whose texel gradient is routed (GradSync) refuses
    tr.texel_grad.attach(torch.zeros_like(tr.texture_dc), None, lambda first: (None, False, None))
    with pytest.raises(RuntimeError, match="GradSync"):
        tr.apply_density(grad_sum, count, max_extent, noise, th, size_prune=False)


def test_controller_schedule_on_a_cpu_trainer():
    """DensityController.update: events at s > start with s % every == 0 while s < stop, size pruning once
    s > reset_every, the reset at multiples of reset_every; the statistics are n_new zeros after an event."""
    tr, sc, g = _one_texel_trainer()
    calls = []

    class _Plan:
        n_new, cloned, split, pruned = 44, 3, 1, 2

    tr.apply_density = lambda *a, **k: calls.append(("event", tr.step, k["size_prune"], k["max_splats"])) or _Plan()
    tr.reset_opacity = lambda v: calls.append(("reset", tr.step, v))
    ctl = dn.DensityController(40, "cpu", 5.0, start=4, stop=13, every=2, reset_every=6, max_splats=99, seed=1)
    got = []
    for s in range(1, 16):
        tr.step = s
        ctl.count += 1.0
        got.append(ctl.update(tr))
        if got[-1] is not None:  # after any event the three statistics arrays are n_new zeros
            for t in (ctl.grad_sum, ctl.count, ctl.max_extent):
                assert tuple(t.shape) == (44,) and not t.any()
    assert calls == [("event", 6, False, 99), ("reset", 6, 0.01), ("event", 8, True, 99), ("event", 10, True, 99),
                     ("event", 12, True, 99), ("reset", 12, 0.01)]
    assert [e for e in got if e is not None] == ctl.events == [
        dn.DensityEvent(s, 40, 44, 3, 1, 2) for s in (6, 8, 10, 12)]
