"""gstex_amd.select without a GPU: the eager twin against a plain loop on the standard chart list under the standard
masks, cluster.keep_mask on hand-written labels, the C ABI of the three entry points (declared, exported, bound,
refusals before any launch) and GStexTrainer.select on a CPU trainer (through the twins)."""
import ctypes
import os

import pytest
import torch

from gstex_amd import _lib
from gstex_amd import select as sel
from select_cases import MASK_NAMES, chart_list, loop_select, masks, sources

NEW = ("gstex_select_plan", "gstex_select_dims", "gstex_select_texels")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mask", MASK_NAMES)
def test_twin_equals_the_loop(mask, reverse):
    dims, T = chart_list(600, reverse=reverse)
    assert T == 60 * 1901 == 114060
    keep = masks(dims)[mask]
    src = sources(T)
    want_dims, want, want_T = loop_select(dims, keep, src)
    new_dims, new, T_new = sel.select_texture_eager(dims, T, keep, src)
    assert T_new == want_T and torch.equal(new_dims, want_dims)
    assert len(new) == 3 and all(torch.equal(a, b) for a, b in zip(new, want))
    assert all(tuple(t.shape) == (T_new, 3) for t in new)
    size = new_dims[:, 0].long() * new_dims[:, 1].long()
    assert torch.equal(new_dims[:, 2].long(), torch.cumsum(size, 0) - size)
    if mask == "zero_texel_only":
        assert T_new == 0 and new_dims.shape[0] == 120
    if mask == "all" and not reverse:
        assert torch.equal(new_dims, dims) and torch.equal(new[0], src[0][:T])
    # select_texture on CPU tensors runs the same twin; the plan's pieces are consistent with it
    d2, n2, t2 = sel.select_texture(dims, T, keep, src)
    assert t2 == T_new and torch.equal(d2, new_dims) and all(torch.equal(a, b) for a, b in zip(n2, new))
    plan = sel.plan_selection(dims, T, keep)
    assert (plan.n_new, plan.n_texels_new, plan.flagged) == (int(keep.sum()), T_new, False)
    assert torch.equal(plan.rows, keep.to(torch.int32)) and int(plan.row_off[-1]) == plan.n_new


def test_twin_flags_each_malformed_kind_and_checks_its_arguments():
    dims, T = chart_list(20)
    keep = torch.ones(20, dtype=torch.bool)
    keep[3] = False  # (a dropped row is checked as well)
    for row in ((-1, 5, 0), (3, -5, 0), (3, 5, -1), (65536, 65536, 0), (3, 5, T - 14)):
        bad = dims.clone()
        bad[3] = torch.tensor(row, dtype=torch.int32)
        assert int(sel.select_plan_eager(bad, T, keep)[4]) == 1, row
        with pytest.raises(ValueError, match="malformed"):
            sel.select_texture_eager(bad, T, keep, sources(T, count=1))
    ok = dims.clone()
    ok[3] = torch.tensor((3, 5, T - 15), dtype=torch.int32)  # the last block that still fits
    assert int(sel.select_plan_eager(ok, T, keep)[4]) == 0
    with pytest.raises(ValueError, match="keep"):
        sel.select_texture_eager(dims, T, keep[:5], [])
    with pytest.raises(ValueError, match="keep"):
        sel.select_texture_eager(dims, T, keep.float(), [])
    with pytest.raises(ValueError, match="texture_dims"):
        sel.select_texture_eager(dims.long(), T, keep, [])


# ---------------------------------------------------------------------------------------- keep_mask
def test_keep_mask_on_hand_written_labels():
    from gstex_amd.cluster import ClusterResult, keep_mask

    lab = torch.tensor([1, 1, 1, -1, 2, 2, 3, -1, 1, 3, 3, 3], dtype=torch.int32)  # sizes 4, 2, 4; two noise
    b = lambda *idx: torch.zeros(12, dtype=torch.bool).index_fill_(0, torch.tensor(idx, dtype=torch.int64), True)  # noqa: E731
    assert torch.equal(keep_mask(lab), lab >= 1)
    assert torch.equal(keep_mask(lab, drop_noise=False), torch.ones(12, dtype=torch.bool))
    assert torch.equal(keep_mask(lab, min_size=3), b(0, 1, 2, 8, 6, 9, 10, 11))
    assert torch.equal(keep_mask(lab, min_size=3, drop_noise=False), b(0, 1, 2, 8, 6, 9, 10, 11, 3, 7))
    assert torch.equal(keep_mask(lab, min_size=5), torch.zeros(12, dtype=torch.bool))
    assert torch.equal(keep_mask(lab, labels=[2]), b(4, 5))
    assert torch.equal(keep_mask(lab, labels=torch.tensor([3, 2])), b(4, 5, 6, 9, 10, 11))
    assert torch.equal(keep_mask(lab, labels=[1], drop_noise=False), b(0, 1, 2, 8, 3, 7))
    assert torch.equal(keep_mask(lab, labels=[7]), torch.zeros(12, dtype=torch.bool))
    res = ClusterResult(lab, torch.zeros(12, dtype=torch.int32), lab >= 1, 3)
    assert torch.equal(keep_mask(res, min_size=3), keep_mask(lab, min_size=3))
    got = keep_mask(res, labels=[1])
    assert got.dtype == torch.bool and got.device == lab.device and torch.equal(got, b(0, 1, 2, 8))
    assert torch.equal(keep_mask(torch.full((4,), -1, dtype=torch.int32)), torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="min_size"):
        keep_mask(lab, min_size=0)
    with pytest.raises(ValueError, match="cluster ids"):
        keep_mask(lab, labels=[-1])


# ---------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "gstex_hip.h")).read()
    for s in NEW:
        assert f"int {s}(" in header and hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert "#define GSTEX_ABI_VERSION 19" in header
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19
    assert f"#define GSTEX_SELECT_MAX_TENSORS {_lib.SELECT_MAX_TENSORS}" in header and _lib.SELECT_MAX_TENSORS >= 3
    assert "select.hip" in open(os.path.join(ROOT, "gstex_amd", "csrc", "Makefile")).read()


def test_struct_layouts_match_header(tmp_path):
    import subprocess

    structs = {"gstex_select_plan_args": _lib.GstexSelectPlanArgs, "gstex_select_dims_args": _lib.GstexSelectDimsArgs,
               "gstex_select_pair": _lib.GstexSelectPair, "gstex_select_texels_args": _lib.GstexSelectTexelsArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[f"{cname} size"]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got[f"{cname} {f[0]}"]) == getattr(cls, f[0]).offset, f"{cname}.{f[0]}"


def _buf():
    """A host word array's address: compared, null- and alignment-checked only (rejected before any launch)."""
    keep = (ctypes.c_float * 64)()
    return keep, ctypes.addressof(keep)


def _status(lib, name, args):
    rc = getattr(lib, name)(ctypes.byref(args) if args is not None else None, None)
    return rc, _lib.last_error()


def test_plan_and_dims_reject_bad_arguments(lib):
    hold, b = _buf()
    hold2, b2 = _buf()
    P = lambda **kw: _lib.GstexSelectPlanArgs(**{**dict(n=4, n_texels=10, keep=b, texture_dims=b, rows=b, texels=b,  # noqa: E731
                                                        flag=b), **kw})
    rc, msg = _status(lib, "gstex_select_plan", None)
    assert rc == 1 and "gstex_select_plan: null args" in msg
    rc, msg = _status(lib, "gstex_select_plan", P(n=-1))
    assert rc == 1 and "n < 0" in msg
    for bad in (-1, 1 << 31):
        rc, msg = _status(lib, "gstex_select_plan", P(n_texels=bad))
        assert rc == 1 and "n_texels" in msg, bad
    for field in ("keep", "texture_dims", "rows", "texels", "flag"):
        rc, msg = _status(lib, "gstex_select_plan", P(**{field: None}))
        assert rc == 1 and "null pointer" in msg and field in msg, field
    for field in ("texture_dims", "rows", "texels", "flag"):
        rc, msg = _status(lib, "gstex_select_plan", P(**{field: b + 2}))
        assert rc == 1 and "misaligned" in msg and field in msg, field
    assert _status(lib, "gstex_select_plan", P(n=0, keep=None, texture_dims=None, rows=None, texels=None))[0] == 0

    D = lambda **kw: _lib.GstexSelectDimsArgs(**{**dict(n=4, n_new=2, keep=b, texture_dims=b, row_off=b, tex_off=b,  # noqa: E731
                                                        new_dims=b2, src_off=b2), **kw})
    rc, msg = _status(lib, "gstex_select_dims", None)
    assert rc == 1 and "gstex_select_dims: null args" in msg
    rc, msg = _status(lib, "gstex_select_dims", D(n=-1))
    assert rc == 1 and "n < 0" in msg
    for bad in (-1, 5):
        rc, msg = _status(lib, "gstex_select_dims", D(n_new=bad))
        assert rc == 1 and "n_new" in msg, bad
    for field in ("keep", "texture_dims", "row_off", "tex_off", "new_dims", "src_off"):
        rc, msg = _status(lib, "gstex_select_dims", D(**{field: None}))
        assert rc == 1 and "null pointer" in msg and field in msg, field
    for field in ("texture_dims", "row_off", "tex_off", "new_dims", "src_off"):
        rc, msg = _status(lib, "gstex_select_dims", D(**{field: b + 2}))
        assert rc == 1 and "misaligned" in msg, field
    rc, msg = _status(lib, "gstex_select_dims", D(new_dims=b))
    assert rc == 1 and "must differ" in msg
    assert _status(lib, "gstex_select_dims", D(n=0, n_new=0))[0] == 0
    assert _status(lib, "gstex_select_dims", D(n_new=0, new_dims=None, src_off=None))[0] == 0
    del hold, hold2


def test_texels_rejects_bad_arguments(lib):
    hold, b = _buf()
    hold2, b2 = _buf()
    Pair = _lib.GstexSelectPair

    def T(pairs=((b, b2),), **kw):
        a = _lib.GstexSelectTexelsArgs(**{**dict(n_new=2, channels=3, n_tensors=len(pairs), n_texels_new=4,
                                                 n_texels=10, new_dims=b, src_off=b), **kw})
        for k, (s, d) in enumerate(pairs[:_lib.SELECT_MAX_TENSORS]):
            a.tensors[k] = Pair(s, d)
        return a

    rc, msg = _status(lib, "gstex_select_texels", None)
    assert rc == 1 and "gstex_select_texels: null args" in msg
    rc, msg = _status(lib, "gstex_select_texels", T(n_new=-1))
    assert rc == 1 and "n_new < 0" in msg
    for bad in (0, 9, -3):
        rc, msg = _status(lib, "gstex_select_texels", T(channels=bad))
        assert rc == 1 and "channels must be in [1, 8]" in msg, bad
    for bad in (_lib.SELECT_MAX_TENSORS + 1, -1):
        rc, msg = _status(lib, "gstex_select_texels", T(n_tensors=bad))
        assert rc == 1 and "n_tensors must be in" in msg, bad
    for field in ("n_texels", "n_texels_new"):
        for bad in (-1, 1 << 31):
            rc, msg = _status(lib, "gstex_select_texels", T(**{field: bad}))
            assert rc == 1 and "n_texels" in msg, (field, bad)
    rc, msg = _status(lib, "gstex_select_texels", T(n_new=0))
    assert rc == 1 and "needs n_new > 0" in msg
    for field in ("new_dims", "src_off"):
        rc, msg = _status(lib, "gstex_select_texels", T(**{field: None}))
        assert rc == 1 and "null pointer" in msg and field in msg, field
        rc, msg = _status(lib, "gstex_select_texels", T(**{field: b + 2}))
        assert rc == 1 and "misaligned" in msg and field in msg, field
    for pairs, what in ((((None, b2),), "tensor 0: null pointer"), (((b, None),), "tensor 0: null pointer"),
                        (((b, b2), (b, None)), "tensor 1: null pointer"), (((b, b),), "tensor 0: src and dst must differ"),
                        (((b + 2, b2),), "tensor 0: misaligned"), (((b, b2 + 1),), "tensor 0: misaligned"),
                        (((b, b2), (b2, b), (b, b)), "tensor 2: src and dst must differ")):
        rc, msg = _status(lib, "gstex_select_texels", T(pairs=pairs))
        assert rc == 1 and what in msg, what
    # nothing to move: a success before any pointer is looked at
    assert _status(lib, "gstex_select_texels", T(pairs=(), new_dims=None, src_off=None))[0] == 0
    assert _status(lib, "gstex_select_texels", T(pairs=((None, None),), n_texels_new=0, new_dims=None))[0] == 0
    del hold, hold2


# ---------------------------------------------------------------------------------------- trainer
def _cpu_trainer(n=30, texels=300, seed=1):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene

    tr = GStexTrainer(make_scene(n, texels, seed=seed), "cpu", sh_degree=1, fused_adam=False)
    g = torch.Generator().manual_seed(seed)
    for _ in range(2):  # two Adam steps, so that the optimizer holds moments and a step count
        for p in tr.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        tr.optimizer.step()
    tr.step = 2
    return tr, g


def _snapshot(tr):
    snap = {}
    for name, (p,) in tr.param_groups().items():
        st = tr.optimizer.state[p]
        snap[name] = (p, p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), int(st["step"]))
    return snap


def test_select_on_a_cpu_trainer():
    tr, g = _cpu_trainer()
    n, T = 30, tr.n_texels
    dims = tr.texture_dims.clone()
    size = dims[:, 0].long() * dims[:, 1].long()
    assert int(size.max()) > 1 and T == int(size.sum()) and tr.texture_dc.shape[0] >= T  # multi-texel charts
    snap, mappings, flat = _snapshot(tr), tr.mappings.clone(), tr.geometry_flat
    keep = torch.rand(n, generator=g) < 0.6
    assert 0 < int(keep.sum()) < n
    kept = torch.nonzero(keep)[:, 0]
    _, _, pm, pv, _ = snap["texture_dc"]
    want_dims, (want_tex, want_m, want_v), want_T = loop_select(dims, keep, [snap["texture_dc"][1], pm, pv])

    res = tr.select(keep)
    m = int(keep.sum())
    assert isinstance(res, sel.Selection) and tuple(res) == (n, m, T, want_T)
    assert res.n_after == m and res.texels_after == want_T < T
    groups = tr.param_groups()
    for g_ in tr.optimizer.param_groups:
        name = g_["name"]
        p = groups[name][0]
        old, val, ea, eas, step = snap[name]
        assert g_["params"][0] is p and p is not old and isinstance(p, torch.nn.Parameter) and p.requires_grad
        st = tr.optimizer.state[p]
        assert int(st["step"]) == step == 2 and old not in tr.optimizer.state
        if name == "texture_dc":
            assert torch.equal(p.detach(), want_tex) and tuple(p.shape) == (want_T, 3)
            assert torch.equal(st["exp_avg"], want_m) and torch.equal(st["exp_avg_sq"], want_v)
        else:
            assert torch.equal(p.detach(), val[kept]), name
            assert torch.equal(st["exp_avg"], ea[kept]) and torch.equal(st["exp_avg_sq"], eas[kept]), name
    assert len(tr.optimizer.state) == 7
    assert torch.equal(tr.texture_dims, want_dims) and tr.n_texels == want_T
    new_size = tr.texture_dims[:, 0].long() * tr.texture_dims[:, 1].long()
    assert torch.equal(tr.texture_dims[:, 2].long(), torch.cumsum(new_size, 0) - new_size)
    assert torch.equal(tr.mappings, mappings[kept])  # gathered, not recomputed
    base = tr.geometry_flat.data_ptr()
    assert tr.geometry_flat is not flat
    for p in (tr.means, tr.scales, tr.quats, tr.opacities):
        assert (p.data_ptr() - base) % 16 == 0 and 0 <= p.data_ptr() - base < 4 * tr.geometry_flat.numel()
    # the trainer still renders nothing on the CPU, but it steps and selects again
    for p in tr.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    tr.optimizer.step()
    assert int(tr.optimizer.state[tr.texture_dc]["step"]) == 3
    again = tr.select(torch.arange(m) != 0)
    assert again.n_after == m - 1 and tr.n_texels == want_T - int(new_size[0])


def test_select_refusals_leave_the_trainer_untouched():
    tr, g = _cpu_trainer()
    n, T = 30, tr.n_texels
    snap, flat, dims, mappings = _snapshot(tr), tr.geometry_flat, tr.texture_dims, tr.mappings

    def untouched():
        assert tr.geometry_flat is flat and tr.n_texels == T and tr.texture_dims is dims and tr.mappings is mappings
        for name, (p,) in tr.param_groups().items():
            old, val, ea, eas, step = snap[name]
            st = tr.optimizer.state[p]
            assert p is old and torch.equal(p.detach(), val) and int(st["step"]) == step, name
            assert torch.equal(st["exp_avg"], ea) and torch.equal(st["exp_avg_sq"], eas), name
        for g_ in tr.optimizer.param_groups:
            assert g_["params"][0] is snap[g_["name"]][0]

    res = tr.select(torch.ones(n, dtype=torch.bool))  # all true: the same Parameter objects
    assert tuple(res) == (n, n, T, T)
    untouched()
    with pytest.raises(RuntimeError, match="every splat"):
        tr.select(torch.zeros(n, dtype=torch.bool))
    untouched()
    with pytest.raises(ValueError, match="keep"):
        tr.select(torch.ones(n - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="keep"):
        tr.select(torch.ones(n))
    with pytest.raises(ValueError, match="keep"):
        tr.select([True] * n)
    untouched()
    size = dims[:, 0].long() * dims[:, 1].long()
    row = int(torch.nonzero(size > 1)[0])
    good = int(dims[row, 2])
    dims[row, 2] = T - int(size[row]) + 1  # offset + h * w > n_texels
    keep = torch.ones(n, dtype=torch.bool)
    keep[row] = False  # (a malformed row is refused even when it is dropped)
    with pytest.raises(ValueError, match="malformed"):
        tr.select(keep)
    dims[row, 2] = good
    untouched()
    tr.texel_grad.attach(torch.zeros_like(tr.texture_dc), None, lambda first: (None, False, None))
    with pytest.raises(RuntimeError, match="GradSync"):
        tr.select(keep)
    untouched()
