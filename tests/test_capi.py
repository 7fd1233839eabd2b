"""C-ABI boundary checks that need no GPU: the library loads, exports every symbol include/gstex_hip.h
declares, and rejects invalid arguments (before any HIP call) with a status and a message."""
import ctypes
import os
import re

import pytest

from gstex_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gstex_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gstex_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_every_header_symbol_is_exported_and_bound(lib):
    syms = declared_symbols()
    assert len(syms) >= 29
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in gstex_hip.h but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature in gstex_amd/_lib.py"
    assert set(_lib.SIGNATURES) == set(syms), "ctypes signatures out of sync with the header"
    # ABI 19: the variant entry points are folded into their base calls
    for s in ("gstex_raster_fwd_zero", "gstex_raster_bwd_zero", "gstex_raster_setup_bwd_aabb",
              "gstex_bin_sort_ordered", "gstex_bin_sort_capped", "gstex_scan_offsets_guarded", "gstex_adam_step_ex",
              "gstex_adam_step_scaled", "gstex_adam_step_guarded"):
        assert s not in syms and not hasattr(lib, s), f"{s} was removed in ABI 19 but is still exported"


def test_abi_version(lib):
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19


def test_workspace_size_queries(lib):
    assert lib.gstex_scan_workspace_size(0) >= 4
    small = lib.gstex_bin_workspace_size(100, 1000, 64)
    big = lib.gstex_bin_workspace_size(100, 100000, 64)
    assert big > small > 0
    # keys (8 B) + scratch (8 B) + rank (4 B) per intersection dominate
    assert big - small >= 20 * (100000 - 1000) - 3 * 256


def _cam(H=32, W=32, block=16):
    return _lib.GstexCamera(None, None, 100.0, 100.0, 16.0, 16.0, H, W, block)


def _status(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, _lib.last_error()


def test_bin_sort_rejects_non16_block(lib):
    rc, msg = _status(lib, "gstex_bin_sort", 10, 10, None, None, None, None, 32, 32, 8, None, None, None, None, 0,
                      None, 0, None)
    assert rc == 1 and "block_width must be 16" in msg


def test_bin_sort_rejects_bad_flags(lib):
    # GSTEX_BIN_CAPPED without a tile_order, and flag bits the ABI does not define
    rc, msg = _status(lib, "gstex_bin_sort", 10, 10, None, None, None, None, 32, 32, 16, None, None, None, None,
                      _lib.BIN_CAPPED, None, 0, None)
    assert rc == 1 and "null tile_order" in msg
    rc, msg = _status(lib, "gstex_bin_sort", 10, 10, None, None, None, None, 32, 32, 16, None, None, None, None,
                      1 << 2, None, 0, None)
    assert rc == 1 and "unknown flags" in msg


def test_scan_rejects_negative_guard_capacity(lib):
    guard = _lib.GstexPairGuard(-1, None, None, 1)
    rc, msg = _status(lib, "gstex_scan_offsets", 0, None, None, None, 0, ctypes.byref(guard), None)
    assert rc == 1 and "capacity < 0" in msg


def _fwd_args(cam, channels=3, settings=0, **kw):
    return _lib.GstexRasterFwdArgs(scene=_lib.GstexRasterScene(cam=cam, channels=channels, settings=settings,
                                                               tex_scale=1.0), **kw)


def _bwd_args(cam, channels=3, settings=0, **kw):
    return _lib.GstexRasterBwdArgs(scene=_lib.GstexRasterScene(cam=cam, channels=channels, settings=settings,
                                                               tex_scale=1.0), **kw)


def test_raster_rejects_bad_channels_and_settings(lib):
    cam = _cam()
    rc, msg = _status(lib, "gstex_raster_fwd", ctypes.byref(_fwd_args(cam, channels=9)), None)
    assert rc == 1 and "channels" in msg
    rc, msg = _status(lib, "gstex_raster_fwd", ctypes.byref(_fwd_args(cam, settings=1 << 2)), None)
    assert rc == 3 and "unsupported settings" in msg
    rc, msg = _status(lib, "gstex_raster_bwd", ctypes.byref(_bwd_args(_cam(block=8))), None)
    assert rc == 1 and "block_width" in msg


def test_raster_rejects_bad_zero_buffers(lib):
    cam = _cam()
    buf = ctypes.addressof((ctypes.c_float * 4)())  # (compared and null-checked only: rejected before any launch)
    rc, msg = _status(lib, "gstex_raster_bwd", ctypes.byref(_bwd_args(cam, v_texture=buf, zero_buf=buf,
                                                                      zero_floats=4)), None)
    assert rc == 1 and "zero_buf" in msg and "must not be the gradient accumulated" in msg
    rc, msg = _status(lib, "gstex_raster_bwd", ctypes.byref(_bwd_args(cam, zero_buf=buf, zero_floats=-1)), None)
    assert rc == 1 and "invalid zero_buf / zero_floats" in msg
    for kw in (dict(zero_buf=buf, zero_floats=-1), dict(zero_buf2=buf, zero_floats2=-1), dict(zero_floats=4)):
        rc, msg = _status(lib, "gstex_raster_fwd", ctypes.byref(_fwd_args(cam, **kw)), None)
        assert rc == 1 and "invalid zero_buf / zero_floats" in msg, kw


def test_raster_aux_bytes(lib):
    # cull-bit words (ceil(I / 64) + n_tiles + 1) * 4 x 8 B, then per backward unit (4 per slot; ceil(I / 256) +
    # n_tiles + 1 slots) cost + order (4 B each), the order's scratch, slot tiles
    # (4 B per slot) and a checkpoint of (4 + C + 6) fields x 64 lanes per unit, each array 256-B aligned
    def al(x):
        return (x + 255) // 256 * 256

    for n_isect, n_tiles, c in [(0, 1, 3), (1_915_389, 2500, 3), (12345, 77, 6)]:
        slots = (n_isect + 255) // 256 + n_tiles + 1
        expect = (al(((n_isect + 63) // 64 + n_tiles + 1) * 32) + 2 * al(slots * 16) + al(lib.gstex_unit_order_scratch_words() * 4) + al(slots * 4)
                  + al(slots * 4 * (4 + c + 6) * 64 * 4))
        assert lib.gstex_raster_aux_bytes(n_isect, n_tiles, c) == expect
    assert lib.gstex_raster_aux_bytes(-1, 1, 3) == 0 and lib.gstex_raster_aux_bytes(1, 1, 9) == 0


def test_sh_rejects_degree(lib):
    rc, msg = _status(lib, "gstex_sh_fwd", 4, 5, 36, None, None, None, None)
    assert rc == 1 and "degree" in msg
    rc, msg = _status(lib, "gstex_sh_fwd", 4, 3, 9, None, None, None, None)
    assert rc == 1 and "coefficients" in msg


def test_empty_inputs_are_noops(lib):
    cam = _cam()
    # n == 0 returns before touching the device
    assert lib.gstex_project_points(0, None, ctypes.byref(cam), None, None, None) == 0
    assert lib.gstex_aabb_2d(0, None, None, 1.0, None, ctypes.byref(cam), None, None, None) == 0
    assert lib.gstex_num_tiles_hit(0, None, None, 32, 32, 16, None, None) == 0
    assert lib.gstex_sh_fwd(0, 3, 16, None, None, None, None) == 0
    assert lib.gstex_texture_sample(0, 3, None, None, 0, None, None, None) == 0


def test_null_pointer_is_an_error(lib):
    cam = _cam()
    rc, msg = _status(lib, "gstex_project_points", 5, None, ctypes.byref(cam), None, None, None)
    assert rc == 1 and "null" in msg


def test_python_wrappers_refuse_cpu_tensors():
    import torch

    from gstex_amd import ops

    with pytest.raises(RuntimeError, match="HIP"):
        ops.project_points(torch.zeros(4, 3), torch.eye(4)[:3], (1.0, 1.0, 0.0, 0.0))


def test_adam_rejects_bad_tables(lib):
    from gstex_amd import _lib

    plain = (0, 1.0, None, None)  # flags, grad_scale, skip, stream
    rc, msg = _status(lib, "gstex_adam_step", 17, None, 0.9, 0.999, 1e-15, *plain)
    assert rc == 1 and "n_tensors" in msg
    t = (_lib.GstexAdamTensor * 1)(_lib.GstexAdamTensor(None, None, None, None, 10, 1e-3, 1.0))
    rc, msg = _status(lib, "gstex_adam_step", 1, t, 0.9, 0.999, 1e-15, *plain)
    assert rc == 1 and "null pointer" in msg
    t = (_lib.GstexAdamTensor * 1)(_lib.GstexAdamTensor(None, None, None, None, 0, 1e-3, 1.0))
    assert _status(lib, "gstex_adam_step", 1, t, 0.9, 0.999, 1e-15, *plain)[0] == 0  # empty: no launch
    rc, msg = _status(lib, "gstex_adam_step", 1, t, 0.9, 0.999, 1e-15, 1 << 1, 1.0, None, None)
    assert rc == 1 and "unknown flags" in msg
    for scale in (0.0, 1.5, float("nan")):
        rc, msg = _status(lib, "gstex_adam_step", 1, t, 0.9, 0.999, 1e-15, 0, scale, None, None)
        assert rc == 1 and "grad_scale must be in (0, 1]" in msg, scale


def test_loss_rejects_small_images_and_channels(lib):
    assert lib.gstex_loss_workspace_size(10, 64) == 0
    assert lib.gstex_loss_workspace_size(64, 64) > 9 * 54 * 54 * 4
    win = (ctypes.c_float * 11)()
    rc, msg = _status(lib, "gstex_loss_fwd", 8, 64, 3, None, None, None, None, None, win, 0.2, None, None, None, 0,
                      None)
    assert rc == 1 and "window" in msg
    rc, msg = _status(lib, "gstex_loss_bwd", 64, 64, 2, None, None, None, None, None, win, 0.2, None, None, None,
                      None, None, 0, None)
    assert rc == 1 and "channels" in msg


def test_activate_and_sh_rest_reject_bad_args(lib):
    rc, msg = _status(lib, "gstex_activate_fwd", 10, None, None, None, None, None, 1, None, None, None, None, None,
                      None, None, None, None)
    assert rc == 1 and "mappings_stride" in msg
    rc, msg = _status(lib, "gstex_activate_fwd", 10, None, None, None, None, None, 2, None, None, None, None, None,
                      None, None, None, None)
    assert rc == 1 and "null pointer" in msg
    rc, msg = _status(lib, "gstex_sh_rest_fwd", 4, 5, 35, None, None, None, None)
    assert rc == 1 and "degree" in msg
    rc, msg = _status(lib, "gstex_sh_rest_fwd", 4, 3, 14, None, None, None, None)
    assert rc == 1 and "coefficients" in msg
    assert lib.gstex_activate_fwd(0, None, None, None, None, None, 2, None, None, None, None, None, None, None, None,
                                  None) == 0


def test_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors in gstex_amd/_lib.py have the header's sizes and field offsets (gcc on the header)."""
    import subprocess

    structs = {"gstex_camera": _lib.GstexCamera, "gstex_pair_guard": _lib.GstexPairGuard,
               "gstex_adam_tensor": _lib.GstexAdamTensor,
               "gstex_train_prologue_args": _lib.GstexTrainPrologueArgs,
               "gstex_train_epilogue_args": _lib.GstexTrainEpilogueArgs,
               "gstex_raster_scene": _lib.GstexRasterScene, "gstex_raster_fwd_args": _lib.GstexRasterFwdArgs,
               "gstex_raster_bwd_args": _lib.GstexRasterBwdArgs,
               "gstex_raster_setup_bwd_args": _lib.GstexRasterSetupBwdArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[f"{cname} size"]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got[f"{cname} {f[0]}"]) == getattr(cls, f[0]).offset, f"{cname}.{f[0]}"


def test_train_prologue_scan_bytes(lib):
    for n in (0, 1, 127, 128, 1025, 200_000):
        b = lib.gstex_train_prologue_scan_bytes(n)
        assert b >= lib.gstex_scan_workspace_size(n) and b >= 4 * ((n + 255) // 256)  # one word per 256-splat block


def test_train_prologue_rejects_null_args(lib):
    rc, msg = _status(lib, "gstex_train_prologue", None, None)
    assert rc != 0 and "null" in msg
    rc, msg = _status(lib, "gstex_train_epilogue", None, None)
    assert rc != 0 and "invalid" in msg


# ---- the four tile-walking raster entry points' argument checks ------------------------------------------------------
_BUF = (ctypes.c_float * 8)()  # stands for every required device pointer: null-checked only, never read before a launch


def _raster_entry_call(lib, entry, H=32, block=16, channels=3, settings=0, n_texels=0, n_isect=0, null=()):
    """One call of `entry` whose arguments are valid except for the given faults (`null`: required pointers passed
    as NULL).  Every case of the table below has a fault, so the call returns before any HIP call."""
    p = ctypes.addressof(_BUF)
    cam = _cam(H=H, block=block)

    def ptrs(*names):
        return {n: (None if n in null else p) for n in names}

    if entry in ("gstex_raster_fwd", "gstex_raster_bwd"):
        scene = _lib.GstexRasterScene(cam=cam, channels=channels, settings=settings, tex_scale=1.0, n_texels=n_texels,
                                      n_isect=n_isect, **ptrs("records", "tile_ranges", "sorted_ids", "texture", "state", "aux"))
        if entry == "gstex_raster_fwd":
            args = _lib.GstexRasterFwdArgs(scene=scene, **ptrs("out_img", "out_alpha", "out_tex"))
        else:
            args = _lib.GstexRasterBwdArgs(scene=scene, **ptrs("sorted_slots", "v_img", "v_alpha", "v_tex",
                                                               "partials", "v_texture"))
        return _status(lib, entry, ctypes.byref(args), None)
    if entry == "gstex_texture_edit":
        q = ptrs("records", "tile_ranges", "sorted_ids", "edit_rgb", "edit_alpha", "depth_lo", "depth_hi", "out")
        return _status(lib, entry, ctypes.byref(cam), settings, q["records"], q["tile_ranges"], None,
                       q["sorted_ids"], q["edit_rgb"], q["edit_alpha"], q["depth_lo"], q["depth_hi"], n_texels,
                       q["out"], None)
    assert entry == "gstex_paint_scatter"
    args = _lib.GstexPaintScatterArgs(cam=cam, settings=settings, stroke_dtype=_lib.GT_F32, eps=0.01,
                                      n_texels=n_texels,
                                      **ptrs("records", "tile_ranges", "sorted_ids", "stroke", "depth", "acc"))
    return _status(lib, entry, ctypes.byref(args), None)


_FWD, _BWD, _EDIT, _PAINT = "gstex_raster_fwd", "gstex_raster_bwd", "gstex_texture_edit", "gstex_paint_scatter"
_REQUIRED = {_FWD: "out_img", _BWD: "aux", _EDIT: "edit_rgb", _PAINT: "depth"}  # the pointer the null cases drop
_GAUSS_SETTINGS = "texture_gaussians: unsupported settings bits 0x%x (supported: 1<<9, 1<<10, 1<<15)"
# (entry point, faults, status, message): status and message as the library gave them before the entry checks were
# shared (the message must still contain that text).  The cases from `block=8, channels=9` on break two rules each and
# pin which one is reported: every entry point keeps its own order of checks.
_RASTER_REJECTIONS = [
    (_FWD, dict(H=0), 1, "gstex_raster_fwd: invalid camera"),
    (_BWD, dict(H=0), 1, "gstex_raster_bwd: invalid camera"),
    (_EDIT, dict(H=0), 1, "gstex_texture_edit: invalid camera"),
    (_PAINT, dict(H=0), 1, "gstex_paint_scatter: invalid camera"),
    (_FWD, dict(block=8), 1, "gstex_raster_fwd: block_width must be 16 (got 8)"),
    (_BWD, dict(block=8), 1, "gstex_raster_bwd: block_width must be 16"),
    (_EDIT, dict(block=8), 1, "gstex_texture_edit: block_width must be 16 (got 8)"),
    (_PAINT, dict(block=8), 1, "gstex_paint_scatter: block_width must be 16 (got 8)"),
    (_FWD, dict(channels=0), 1, "gstex_raster_fwd: channels must be in [1, 8] (got 0)"),
    (_FWD, dict(channels=9), 1, "gstex_raster_fwd: channels must be in [1, 8] (got 9)"),
    (_BWD, dict(channels=0), 1, "gstex_raster_bwd: channels must be in [1, 8]"),
    (_BWD, dict(channels=9), 1, "gstex_raster_bwd: channels must be in [1, 8]"),
    (_FWD, dict(settings=1 << 2), 3, _GAUSS_SETTINGS % 4),
    (_BWD, dict(settings=1 << 2), 3, _GAUSS_SETTINGS % 4),
    (_EDIT, dict(settings=1 << 2), 3, "texture_edit: unsupported settings bits 0x4"),
    (_PAINT, dict(settings=1 << 2), 3, "gstex_paint_scatter: unsupported settings bits 0x4"),
    # bit 13 (GSTEX_SETTING_EDIT): the renders reject it; edit and paint accept it and go on to the pointer check
    (_FWD, dict(settings=1 << 13), 3, _GAUSS_SETTINGS % 0x2000),
    (_BWD, dict(settings=1 << 13), 3, _GAUSS_SETTINGS % 0x2000),
    (_EDIT, dict(settings=1 << 13, null=("tile_ranges",)), 1, "gstex_texture_edit: null pointer"),
    (_PAINT, dict(settings=1 << 13, null=("tile_ranges",)), 1, "gstex_paint_scatter: null pointer"),
    (_FWD, dict(n_texels=-1), 1, "gstex_raster_fwd: n_texels out of range"),
    (_BWD, dict(n_texels=-1), 1, "gstex_raster_bwd: n_texels out of range"),
    (_EDIT, dict(n_texels=-1), 1, "gstex_texture_edit: n_texels < 0"),
    (_PAINT, dict(n_texels=-1), 1, "gstex_paint_scatter: n_texels out of range (-1)"),
    (_FWD, dict(n_isect=-1), 1, "gstex_raster_fwd: n_isect out of range"),
    (_BWD, dict(n_isect=-1), 1, "gstex_raster_bwd: n_isect out of range"),
    (_FWD, dict(null=(_REQUIRED[_FWD],)), 1, "gstex_raster_fwd: null pointer"),
    (_BWD, dict(null=(_REQUIRED[_BWD],)), 1, "gstex_raster_bwd: null pointer (tile_ranges, state and the forward's aux)"),
    (_EDIT, dict(null=(_REQUIRED[_EDIT],)), 1, "gstex_texture_edit: null pointer"),
    (_PAINT, dict(null=(_REQUIRED[_PAINT],)), 1, "gstex_paint_scatter: null pointer"),
    (_FWD, dict(block=8, channels=9), 1, "gstex_raster_fwd: block_width must be 16 (got 8)"),
    (_BWD, dict(block=8, channels=9), 1, "gstex_raster_bwd: block_width must be 16"),
    (_FWD, dict(settings=1 << 2, null=(_REQUIRED[_FWD],)), 3, _GAUSS_SETTINGS % 4),
    (_BWD, dict(settings=1 << 2, null=(_REQUIRED[_BWD],)), 3, _GAUSS_SETTINGS % 4),
    (_EDIT, dict(settings=1 << 2, null=(_REQUIRED[_EDIT],)), 3, "texture_edit: unsupported settings bits 0x4"),
    (_PAINT, dict(settings=1 << 2, null=(_REQUIRED[_PAINT],)), 3, "gstex_paint_scatter: unsupported settings bits 0x4"),
    # the settings against the ranges: only the forward checks n_texels (and its texture) ahead of the settings
    (_FWD, dict(settings=1 << 2, n_texels=-1), 1, "gstex_raster_fwd: n_texels out of range"),
    (_BWD, dict(settings=1 << 2, n_texels=-1), 3, _GAUSS_SETTINGS % 4),
    (_EDIT, dict(settings=1 << 2, n_texels=-1), 3, "texture_edit: unsupported settings bits 0x4"),
    (_PAINT, dict(settings=1 << 2, n_texels=-1), 3, "gstex_paint_scatter: unsupported settings bits 0x4"),
    (_FWD, dict(settings=1 << 2, n_isect=-1), 3, _GAUSS_SETTINGS % 4),
    (_BWD, dict(settings=1 << 2, n_isect=-1), 3, _GAUSS_SETTINGS % 4),
    (_FWD, dict(settings=1 << 2, n_texels=1, null=("texture",)), 1, "gstex_raster_fwd: null texture"),
    (_BWD, dict(settings=1 << 2, n_texels=1, null=("texture",)), 3, _GAUSS_SETTINGS % 4),
    # the required pointers come before n_isect; the channels before n_texels; n_texels and n_isect either way round
    (_FWD, dict(n_isect=-1, null=(_REQUIRED[_FWD],)), 1, "gstex_raster_fwd: null pointer"),
    (_BWD, dict(n_isect=-1, null=(_REQUIRED[_BWD],)), 1, "gstex_raster_bwd: null pointer (tile_ranges, state and the forward's aux)"),
    (_FWD, dict(channels=9, n_texels=-1), 1, "gstex_raster_fwd: channels must be in [1, 8] (got 9)"),
    (_BWD, dict(channels=9, n_texels=-1), 1, "gstex_raster_bwd: channels must be in [1, 8]"),
    (_FWD, dict(n_texels=-1, n_isect=-1), 1, "gstex_raster_fwd: n_texels out of range"),
    (_BWD, dict(n_texels=-1, n_isect=-1), 1, "gstex_raster_bwd: n_isect out of range"),
    (_BWD, dict(n_texels=1, null=("v_texture",)), 1, "gstex_raster_bwd: null texture"),
    # gstex_texture_edit puts no upper bound on n_texels: the call goes on to its pointer check
    (_EDIT, dict(n_texels=2**31 - 1, null=("tile_ranges",)), 1, "gstex_texture_edit: null pointer"),
]


def test_raster_entry_rejections(lib):
    for entry, faults, status, text in _RASTER_REJECTIONS:
        rc, msg = _raster_entry_call(lib, entry, **faults)
        assert rc == status and text in msg, (entry, faults, rc, msg)
