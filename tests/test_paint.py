"""Painting without a GPU: the C ABI additions (gstex_paint_scatter / gstex_paint_blend) are declared, exported, bound,
laid out as the header says and reject invalid arguments before any launch; paint_blend_eager gives its known answer
on the CPU; the edit list round-trips through the reference's on-disk format."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gstex_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gstex_hip.h")
NEW = ("gstex_paint_scatter", "gstex_paint_blend")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------- C ABI
def test_new_symbols_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} is not declared in gstex_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19  # additive: the number counts incompatible changes


def test_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors have the header's sizes and field offsets (gcc on the header)."""
    structs = {"gstex_paint_scatter_args": _lib.GstexPaintScatterArgs,
               "gstex_paint_blend_args": _lib.GstexPaintBlendArgs}
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


# host memory standing in for device pointers: compared with NULL and checked for alignment only, every call below is
# rejected before any launch
_BUF = (ctypes.c_float * 8)()


def _cam(H=32, W=32, block=16):
    return _lib.GstexCamera(None, None, 100.0, 100.0, 16.0, 16.0, H, W, block)


def _scatter(lib, **kw):
    fake = ctypes.addressof(_BUF)
    base = dict(cam=_cam(), settings=1 << 13, stroke_dtype=_lib.GT_F32, eps=1e-2, records=fake, tile_ranges=fake,
                tile_order=None, sorted_ids=fake, stroke=fake, depth=fake, n_texels=4, acc=fake)
    base.update(kw)
    rc = lib.gstex_paint_scatter(ctypes.byref(_lib.GstexPaintScatterArgs(**base)), None)
    return rc, _lib.last_error()


def _blend(lib, **kw):
    fake = ctypes.addressof(_BUF)
    base = dict(n_texels=4, acc=fake, texture=fake, scale=1.0, shift=0.0)
    base.update(kw)
    rc = lib.gstex_paint_blend(ctypes.byref(_lib.GstexPaintBlendArgs(**base)), None)
    return rc, _lib.last_error()


def test_scatter_rejects_invalid_arguments(lib):
    rc = lib.gstex_paint_scatter(None, None)
    assert rc == 1 and "null args" in _lib.last_error()
    fake = ctypes.addressof(_BUF)
    cases = [
        (dict(cam=_cam(block=8)), 1, "block_width must be 16"),
        (dict(cam=_cam(H=0)), 1, "invalid camera"),
        (dict(settings=(1 << 13) | (1 << 2)), 3, "unsupported settings"),
        (dict(n_texels=-1), 1, "n_texels"),
        (dict(n_texels=1 << 31), 1, "n_texels"),
        (dict(eps=-1e-3), 1, "eps"),
        (dict(eps=float("nan")), 1, "eps"),
        (dict(stroke_dtype=2), 1, "stroke_dtype"),
        (dict(stroke=None), 1, "null pointer"),
        (dict(depth=None), 1, "null pointer"),
        (dict(tile_ranges=None), 1, "null pointer"),
        (dict(acc=None), 1, "null pointer"),
        (dict(stroke=fake + 4), 1, "aligned"),  # an fp32 RGBA pixel is one 16-byte load
        (dict(stroke=fake + 2, stroke_dtype=_lib.GT_U8), 1, "aligned"),
    ]
    for kw, status, word in cases:
        rc, msg = _scatter(lib, **kw)
        assert rc == status and word in msg and msg.startswith("gstex_paint_scatter"), (kw, rc, msg)


def test_blend_rejects_invalid_arguments(lib):
    rc = lib.gstex_paint_blend(None, None)
    assert rc == 1 and "null args" in _lib.last_error()
    cases = [
        (dict(n_texels=-1), "n_texels"),
        (dict(n_texels=1 << 31), "n_texels"),
        (dict(scale=0.0), "scale"),
        (dict(scale=float("inf")), "scale"),
        (dict(shift=float("nan")), "scale"),
        (dict(acc=None), "null pointer"),
        (dict(texture=None), "null pointer"),
    ]
    for kw, word in cases:
        rc, msg = _blend(lib, **kw)
        assert rc == 1 and word in msg and msg.startswith("gstex_paint_blend"), (kw, rc, msg)
    assert _blend(lib, n_texels=0, acc=None, texture=None)[0] == 0  # no texels: no launch


def test_python_wrappers_refuse_bad_inputs():
    from gstex_amd import ops

    acc, tex = torch.zeros(4, 5), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.paint_blend(acc, tex, 4)
    with pytest.raises(RuntimeError, match="n_texels"):
        ops.paint_blend(acc, tex, -1)
    with pytest.raises(RuntimeError, match="transform"):
        ops.paint_blend(acc, tex, 4, transform=(0.0, 0.5))
    with pytest.raises(RuntimeError, match="eps"):
        ops.paint_scatter(acc, None, None, None, None, None, None, None, None, 1.0, 1.0, 0.0, 0.0, 16, 16, 4, eps=-1.0)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.paint_scatter(acc, None, None, None, None, None, None, None, None, 1.0, 1.0, 0.0, 0.0, 16, 16, 4)


# ---------------------------------------------------------------- the blend's torch twin
def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    from gstex_amd.ops import _fma32

    g = torch.Generator().manual_seed(0)
    a = torch.randn(20000, generator=g) * torch.exp(4 * torch.randn(20000, generator=g))
    b = torch.randn(20000, generator=g)
    c = -(a * b) + 1e-7 * torch.randn(20000, generator=g) * (a * b).abs()  # heavy cancellation: where fma differs
    got = _fma32(a, b, c).numpy()
    from fractions import Fraction

    an, bn, cn = a.numpy(), b.numpy(), c.numpy()
    for i in range(0, 20000, 97):  # exact rational arithmetic, rounded once
        exact = Fraction(float(an[i])) * Fraction(float(bn[i])) + Fraction(float(cn[i]))
        assert got[i] == _round_fraction_f32(exact), i


def _round_fraction_f32(x):
    """The fp32 nearest (ties to even) to a Fraction."""
    if x == 0:
        return np.float32(0.0)
    lo = np.float32(float(x))  # float(Fraction) is correctly rounded to fp64; its fp32 rounding is within one ulp
    cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
    from fractions import Fraction

    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def test_paint_blend_eager_known_answer():
    """test_oracle.py's facing-camera splat under a full-coverage opaque stroke of colour c: a == wt on every hit
    texel, so the blend weight is wt / (wt + 1e-6) and the texel moves from cur to c * a / (a + 1e-6) by exactly that
    weight; texels with a == 0 keep their bits."""
    from test_oracle import facing_camera_case

    from gstex_amd.ops import paint_blend_eager
    from oracle import raster as O

    inp = facing_camera_case([((0.0, 0.0, 2.0), 0.05, 0.8, (0.1, 0.2, 0.3)),
                              ((5.0, 0.0, 2.0), 0.05, 0.8, (0.1, 0.2, 0.3))],  # the second splat is off screen
                             tex_hw=(4, 4), settings=1 << 13)
    H, W = inp.cam.H, inp.cam.W
    c = torch.tensor([0.2, 0.4, 0.6])
    out = O.texture_edit(inp, c.expand(H, W, 3).clone(), torch.ones(H, W), torch.full((H, W), -1e9),
                         torch.full((H, W), 1e9))
    acc = out.float()
    hit = acc[:, 3] > 0
    assert int(hit.sum()) == 16 and not bool(hit[16:].any())
    assert torch.equal(acc[:, 3], acc[:, 4])  # opaque stroke: the same sums
    cur = inp.texture[:, :3].clone()
    res = paint_blend_eager(acc, cur)
    assert torch.equal(cur, inp.texture[:, :3]) and res.data_ptr() != cur.data_ptr()  # inputs untouched
    assert torch.equal(res[~hit], cur[~hit])  # a == 0: bits kept
    a64, wt64 = acc[hit, 3:4].double(), acc[hit, 4:5].double()
    weight = wt64 / (wt64 + np.float64(np.float32(1e-6)))
    colour = acc[hit, :3].double() / (a64 + np.float64(np.float32(1e-6)))
    expect = colour * weight + cur[hit].double() * (1 - weight)
    assert float((res[hit].double() - expect).abs().max()) <= 4 * 2.0 ** -24  # a few fp32 roundings of values <= 1
    # the move towards the stroke colour, as a fraction of the way: the weight
    moved = (res[hit].double() - cur[hit].double()) / (colour - cur[hit].double())
    assert float((moved - weight).abs().max()) <= 1e-5
    # the colour falls short of c by c * 1e-6 / (a + 1e-6) (plus the fp32 rounding of the sums), the weight of 1 by
    # 1e-6 / (wt + 1e-6): both small wherever the stroke put weight on the texel
    assert bool(((colour - c.double()).abs() <= c.double() * 1e-6 / a64 + 1e-6).all())
    assert bool(((1 - weight) <= 1e-6 / wt64 + 1e-12).all())
    # transform mode on the SH-DC store: the same edit in raster space, untouched texels bit-identical
    C0 = 0.28209479177387814
    dc = (cur - 0.5) / C0
    res_dc = paint_blend_eager(acc, dc, transform=(C0, 0.5))
    assert torch.equal(res_dc[~hit], dc[~hit])
    assert float((res_dc[hit] * C0 + 0.5 - res[hit]).abs().max()) <= 1e-6
    # rows past the accumulator's are passed through
    longer = torch.cat([cur, torch.full((3, 3), 7.0)])
    assert torch.equal(paint_blend_eager(acc, longer)[-3:], longer[-3:])


# ---------------------------------------------------------------- the edit list on disk
def _views():
    from gstex_amd.data import view_from_c2w

    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(2):
        q, _r = torch.linalg.qr(torch.randn(3, 3, generator=g))
        pose = torch.cat([q, torch.randn(3, 1, generator=g)], 1).float().numpy()  # a float32 pose, as to_json writes
        out.append((pose, view_from_c2w(pose, 111.5, 112.25, 20.0, 14.5, 28, 40)))
    return out


def _same_view(a, b):
    return (torch.equal(a.viewmat, b.viewmat) and torch.equal(a.c2w, b.c2w)
            and (a.fx, a.fy, a.cx, a.cy, a.H, a.W) == (b.fx, b.fy, b.cx, b.cy, b.H, b.W))


def test_view_from_camera_json_equals_view_from_c2w():
    from gstex_amd.edit import camera_json_from_view, view_from_camera_json

    for pose, view in _views():
        d = {"type": "PinholeCamera", "cx": 20.0, "cy": 14.5, "fx": 111.5, "fy": 112.25,
             "camera_to_world": pose.tolist(), "camera_index": 0, "times": None}
        assert _same_view(view_from_camera_json(d, 28, 40), view)
        back = camera_json_from_view(view)
        assert back["camera_to_world"] == d["camera_to_world"] and set(back) == set(d)


def test_save_edits_load_edits_round_trip(tmp_path):
    from gstex_amd.edit import Edit, load_edits, save_edits

    g = torch.Generator().manual_seed(6)
    edits = [Edit(view, torch.randint(0, 256, (28, 40, 4), generator=g, dtype=torch.uint8), f"stroke{i}.png")
             for i, (_, view) in enumerate(_views())]
    info = save_edits(str(tmp_path / "edit"), edits)
    assert os.path.basename(info) == "info.json"
    listed = json.load(open(info))
    assert [set(e) for e in listed] == [{"camera", "file"}] * 2
    back = load_edits(info)
    assert len(back) == 2
    for a, b in zip(edits, back):
        assert _same_view(a.view, b.view)
        assert b.canvas.dtype == torch.uint8 and torch.equal(a.canvas, b.canvas)
    again = load_edits(save_edits(str(tmp_path / "edit2"), back))
    assert all(_same_view(a.view, b.view) and torch.equal(a.canvas, b.canvas) for a, b in zip(back, again))


def test_load_edits_reads_a_hand_written_info_json(tmp_path):
    from PIL import Image

    from gstex_amd.edit import load_edits

    (pose, view), _ = _views()
    canvas = np.zeros((28, 40, 4), np.uint8)
    canvas[5:9, 3:30] = (255, 0, 0, 255)
    png = tmp_path / "images" / "2024-01-01_000000.png"
    png.parent.mkdir()
    Image.fromarray(canvas).save(png)
    info = tmp_path / "info.json"
    info.write_text(json.dumps([{"camera": {"type": "PinholeCamera", "cx": 20.0, "cy": 14.5, "fx": 111.5,
                                            "fy": 112.25, "camera_to_world": pose.tolist(), "camera_index": 0,
                                            "times": None}, "file": str(png)}]))
    (edit,) = load_edits(str(info))
    assert _same_view(edit.view, view) and edit.file == str(png)
    assert torch.equal(edit.canvas, torch.from_numpy(canvas))
