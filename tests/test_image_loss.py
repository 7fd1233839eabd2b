"""The dataset-target loss without a GPU: the C ABI additions (gstex_loss_target_*) are declared, exported, bound and
reject invalid arguments before any launch; image_loss refuses bad inputs in Python; image_loss_eager gives its known
answers on the CPU; the Blender-format loader builds the trainer's cameras and the reference's uint8 images."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gstex_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gstex_hip.h")
NEW = ("gstex_loss_target_workspace_size", "gstex_loss_target_fwd", "gstex_loss_target_bwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------- C ABI
def test_new_symbols_declared_exported_and_bound(lib):
    import re

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} is not declared in gstex_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert lib.gstex_abi_version() == _lib.ABI_VERSION == 19  # additive: the number counts incompatible changes


def test_target_workspace_size(lib):
    assert lib.gstex_loss_target_workspace_size(10, 64) == 0 and lib.gstex_loss_target_workspace_size(64, 10) == 0
    assert lib.gstex_loss_target_workspace_size(64, 64) >= lib.gstex_loss_workspace_size(64, 64) > 0
    # three floats per forward workgroup (4 x 4 tiles x 3 channels), 256-B aligned, then the 9 gmap planes
    assert lib.gstex_loss_target_workspace_size(64, 64) == 768 + 9 * 54 * 54 * 4


def _target(**kw):
    fake = ctypes.addressof(_BUF)
    base = dict(gt=fake, mask=None, gt_dtype=_lib.GT_U8, gt_channels=4, mask_dtype=_lib.MASK_F32, reserved=0)
    base.update(kw)
    return _lib.GstexLossTarget(**base)


# host memory standing in for device pointers: compared with NULL and checked for alignment only, every call below is
# rejected before any launch
_BUF = (ctypes.c_float * 8)()


def _fwd(lib, target, H=64, W=64, C=3, ptrs=None, terms=None, ws=None, ws_bytes=0):
    win = (ctypes.c_float * 11)()
    rc = lib.gstex_loss_target_fwd(H, W, C, ptrs, ptrs, ptrs, ptrs, ctypes.byref(target) if target else None, win,
                                   0.2, None, None, terms, ws, ws_bytes, None)
    return rc, _lib.last_error()


def _bwd(lib, target, H=64, W=64, C=3, ptrs=None, ws=None, ws_bytes=0):
    win = (ctypes.c_float * 11)()
    rc = lib.gstex_loss_target_bwd(H, W, C, ptrs, ptrs, ptrs, ptrs, ctypes.byref(target) if target else None, win,
                                   0.2, ptrs, ptrs, ptrs, ptrs, ws, ws_bytes, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_target_entry_points_reject_invalid_arguments(lib, call):
    fake = ctypes.addressof(_BUF)
    cases = [
        (dict(target=None), "null target"),
        (dict(target=_target(gt=None)), "null target gt"),
        (dict(target=_target(gt_dtype=2)), "gt_dtype"),
        (dict(target=_target(gt_dtype=-1)), "gt_dtype"),
        (dict(target=_target(mask=fake, mask_dtype=2)), "mask_dtype"),
        (dict(target=_target(reserved=1)), "reserved"),
        (dict(target=_target(gt_channels=5)), "gt_channels"),
        (dict(target=_target(gt_channels=2)), "gt_channels"),
        (dict(target=_target(gt=fake + 2)), "aligned"),  # an RGBA uint8 pixel is one 32-bit load
        (dict(target=_target(), H=10), "window"),
        (dict(target=_target(), W=8), "window"),
        (dict(target=_target(), C=2), "channels"),
        (dict(target=_target(), C=9), "channels"),
        (dict(target=_target()), "null pointer"),  # null images / outputs
        (dict(target=_target(), ptrs=fake, ws=fake, ws_bytes=lib.gstex_loss_target_workspace_size(64, 64) - 1),
         "workspace too small"),
        (dict(target=_target(), ptrs=fake, ws=None, ws_bytes=1 << 20), "workspace too small"),
    ]
    for kw, word in cases:
        kw = dict(kw)
        if call is _fwd and kw.get("ptrs"):
            kw["terms"] = fake
        rc, msg = call(lib, kw.pop("target"), **kw)
        assert rc == 1 and word in msg and msg.startswith(f"gstex_loss_target_{call.__name__[1:]}"), (kw, rc, msg)
    if call is _fwd:  # the forward's own output: images given, terms_out null
        rc, msg = _fwd(lib, _target(), ptrs=fake, terms=None, ws=fake, ws_bytes=1 << 20)
        assert rc == 1 and "null pointer" in msg


def test_target_struct_layout_matches_header(tmp_path):
    """The ctypes mirror has the header's size and field offsets (gcc on the header), and the enums their values."""
    cls, cname = _lib.GstexLossTarget, "gstex_loss_target"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gstex_hip.h"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({cname}));',
             'printf("enums %d %d %d %d\\n", GSTEX_GT_F32, GSTEX_GT_U8, GSTEX_MASK_F32, GSTEX_MASK_BOOL);']
    for f in cls._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
    assert got["enums"].split() == [str(v) for v in (_lib.GT_F32, _lib.GT_U8, _lib.MASK_F32, _lib.MASK_BOOL)]


# ---------------------------------------------------------------- image_loss refusals (no device is touched)
def _raster_outputs(H=16, W=20, C=3):
    g = torch.Generator().manual_seed(0)
    return (torch.rand(H, W, 3, generator=g), torch.rand(H, W, C, generator=g), torch.rand(H, W, generator=g),
            torch.rand(3, generator=g))


def test_image_loss_refuses_bad_inputs():
    from gstex_amd.loss import image_loss

    H, W = 16, 20
    img, tex, alpha, bg = _raster_outputs(H, W)
    u8 = torch.zeros(H, W, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        image_loss(img, tex, alpha, bg, u8)  # CPU tensors
    with pytest.raises(ValueError, match="float32 or uint8"):
        image_loss(img, tex, alpha, bg, torch.zeros(H, W, 3, dtype=torch.int16))
    with pytest.raises(ValueError, match="image must have shape"):
        image_loss(img, tex, alpha, bg, torch.zeros(H, W, 5))
    with pytest.raises(ValueError, match="image must have shape"):
        image_loss(img, tex, alpha, bg, torch.zeros(H, W + 1, 3))
    with pytest.raises(ValueError, match="uint8 mask is ambiguous"):
        image_loss(img, tex, alpha, bg, u8, mask=torch.ones(H, W, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask must be bool or float32"):
        image_loss(img, tex, alpha, bg, u8, mask=torch.ones(H, W, dtype=torch.float64))
    for shape in ((H, W, 3), (W, H), (H * W,)):
        with pytest.raises(ValueError, match="mask must have shape"):
            image_loss(img, tex, alpha, bg, u8, mask=torch.ones(shape, dtype=torch.bool))
    img, tex, alpha, bg = _raster_outputs(10, W)
    with pytest.raises(ValueError, match="larger than the 11-tap"):
        image_loss(img, tex, alpha, bg, torch.zeros(10, W, 3, dtype=torch.uint8))


# ---------------------------------------------------------------- image_loss_eager known answers (CPU)
def _eager_case(H=23, W=31, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(H, W, 3, generator=g)
    bg = torch.rand(3, generator=g)
    rgba = torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8)
    return rgb, bg, rgba


def test_eager_all_false_mask_gives_zero_loss_and_plain_mse():
    from gstex_amd.loss import image_loss_eager

    rgb, bg, rgba = _eager_case()
    res = image_loss_eager(rgb, bg, rgba, mask=torch.zeros(23, 31, dtype=torch.bool))
    assert float(res.loss) == 0.0 and float(res.terms[0]) == 0.0  # L1 = 0 and the SSIM of two zero images is 1
    assert float(res.terms[1]) == 0.0 and float(res.terms[2]) == 1.0
    assert torch.equal(res.terms[3], ((rgb - res.gt) ** 2).mean())  # the MSE is unmasked
    assert float(res.terms[3]) > 0.0


def test_eager_transparent_rgba_is_the_background():
    from gstex_amd.loss import image_loss_eager

    rgb, bg, rgba = _eager_case()
    rgba[..., 3] = 0
    res = image_loss_eager(rgb, bg, rgba)
    assert torch.equal(res.gt, bg[None, None, :].expand(23, 31, 3))


def test_eager_uint8_is_divided_by_255():
    from gstex_amd.loss import image_loss_eager

    rgb, bg, rgba = _eager_case()
    image = rgba[..., :3].contiguous()
    image.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)  # every byte value
    res = image_loss_eager(rgb, bg, image)
    assert torch.equal(res.gt, image.float() / 255.0)


def test_eager_all_true_mask_equals_no_mask():
    from gstex_amd.loss import image_loss_eager

    rgb, bg, rgba = _eager_case()
    plain = image_loss_eager(rgb, bg, rgba)
    for mask in (torch.ones(23, 31, dtype=torch.bool), torch.ones(23, 31, 1)):
        res = image_loss_eager(rgb, bg, rgba, mask=mask)
        assert torch.equal(res.terms, plain.terms) and torch.equal(res.gt, plain.gt)
    assert float(plain.terms[0]) == pytest.approx(0.8 * float(plain.terms[1]) + 0.2 * (1 - float(plain.terms[2])),
                                                  abs=1e-6)


def test_eager_loss_is_differentiable_in_rgb_only_where_unmasked():
    from gstex_amd.loss import image_loss_eager

    rgb, bg, rgba = _eager_case()
    mask = torch.ones(23, 31, dtype=torch.bool)
    mask[:12] = False
    leaf = rgb.clone().requires_grad_(True)
    image_loss_eager(leaf, bg, rgba, mask=mask).loss.backward()
    assert float(leaf.grad[:12].abs().max()) == 0.0 and float(leaf.grad[12:].abs().max()) > 0.0


# ---------------------------------------------------------------- Blender-format loader
def _write_scene(root, n=3, H=12, W=16, angle=0.6911112):
    from PIL import Image

    from gstex_amd.scene import look_at

    g = np.random.default_rng(5)
    frames = []
    for i in range(n):
        px = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
        px[0, 0] = (100, 100, 100, 128)
        px[0, 1] = (7, 200, 31, 0)
        px[0, 2] = (7, 200, 31, 255)
        Image.fromarray(px, "RGBA").save(os.path.join(root, f"r_{i}.png"))
        # an OpenGL camera-to-world looking at the origin (undo look_at's y/z flip)
        pos = (3.0 * math.cos(0.7 * i), 3.0 * math.sin(0.7 * i), 1.0 + 0.5 * i)
        c2w_cv = look_at(pos)[1].double().numpy()
        c2w_gl = c2w_cv.copy()
        c2w_gl[:3, :3] = c2w_cv[:3, :3] @ np.diag([1.0, -1.0, -1.0])
        frames.append({"file_path": f"./r_{i}", "transform_matrix": c2w_gl.tolist()})
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": angle, "frames": frames}, f)
    return frames


def test_load_blender(tmp_path):
    from gstex_amd.data import load_blender
    from gstex_amd.scene import look_at

    H, W, angle = 12, 16, 0.6911112
    frames = _write_scene(str(tmp_path), 3, H, W, angle)
    white = load_blender(str(tmp_path), "train", alpha_color="white")
    rgba = load_blender(str(tmp_path), "train", alpha_color=None)
    assert len(white) == len(rgba) == 3
    for i, ((view, image), (view4, image4)) in enumerate(zip(white, rgba)):
        assert (view.H, view.W) == (H, W)
        assert view.fx == view.fy == pytest.approx(0.5 * W / math.tan(0.5 * angle), rel=1e-7)
        assert view.cx == W / 2 and view.cy == H / 2
        vm4 = torch.cat([view.viewmat, torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
        assert tuple(view.viewmat.shape) == (3, 4) and tuple(view.c2w.shape) == (4, 4)
        assert float((view.c2w - torch.linalg.inv(vm4.double()).float()).abs().max()) <= 1e-6
        campos = torch.tensor(frames[i]["transform_matrix"], dtype=torch.float64)[:3, 3]
        at_origin = view.viewmat.double() @ torch.cat([campos, torch.ones(1, dtype=torch.float64)])
        assert float(at_origin.abs().max()) <= 1e-6  # the camera centre maps to the view-space origin
        # the same matrices scene.look_at builds for this camera position
        vm_ref, c2w_ref = look_at(campos.numpy())
        assert float((view.viewmat - vm_ref).abs().max()) <= 1e-6 and float((view.c2w - c2w_ref).abs().max()) <= 1e-6
        assert torch.equal(view4.viewmat, view.viewmat) and view4.fx == view.fx
        assert image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3) and not image.is_cuda
        assert image4.dtype == torch.uint8 and tuple(image4.shape) == (H, W, 4)
        # 100 * 128/255 + 255 * (1 - 128/255) = 177.196..., truncated
        assert image[0, 0].tolist() == [177, 177, 177]
        assert image4[0, 0].tolist() == [100, 100, 100, 128]
        assert image[0, 1].tolist() == [255, 255, 255] and image[0, 2].tolist() == [7, 200, 31]
    black = load_blender(str(tmp_path), "train", alpha_color="black")
    assert black[0][1][0, 0].tolist() == [50, 50, 50]  # 100 * 128/255 = 50.196...
    with pytest.raises(ValueError, match="alpha_color"):
        load_blender(str(tmp_path), "train", alpha_color="grey")
