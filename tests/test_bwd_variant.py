"""gstex_raster_bwd_variant: which build of the raster backward a call takes (a host-side query: no device).

The training build (GSTEX_BWD_TRAIN) is taken exactly when the call is the photometric training step's: 3 channels,
no depth / normal / enabled-distortion gradient, float-atomic accumulation (row_flags NULL), v_img / v_alpha / v_tex
given, and v_tex the SAME address as v_img.  Any one condition broken: the generic build."""
import ctypes

import pytest

from gstex_amd import _lib

# addresses only (the query dereferences nothing but the argument struct)
IMG, ALPHA, OTHER, DEPTH, FLAGS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _args(channels=3, settings=_lib.SETTING_AA_BLUR | _lib.SETTING_DIST_REG, **fields):
    scene = _lib.GstexRasterScene(channels=channels, settings=settings)
    base = dict(v_img=IMG, v_alpha=ALPHA, v_tex=IMG)
    base.update(fields)
    return _lib.GstexRasterBwdArgs(scene=scene, **base)


def _variant(a):
    return _lib.load().gstex_raster_bwd_variant(ctypes.byref(a))


def test_training_call_selects_train():
    assert _variant(_args()) == _lib.BWD_TRAIN
    # a distortion gradient with the distortion term switched off does not count (as in gstex_raster_bwd)
    assert _variant(_args(settings=_lib.SETTING_AA_BLUR, v_reg=OTHER)) == _lib.BWD_TRAIN


@pytest.mark.parametrize("name,broken", [
    ("six channels", dict(channels=6)),
    ("one channel", dict(channels=1)),
    ("deterministic rows", dict(row_flags=FLAGS)),
    ("depth gradient", dict(v_depth=DEPTH)),
    ("normal gradient", dict(v_normal=DEPTH)),
    ("distortion gradient, enabled", dict(v_reg=DEPTH)),
    ("v_tex a distinct address", dict(v_tex=OTHER)),
    ("v_tex NULL", dict(v_tex=None)),
    ("v_img and v_tex NULL", dict(v_img=None, v_tex=None)),
    ("v_alpha NULL", dict(v_alpha=None)),
])
def test_any_broken_condition_selects_generic(name, broken):
    assert _variant(_args(**broken)) == _lib.BWD_GENERIC, name


def test_null_args_and_abi():
    lib = _lib.load()
    assert lib.gstex_raster_bwd_variant(None) == -1
    assert lib.gstex_abi_version() == 19 == _lib.ABI_VERSION
