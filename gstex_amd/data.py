"""Blender-format (NeRF synthetic) dataset loader.

``load_blender(root, split, alpha_color)`` restates the reference's Blender data parser
(nerfstudio/data/dataparsers/blender_dataparser.py:65-105) and its uint8 image path
(data/datasets/base_dataset.py:95-110): ``transforms_{split}.json`` gives one horizontal field of view and a
camera-to-world matrix per frame, the images are ``file_path + ".png"``, RGBA.  The views come out in the trainer's
conventions (``scene.View``: the y/z flip of gstex.py:1031-1042), the images as uint8 CPU tensors -- what
``GStexTrainer.forward_backward`` takes after a ``.to(device)``.  No downscale schedule (num_downscales is 0 in every
preset) and no other dataset format.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from .scene import View


def view_from_c2w(c2w_gl, fx: float, fy: float, cx: float, cy: float, H: int, W: int) -> View:
    """A View from an OpenGL camera-to-world matrix (3x4 or 4x4), as get_outputs derives its matrices
    (gstex.py:1031-1042): flip y and z, invert analytically for the viewmat, invert that for c2w -- the construction
    of scene.look_at."""
    m = np.asarray(c2w_gl, np.float64)
    R = m[:3, :3] @ np.diag([1.0, -1.0, -1.0])
    vm = np.eye(4)
    vm[:3, :3] = R.T
    vm[:3, 3] = -R.T @ m[:3, 3]
    c2w = np.linalg.inv(vm)
    return View(torch.tensor(vm[:3, :], dtype=torch.float32), torch.tensor(c2w, dtype=torch.float32), float(fx),
                float(fy), float(cx), float(cy), int(H), int(W))


def _read_png(path: str) -> np.ndarray:
    from PIL import Image  # (only the loader needs Pillow)

    image = np.array(Image.open(path), dtype="uint8")
    if image.ndim == 2:  # greyscale: repeated over three channels (base_dataset.py:74-75)
        image = image[:, :, None].repeat(3, axis=2)
    if image.ndim != 3 or image.shape[2] not in (3, 4):
        raise ValueError(f"load_blender: {path} has shape {image.shape}; expected (H, W, 3) or (H, W, 4)")
    return image


def composite_uint8(image: torch.Tensor, alpha_color) -> torch.Tensor:
    """An RGBA uint8 image on a fixed colour, in uint8, as get_image_uint8 does it (base_dataset.py:102-109): the sum
    is formed in float, clamped to [0, 255] and truncated."""
    color = torch.as_tensor(alpha_color, dtype=torch.float32)
    a = image[:, :, -1:] / 255.0
    out = image[:, :, :3] * a + 255.0 * color * (1.0 - a)
    return torch.clamp(out, min=0, max=255).to(torch.uint8)


ALPHA_COLORS = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}


def load_blender(root: str, split: str = "train", alpha_color="white"):
    """[(View, image)] of a Blender-format scene.  alpha_color: "white", "black" or an (r, g, b) in [0, 1] -- the
    images are pre-composited on it and have three channels -- or None: they keep their alpha channel, for a trainer
    with background="random" to composite on each step's colour."""
    with open(os.path.join(root, f"transforms_{split}.json")) as f:
        meta = json.load(f)
    if isinstance(alpha_color, str):
        if alpha_color not in ALPHA_COLORS:
            raise ValueError('load_blender: alpha_color must be "white", "black", a colour or None '
                             f"(got {alpha_color!r})")
        alpha_color = ALPHA_COLORS[alpha_color]
    angle = float(meta["camera_angle_x"])
    out = []
    for frame in meta["frames"]:
        path = os.path.join(root, frame["file_path"].replace("./", "") + ".png")
        image = torch.from_numpy(_read_png(path))
        H, W = int(image.shape[0]), int(image.shape[1])
        focal = 0.5 * W / math.tan(0.5 * angle)  # fx = fy (blender_dataparser.py:78, 90-91)
        pose = np.array(frame["transform_matrix"], dtype=np.float32)
        view = view_from_c2w(pose, focal, focal, W / 2.0, H / 2.0, H, W)
        if alpha_color is not None and image.shape[2] == 4:
            image = composite_uint8(image, alpha_color)
        out.append((view, image))
    return out
