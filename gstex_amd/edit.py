"""The edit list of the reference's viewer paint tool, in its on-disk format.

The reference keeps one entry per stroke session -- the drawing camera as ``Cameras.to_json`` writes it, the canvas (a
uint8 RGBA image the polylines are drawn into) and the canvas's file name (gstex.py:451-464) -- saves the list as
``info.json`` plus one PNG per canvas (``handle_save``, gstex.py:404-419) and reads it back at start-up
(``import_edit_json``, gstex.py:364-375).  ``load_edits`` / ``save_edits`` read and write that format;
``GStexTrainer.edit_texture`` / ``bake_edits`` replay a list (``update_edit_texture``, gstex.py:427-437).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass

import numpy as np
import torch

from .data import view_from_c2w
from .scene import View


@dataclass
class Edit:
    view: View            # the drawing camera, in the trainer's conventions
    canvas: torch.Tensor  # uint8 (H, W, 4): the stroke, straight alpha
    file: str             # the canvas's PNG, as info.json names it


def view_from_camera_json(d: dict, H: int, W: int) -> View:
    """The View of a camera dict written by Cameras.to_json (cameras/cameras.py:964-973): camera_to_world 3x4 (or 4x4)
    in OpenGL axes, fx, fy, cx, cy.  The dict carries no image size: H and W come from the canvas, as in
    draw_from_view's caller (gstex.py:432-435)."""
    c2w = np.asarray(d["camera_to_world"], np.float64).reshape(-1, 4)
    return view_from_c2w(c2w, d["fx"], d["fy"], d["cx"], d["cy"], H, W)


def camera_json_from_view(view: View) -> dict:
    """to_json's dict for a View: the inverse of view_from_camera_json.  The rotation is the viewmat's transpose with
    the y/z flip undone (exact: a transpose and two sign changes), the position is c2w's: a View made from a float32
    pose -- any pose the reference wrote -- gives that pose back bit for bit, so save -> load reproduces the View."""
    vm = view.viewmat.detach().cpu().numpy().astype(np.float64)
    c2w = view.c2w.detach().cpu().numpy().astype(np.float64)
    gl = np.concatenate([vm[:3, :3].T @ np.diag([1.0, -1.0, -1.0]), c2w[:3, 3:4]], axis=1)
    return {"type": "PinholeCamera", "cx": float(view.cx), "cy": float(view.cy), "fx": float(view.fx),
            "fy": float(view.fy), "camera_to_world": gl.tolist(), "camera_index": 0, "times": None}


def _canvas(path: str) -> torch.Tensor:
    from PIL import Image  # (lazily, as gstex_amd.data)

    image = np.array(Image.open(path), dtype="uint8")
    if image.ndim != 3 or image.shape[2] != 4:
        raise ValueError(f"load_edits: {path} has shape {image.shape}; a canvas is (H, W, 4) RGBA")
    return torch.from_numpy(image)


def load_edits(info_json: str) -> list:
    """[Edit] of an info.json: a list of {"camera", "file"}.  A relative file name that does not exist as given is
    looked up beside info.json."""
    with open(info_json) as f:
        entries = json.load(f)
    edits = []
    for e in entries:
        path = e["file"]
        if not os.path.isabs(path) and not os.path.exists(path):
            path = os.path.join(os.path.dirname(os.path.abspath(info_json)), path)
        canvas = _canvas(path)
        edits.append(Edit(view_from_camera_json(e["camera"], int(canvas.shape[0]), int(canvas.shape[1])), canvas,
                          e["file"]))
    return edits


def save_edits(directory: str, edits) -> str:
    """handle_save: every canvas as a PNG under directory/images/ (its `file`'s base name) and directory/info.json
    naming them relative to the directory.  Returns the path of info.json."""
    from PIL import Image

    os.makedirs(os.path.join(directory, "images"), exist_ok=True)
    entries = []
    for i, e in enumerate(edits):
        canvas = torch.as_tensor(e.canvas).detach().cpu()
        if canvas.dtype != torch.uint8 or canvas.dim() != 3 or canvas.shape[2] != 4:
            raise ValueError(f"save_edits: canvas {i} must be uint8 (H, W, 4) "
                             f"(got {canvas.dtype} {tuple(canvas.shape)})")
        name = os.path.join("images", os.path.basename(e.file) or f"{i:06d}.png")
        Image.fromarray(canvas.numpy()).save(os.path.join(directory, name))
        entries.append({"camera": camera_json_from_view(e.view), "file": name})
    path = os.path.join(directory, "info.json")
    with open(path, "w") as f:
        json.dump(entries, f)
    return path
