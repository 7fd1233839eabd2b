"""Pin gstex_amd.pose against the REFERENCE's own pose-correction code.

Run in the build container only (reads the reference checkout, which the GPU box does not have):
    python tests/golden/make_pose_golden.py
Writes tests/golden/pose_golden.npz.  Like make_conventions_golden.py, functions are AST-extracted from the source text
and exec'd; only inputs and outputs (arrays) are committed.

1. exp_map_SO3xR3 / exp_map_SE3 (nerfstudio/cameras/lie_groups.py) on a dozen tangent vectors (translation, rotation),
   fp32 as the reference evaluates them: zero, a tiny rotation (below both functions' small-angle guards), pure
   translations, pure rotations, a rotation just above the guards, a large rotation, and seeded random ones.
2. The camera the reference renders for each: CameraOptimizer.apply_to_camera's product (camera_optimizers.py:154-162,
   camera_to_worlds @ [adj; 0 0 0 1], with poses.multiply's convention checked on the way) followed by the statements of
   GStexModel.get_outputs that flip y / z and invert (gstex.py:1031-1042), on the OpenGL camera_to_worlds of
   gstex_amd.scene.sphere_view(1, 64, 80).  Committed: the base View's post-flip viewmat / c2w (what PoseRefiner.view
   takes) and the reference's viewmat / c2w per tangent and mode.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF_ROOT = os.environ.get("GSTEX_REFERENCE", "/root/reference")
REF_LIE = os.path.join(REF_ROOT, "nerfstudio/cameras/lie_groups.py")
REF_POSES = os.path.join(REF_ROOT, "nerfstudio/utils/poses.py")
REF_MODEL = os.path.join(REF_ROOT, "nerfstudio/models/gstex.py")
OUT = os.path.join(HERE, "pose_golden.npz")


def extract_functions(path, names):
    src = open(path).read()
    tree = ast.parse(src)
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in found:
            node.returns = None  # (jaxtyping annotations are not importable here)
            for a in node.args.args:
                a.annotation = None
            found[node.name] = ast.unparse(node)
    assert set(found) == set(names), set(names) - set(found)
    return found


def extract_flip_inverse(path):
    """The statements of get_outputs from `R = camera.camera_to_worlds[...]` to `c2w = viewmat...inverse()`."""
    src = open(path).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "get_outputs")
    body = fn.body
    first = next(i for i, n in enumerate(body) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name)
                 and n.targets[0].id == "R" and "camera_to_worlds" in ast.get_source_segment(src, n))
    last = next(i for i, n in enumerate(body) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name)
                and n.targets[0].id == "c2w")
    assert first < last <= first + 12, (first, last)
    return "\n".join(ast.get_source_segment(src, n) for n in body[first:last + 1]), (body[first].lineno,
                                                                                      body[last].lineno)


def tangents():
    g = torch.Generator().manual_seed(7)
    rows = [
        [0, 0, 0, 0, 0, 0],
        [0, 0, 0, 1e-4, -2e-4, 5e-5],            # a tiny rotation (below both small-angle guards)
        [0.05, -0.02, 0.03, 0, 0, 0],            # a pure translation
        [-0.3, 0.1, 0.2, 0, 0, 0],
        [0, 0, 0, 0.02, 0.01, -0.03],            # pure rotations
        [0, 0, 0, 0.0, 0.3, 0.0],
        [0.01, 0.02, -0.01, 0.008, -0.004, 0.006],  # just above the guards (|w| = 0.0108)
        [0.2, -0.1, 0.05, 1.2, -0.7, 0.9],       # a large rotation
    ]
    t = torch.tensor(rows, dtype=torch.float32)
    rnd = torch.cat([0.1 * torch.randn((4, 3), generator=g), 0.2 * torch.randn((4, 3), generator=g)], 1)
    return torch.cat([t, rnd.float()], 0)


def main():
    from gstex_amd.scene import sphere_view

    ns = {"torch": torch}
    for src in extract_functions(REF_LIE, ["exp_map_SO3xR3", "exp_map_SE3"]).values():
        exec(src, ns)
    exec(extract_functions(REF_POSES, ["multiply"])["multiply"], ns)
    flip_src, lines = extract_flip_inverse(REF_MODEL)
    print(f"flip / inverse: gstex.py:{lines[0]}-{lines[1]}")

    tan = tangents()
    base = sphere_view(1, 64, 80)
    # the OpenGL camera_to_worlds whose flip / inverse is the base View: [R F | T] (F = diag(1, -1, -1), F F = I)
    c2w_gl = base.c2w.clone()
    c2w_gl[:3, :3] = base.c2w[:3, :3] @ torch.diag(torch.tensor([1.0, -1.0, -1.0]))

    class Cam:
        pass

    class Self:
        device = "cpu"

    out = dict(tangents=tan.numpy(), base_viewmat=base.viewmat.numpy(), base_c2w=base.c2w.numpy(),
               c2w_gl=c2w_gl.numpy())
    for mode, fn in (("SO3xR3", ns["exp_map_SO3xR3"]), ("SE3", ns["exp_map_SE3"])):
        corr = fn(tan)
        out[f"exp_{mode}"] = corr.numpy()
        vms, c2ws = [], []
        for i in range(tan.shape[0]):
            # apply_to_camera: camera_to_worlds (1, 3, 4) bmm [adj; 0 0 0 1] (camera_optimizers.py:160-162)
            adj = torch.cat([corr[i:i + 1], torch.Tensor([0, 0, 0, 1])[None, None]], dim=1)
            cam = Cam()
            cam.camera_to_worlds = torch.bmm(c2w_gl[None, :3, :], adj)
            # (the same product by poses.multiply, the convention forward() composes corrections with)
            assert torch.allclose(cam.camera_to_worlds[0], ns["multiply"](c2w_gl[:3, :], corr[i]), atol=1e-6)
            env = {"torch": torch, "camera": cam, "self": Self()}
            exec(flip_src, env)
            vms.append(env["viewmat"].numpy())
            c2ws.append(env["c2w"].numpy())
        out[f"viewmat_{mode}"] = np.stack(vms)
        out[f"c2w_{mode}"] = np.stack(c2ws)
    # sanity: the zero tangent gives the base View back
    for mode in ("SO3xR3", "SE3"):
        assert np.abs(out[f"viewmat_{mode}"][0][:3] - out["base_viewmat"]).max() < 1e-6
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
