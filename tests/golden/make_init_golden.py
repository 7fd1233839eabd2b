"""Generate the initialisation-file goldens from the REFERENCE's own loaders.

Run on the build machine only (it reads the reference checkout, which a GPU machine does not have):
    python tests/golden/make_init_golden.py path/to/reference
It writes two tiny inputs with gstex_amd.ply.write_ply
    tests/golden/init_2dgs.ply   16 splats, SH degree 3, 2DGS columns in a shuffled order with nx ny nz,
                                 quaternion norms in [0.5, 2]
    tests/golden/init_lod.ply    64 points, double x y z and uchar red green blue
and stores what the reference's loaders return for them in tests/golden/init_golden.npz, for fix_init /
fix_lod_init False and True.  The reference module cannot be imported whole (plyfile, open3d, gstex_cuda, ... are
absent), so load_ply, load_from_lod_ply and k_nearest_sklearn are AST-extracted from the source text and exec'd with a
stub PlyData backed by gstex_amd.ply.read_ply; utils/rotations.py (pure torch) is loaded stand-alone.  Only inputs and
outputs are committed.

Functions exercised (file:line):
  models/gstex.py:608   GStexModel.load_ply            (self.config stubbed)
  models/gstex.py:672   GStexModel.load_from_lod_ply
  models/gstex.py:775   GStexModel.k_nearest_sklearn
  utils/rotations.py    quaternion_to_matrix, matrix_to_quaternion
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from gstex_amd.ply import read_ply, write_ply  # noqa: E402

if len(sys.argv) != 2:
    sys.exit("usage: make_init_golden.py path/to/reference")
REF = os.path.join(sys.argv[1], "nerfstudio")


def extract(path, names):
    src = open(path).read()
    found = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in found:
            found[node.name] = ast.get_source_segment(src, node)
    missing = set(names) - set(found)
    assert not missing, missing
    return found


class _Element:
    """plyfile's PlyElement as the loaders use it: element[name] and element.properties[i].name."""

    def __init__(self, cols):
        self.cols = cols
        self.properties = [types.SimpleNamespace(name=k) for k in cols]

    def __getitem__(self, name):
        return self.cols[name]


class PlyData:
    @staticmethod
    def read(path):
        return types.SimpleNamespace(elements=[_Element(read_ply(path))])


def write_inputs():
    rng = np.random.default_rng(20240521)
    n, k = 16, 16
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    cols = {}
    for name, a in zip("xyz", f32(rng.uniform(-1, 1, (3, n)))):
        cols[name] = a
    for name in ("nx", "ny", "nz"):
        cols[name] = np.zeros(n, np.float32)
    for i in range(3):
        cols[f"f_dc_{i}"] = f32(rng.normal(0, 1, n))
    for i in range(3 * k - 3):
        cols[f"f_rest_{i}"] = f32(rng.normal(0, 0.1, n))
    cols["opacity"] = f32(rng.normal(0, 2, n))
    for i in range(2):
        cols[f"scale_{i}"] = f32(np.log(rng.uniform(0.02, 0.2, n)))
    q = rng.normal(0, 1, (n, 4))
    q *= (rng.uniform(0.5, 2.0, n) / np.linalg.norm(q, axis=1))[:, None]
    for i in range(4):
        cols[f"rot_{i}"] = f32(q[:, i])
    names = list(cols)
    rng.shuffle(names)
    write_ply(os.path.join(HERE, "init_2dgs.ply"), {name: cols[name] for name in names},
              comments=("gstex-mi355x test input: 16 splats in 2DGS layout, shuffled columns",))

    m = 64
    xyz = rng.uniform(-1, 1, (m, 3))
    rgb = rng.integers(0, 256, (m, 3)).astype(np.uint8)
    rgb[0], rgb[1] = 0, 255
    write_ply(os.path.join(HERE, "init_lod.ply"),
              {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "red": rgb[:, 0], "green": rgb[:, 1],
               "blue": rgb[:, 2]},
              comments=("gstex-mi355x test input: 64 coloured points",))


def main():
    write_inputs()
    spec = importlib.util.spec_from_file_location("ref_rotations", f"{REF}/utils/rotations.py")
    rot = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rot)
    ns = {"torch": torch, "np": np, "PlyData": PlyData, "quaternion_to_matrix": rot.quaternion_to_matrix,
          "matrix_to_quaternion": rot.matrix_to_quaternion}
    for code in extract(f"{REF}/models/gstex.py", ["load_ply", "load_from_lod_ply", "k_nearest_sklearn"]).values():
        exec(code, ns)

    out = {}
    for tag, fix in (("raw", False), ("fix", True)):
        me = types.SimpleNamespace(config=types.SimpleNamespace(sh_degree=3, fix_init=fix, fix_lod_init=fix))
        with torch.no_grad():
            res = ns["load_ply"](me, os.path.join(HERE, "init_2dgs.ply"))
        for name, t in zip(("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"), res):
            out[f"ply_{tag}_{name}"] = t.detach().numpy()
        xyz, rgbs = ns["load_from_lod_ply"](me, os.path.join(HERE, "init_lod.ply"))
        out[f"lod_{tag}_xyz"] = xyz.numpy()
        out[f"lod_{tag}_rgbs"] = rgbs.numpy()
        dist, _ = ns["k_nearest_sklearn"](me, xyz, 3)
        out[f"lod_{tag}_knn_dist"] = dist
    path = os.path.join(HERE, "init_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
