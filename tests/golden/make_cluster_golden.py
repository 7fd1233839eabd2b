"""Pin the splat clustering with the REFERENCE's own code (dbscan_clustering/dbscan_ballquery.py).

Run where the reference's sources are (a GPU test machine does not have them):
    python tests/golden/make_cluster_golden.py <reference checkout>      (or GSTEX_REFERENCE=<reference checkout>)
Writes tests/golden/cluster.npz.  wasserstein_3d_gaussians, sqrtm_psd_3x3, make_covariance_3d and BallQueryDBSCAN's
find_neighbors and fit are AST-extracted from the source text (as make_conventions_golden.py does) and exec'd in
float64, with quaternion_to_matrix extracted from nerfstudio/utils/rotations.py; pytorch3d's ball_query is replaced by
brute force (the points with squared distance below radius^2, in index order, at most K, padded with -1), tqdm by the
identity and the logger by a silent one.  Only inputs and outputs are committed.

The inputs (inputs() below): a thinned, jittered lattice of randomly oriented splats and two sets of near-coincident
discs that only the trace term separates, about 300 in all, every mean, log-scale and quaternion a float32 number held
in float64.  The generator asserts what makes the reference's result the definition's:
  * eps * multiplier >= sqrt(eps): the ball holds every true neighbour;
  * every ball holds fewer than 1000 candidates and fewer than 80 % of the points (no cap, no halved radius);
  * no pair has the reference's W^2 within m = 10 gap of eps, gap being the largest difference over the stored pairs
    between the closed form of the contract evaluated in float64 and the reference's float64 value (its 1e-12
    eigenvalue clamp and the dropped third scale).
Stored: the inputs, eps, min_pts, multiplier, the reference's labels, the pairs i < j inside a ball with the
reference's W^2, and gap.
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "cluster.npz")

EPS, MIN_PTS, MULTIPLIER = 0.0038, 4, 20.0


def extract(path, names):
    src = open(path).read()
    found = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in found:
            found[node.name] = textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    assert set(found) == set(names), set(names) - set(found)
    return found


def ball_query_brute(p1, p2, radius, K, return_nn=False):
    d2 = ((p1[0, :, None, :] - p2[0, None, :, :]) ** 2).sum(-1)  # (Q, N)
    idx = torch.full((1, p1.shape[1], K), -1, dtype=torch.long)
    for q in range(p1.shape[1]):
        hit = torch.nonzero(d2[q] < radius * radius)[:, 0][:K]
        idx[0, q, :hit.shape[0]] = hit
    return None, idx, None


def reference(ref_root):
    fns = extract(os.path.join(ref_root, "dbscan_clustering", "dbscan_ballquery.py"),
                  ["wasserstein_3d_gaussians", "sqrtm_psd_3x3", "make_covariance_3d", "find_neighbors", "fit"])
    fns.update(extract(os.path.join(ref_root, "nerfstudio", "utils", "rotations.py"), ["quaternion_to_matrix"]))
    quiet = types.SimpleNamespace(debug=lambda *a, **k: None, info=lambda *a, **k: None,
                                  warning=lambda *a, **k: (_ for _ in ()).throw(AssertionError(a)))
    ns = {"torch": torch, "np": np, "logger": quiet, "tqdm": lambda it, **k: it, "ball_query": ball_query_brute}
    for name in ("quaternion_to_matrix", "make_covariance_3d", "sqrtm_psd_3x3", "wasserstein_3d_gaussians",
                 "find_neighbors", "fit"):
        exec(fns[name], ns)
    return ns


def inputs(seed):
    """A 7 x 7 x 7 lattice of pitch 0.05 with a fifth of its sites left empty and every kept site moved by up to
    0.002 per axis, splats of random orientation and scales 0.004 to 0.01: pairs one pitch apart have W^2 below
    0.0034, every other pair has d^2 above 0.0042, and eps = 0.0038 lies in between; the empty sites leave cores,
    border splats and noise.  Next to it 2 x 10 discs of radius 0.05 with near-coincident centres, the normals of one
    half along z and of the other along x: parallel discs have W^2 near 0, perpendicular ones near 2 * 0.05^2 =
    0.005, so only the trace term keeps them apart."""
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(7, dtype=torch.float32) * 0.05
    sites = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    sites = sites[torch.rand((sites.shape[0],), generator=g) < 0.8]
    means = sites + (torch.rand(sites.shape, generator=g) * 2 - 1) * 0.002
    k = means.shape[0]
    scales = 0.004 + 0.006 * torch.rand((k, 3), generator=g)
    quats = torch.randn((k, 4), generator=g)
    discs = torch.tensor([0.6, 0.6, 0.6]) + 1e-3 * torch.rand((20, 3), generator=g)
    c = 0.5 ** 0.5
    tilt = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 10 + [[c, 0.0, c, 0.0]] * 10)
    means, scales, quats = torch.cat([means, discs]), torch.cat([scales, torch.full((20, 3), 0.05)]), torch.cat([quats, tilt])
    quats = quats / quats.norm(dim=1, keepdim=True)
    perm = torch.randperm(means.shape[0], generator=g)
    return means[perm].double(), torch.log(scales)[perm].double(), quats[perm].double()  # float32 numbers, in float64


def closed_form64(means, scales, quats, i, j):
    from gstex_amd import cluster as C

    a, b, T = C.shapes_eager(scales, quats / quats.norm(dim=1, keepdim=True))
    return C._d2_eager(means[i], means[j]) + C._trace_eager(a[i], b[i], T[i], a[j], b[j], T[j])


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["GSTEX_REFERENCE"]
    ns = reference(ref_root)
    assert EPS * MULTIPLIER >= np.sqrt(EPS)
    radius = EPS * MULTIPLIER
    for seed in range(100):  # the first seed whose W^2 values keep clear of eps
        means, log_scales, quats = inputs(seed)
        n = means.shape[0]
        d2 = ((means[:, None] - means[None]) ** 2).sum(-1)
        inside = d2 < radius * radius
        per_ball = inside.sum(1)
        assert int(per_ball.max()) < min(1000, 0.8 * n), int(per_ball.max())
        i, j = torch.nonzero(torch.triu(inside, diagonal=1), as_tuple=True)
        w2 = ns["wasserstein_3d_gaussians"](means[i], log_scales[i], quats[i], means[j], log_scales[j], quats[j])
        gap = float((closed_form64(means, torch.exp(log_scales[:, :2]), quats, i, j) - w2).abs().max())
        clear = float((w2 - EPS).abs().min())
        print(f"seed {seed}: n {n}, {i.shape[0]} pairs inside a ball, at most {int(per_ball.max())} per ball, gap "
              f"{gap:.3e}, nearest W^2 to eps {clear:.3e}")
        if clear >= 10 * gap:
            break
    else:
        raise AssertionError("no seed keeps every W^2 clear of eps")
    model = types.SimpleNamespace(eps=EPS, min_pts=MIN_PTS, search_radius_multiplier=MULTIPLIER)
    model.find_neighbors = types.MethodType(ns["find_neighbors"], model)
    gaussians = types.SimpleNamespace(xyz=means, scaling=log_scales, rotation=quats)
    labels = ns["fit"](model, gaussians)
    assert int((labels == -2).sum()) == 0 and int(labels.max()) >= 2
    print(f"labels: {int(labels.max())} clusters, {int((labels == -1).sum())} noise")
    np.savez_compressed(OUT, means=means.numpy(), log_scales=log_scales.numpy(), quats=quats.numpy(),
                        eps=np.float64(EPS), min_pts=np.int64(MIN_PTS), multiplier=np.float64(MULTIPLIER),
                        labels=labels.numpy().astype(np.int32), pair_i=i.numpy().astype(np.int16),
                        pair_j=j.numpy().astype(np.int16), pair_w2=w2.numpy(), gap=np.float64(gap), seed=np.int64(seed))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 100 * 1024


if __name__ == "__main__":
    main()
