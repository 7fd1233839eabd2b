"""Shared inputs of tests/test_cluster.py and tests/test_gpu_cluster.py (no tests here): small splat sets that each
exercise one property of the clustering (gstex_amd.cluster), as CPU tensors.  A case is a dict: means (n, 3), scales
(n, 2) activated, quats (n, 4) unit wxyz, eps (on the SQUARED distance), min_pts (a tuple: the case runs once per
value) and cell_sizes (a tuple; None is the default cell)."""
import functools
import math

import torch


def _unit(q):
    return q / q.norm(dim=-1, keepdim=True)


def _qmul(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def sphere_shell_splats(n, seed, radius=1.0):
    """n splats on a sphere shell: normals radial, a random rotation in the surface, scales 0.3 to 0.6 of the mean
    spacing sqrt(4 pi / n) radius.  -> (means, scales (n, 2), quats), float32."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn((n, 3), generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    d[:, 2] = d[:, 2].clamp(min=-0.999)  # (the alignment below is singular at -z)
    d = d / d.norm(dim=1, keepdim=True)
    align = _unit(torch.stack([1.0 + d[:, 2], -d[:, 1], d[:, 0], torch.zeros(n, dtype=torch.float64)], -1))  # z -> d
    theta = torch.rand((n,), generator=g, dtype=torch.float64) * (2 * math.pi)
    spin = torch.stack([torch.cos(theta / 2), torch.zeros_like(theta), torch.zeros_like(theta), torch.sin(theta / 2)], -1)
    quats = _unit(_qmul(align, spin))
    spacing = math.sqrt(4 * math.pi / max(n, 1)) * radius
    scales = spacing * (0.3 + 0.3 * torch.rand((n, 2), generator=g, dtype=torch.float64))
    return (d * radius).float().contiguous(), scales.float().contiguous(), quats.float().contiguous()


def _shuffle(seed, *tensors):
    perm = torch.randperm(tensors[0].shape[0], generator=torch.Generator().manual_seed(seed))
    return tuple(t[perm].contiguous() for t in tensors)


def _identity(n):
    return torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)


def _case(means, scales, quats, eps, min_pts, cell_sizes=(None,)):
    return dict(means=means.float().contiguous(), scales=scales.float().contiguous(), quats=quats.float().contiguous(),
                eps=float(eps), min_pts=tuple(min_pts), cell_sizes=tuple(cell_sizes))


def _two_blobs_noise():
    g = torch.Generator().manual_seed(11)
    a = 0.05 * torch.randn((120, 3), generator=g)
    b = 0.05 * torch.randn((100, 3), generator=g) + torch.tensor([1.0, 0.0, 0.0])
    out = torch.rand((30, 3), generator=g) * 5.0 - 2.0
    means = torch.cat([a, b, out])
    n = means.shape[0]
    scales = 0.01 + 0.01 * torch.rand((n, 2), generator=g)
    quats = _unit(torch.randn((n, 4), generator=g))
    return _case(*_shuffle(12, means, scales, quats), eps=0.0016, min_pts=(5,))


def _chain():
    n = 300
    means = torch.zeros((n, 3))
    means[:, 0] = torch.arange(n) * 0.1
    scales = torch.full((n, 2), 0.01)
    return _case(*_shuffle(13, means, scales, _identity(n)), eps=0.012, min_pts=(2, 3))


def _contested_border():
    # along x: cluster X (indices 0..4) runs away to the left, cluster Y (5..9) to the right and comes nearer; the
    # border splat (index 10) sees one core of each.  eps = 1, min_pts = 3.
    xs = [-0.9, -1.3, -1.7, -2.1, -2.5, 0.8, 1.2, 1.6, 2.0, 2.4, 0.0]
    means = torch.zeros((len(xs), 3))
    means[:, 0] = torch.tensor(xs)
    scales = torch.full((len(xs), 2), 0.001)
    return _case(means, scales, _identity(len(xs)), eps=1.0, min_pts=(3,))


def _orientation_splits():
    # 20 discs with the normal along z (identity) and 20 with the normal along x (a quarter turn about y), each
    # spun about its own normal; radius 0.1, centres within 1e-3: parallel discs have tr = 0, perpendicular ones
    # tr = 2 s^2 = 0.02, and eps = 0.01 lies between.
    g = torch.Generator().manual_seed(14)
    n = 40
    means = 1e-3 * torch.rand((n, 3), generator=g)
    tilt = _identity(n).double()
    c = math.sqrt(0.5)
    tilt[n // 2:] = torch.tensor([c, 0.0, c, 0.0], dtype=torch.float64)
    theta = torch.rand((n,), generator=g, dtype=torch.float64) * (2 * math.pi)
    spin = torch.stack([torch.cos(theta / 2), torch.zeros_like(theta), torch.zeros_like(theta), torch.sin(theta / 2)], -1)
    quats = _unit(_qmul(tilt, spin)).float()
    scales = torch.full((n, 2), 0.1)
    means, scales, quats, normal_x = _shuffle(15, means, scales, quats, torch.arange(n) >= n // 2)
    case = _case(means, scales, quats, eps=0.01, min_pts=(5,))
    case["normal_x"] = normal_x
    return case


def _ties():
    r = torch.arange(5, dtype=torch.float32)
    means = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    n = means.shape[0]
    scales = torch.tensor([0.25, 0.5]).repeat(n, 1)
    return _case(*_shuffle(16, means, scales, _identity(n)), eps=1.0, min_pts=(6, 7))


def _duplicates():
    g = torch.Generator().manual_seed(17)
    base = torch.rand((30, 3), generator=g)
    means = torch.cat([base, base[:20], base[:10]])  # the first 10 three times, the next 10 twice, the last 10 once
    n = means.shape[0]
    scales = torch.tensor([0.25, 0.5]).repeat(n, 1)
    case = _case(*_shuffle(18, means, scales, _identity(n)), eps=0.0, min_pts=(1, 2))
    return case


def _shell(n, seed, cell_sizes=(None,)):
    means, scales, quats = sphere_shell_splats(n, seed)
    spacing = math.sqrt(4 * math.pi / n)
    # a radius of 1.8 spacings and min_pts = 10: cores, border splats and noise side by side, several clusters; the
    # radius is a twentieth of the sphere's diameter or more, so cells of sqrt(eps) / 20 still fit the cell limits
    return _case(means, scales, quats, eps=(1.8 * spacing) ** 2, min_pts=(10,), cell_sizes=cell_sizes)


@functools.lru_cache(maxsize=None)
def cases():
    big = _shell(4001, 23)
    root = math.sqrt(big["eps"])
    big["cell_sizes"] = (4.0, None, root / 20.0)  # one cell, the default, cells far below the radius
    return {"two_blobs_noise": _two_blobs_noise(), "chain": _chain(), "contested_border": _contested_border(),
            "orientation_splits": _orientation_splits(), "ties": _ties(), "duplicates": _duplicates(),
            "single": _shell(1, 21), "n=65": _shell(65, 22), "n=4001": big}


def runs(small_only=False):
    """(case name, min_pts, cell_size) of every run."""
    out = []
    for name, c in cases().items():
        if small_only and c["means"].shape[0] > 1000:
            continue
        for m in c["min_pts"]:
            for h in c["cell_sizes"]:
                out.append((name, m, h))
    return out
