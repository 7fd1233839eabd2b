"""Shared inputs of tests/test_neighbors.py and tests/test_gpu_neighbors.py (no test in here): the grid cases of the
nearest-neighbour search and the meshes of the sampler tests."""
import functools
import math

import torch


def _rand(n, seed, scale=1.0, shift=0.0):
    return torch.rand((n, 3), generator=torch.Generator().manual_seed(seed)) * scale + shift


def _lattice(n, step=1.0):
    ax = torch.arange(n, dtype=torch.float32) * step
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def grid_cases():
    """name -> dict(points, queries, cell_size, k, exclude_self, max_radius): every case of the issue's list.  The
    points of a case with exclude_self are its queries."""
    cases = {}

    def add(name, points, queries, cell_size, k=3, exclude_self=False, max_radius=None):
        cases[name] = dict(points=points.contiguous(), queries=queries.contiguous(), cell_size=cell_size, k=k,
                           exclude_self=exclude_self, max_radius=max_radius)

    p = _rand(200, 1)
    add("one_cell", p, _rand(50, 2, 1.4, -0.2), 4.0)
    # nine points a unit apart in a plane, cells of 0.02: up to fifty empty rings between neighbours
    plane = _lattice(3)[:9].clone()
    add("tiny_cells", plane, torch.cat([plane + 0.3, _rand(6, 3, 2.0)[:, :3] * torch.tensor([1.0, 1.0, 0.0])]), 0.02,
        k=2)
    # points exactly on cell boundaries lo + i h (h = 0.25, exact in fp32) and at the maximum corner
    edge = _lattice(5, 0.25)
    add("boundaries", edge, torch.cat([edge, edge + 0.125, _rand(40, 4, 1.2, -0.1)]), 0.25, k=4)
    add("coincident", torch.full((7, 3), 0.37), torch.cat([torch.full((1, 3), 0.37), _rand(5, 5)]), 0.1, k=8)
    add("single_point", torch.tensor([[0.2, -0.1, 0.4]]), _rand(9, 6, 2.0, -1.0), 0.5, k=3)
    far = torch.tensor([[-90.0, 0.5, 0.5], [90.0, 0.5, 0.5], [0.5, -75.0, 0.5], [0.5, 75.0, 0.5], [0.5, 0.5, -60.0],
                        [0.5, 0.5, 60.0], [-40.0, 55.0, -70.0], [1e6, -1e6, 1e6]])
    add("far_outside", p, far, 0.2, k=3)
    add("k_above_n", _rand(5, 7), _rand(11, 8), 0.3, k=8)
    add("radius_excludes_all", p, _rand(30, 9, 1.0, 5.0), 0.2, k=3, max_radius=0.5)
    # collinear points at 0, 1, 2.5, 4.5: from the query at -0.5 the neighbours are 0.5, 1.5, 3.0, 5.0 away
    line = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.5, 0.0, 0.0], [4.5, 0.0, 0.0]])
    add("radius_cuts_2_3", line, torch.tensor([[-0.5, 0.0, 0.0]]), 0.5, k=4, max_radius=2.0)
    dup = torch.cat([p[:40], p[:40], p[:10]])  # every point two or three times
    add("duplicates_exclude_self", dup, dup, 0.15, k=3, exclude_self=True)
    lat = _lattice(4)
    lat = lat[torch.randperm(lat.shape[0], generator=torch.Generator().manual_seed(10))]
    # queries at cell centres of the lattice: eight equidistant neighbours each; and at lattice points: six at 1
    add("lattice_ties", lat, torch.cat([_lattice(3) + 0.5, _lattice(4)]), 0.7, k=8)
    return cases


def random_case():
    """5,000 points and 4,001 queries (no multiple of 64 or 256), the queries reaching past the points' box."""
    return _rand(5000, 21), _rand(4001, 22, 1.2, -0.1)


# ------------------------------------------------------------------------------------------ sampler meshes
def hand_mesh():
    """A hand-made mesh at spacing 1: faces with n = 1, 2 and 5, a sliver, a degenerate zero-area face (three collinear
    vertices) and a face repeated with another winding.  -> (vertices, faces, spacing, n per face)."""
    v = torch.tensor([[0.0, 0.0, 0.0], [0.6, 0.0, 0.0], [0.0, 0.6, 0.1],      # longest edge 0.85: n = 1
                      [2.0, 0.0, 0.0], [3.7, 0.1, 0.0], [2.6, 1.2, 0.3],      # longest edge 1.70: n = 2
                      [0.0, 3.0, 1.0], [4.6, 3.0, 1.0], [0.3, 5.0, 1.5],      # longest edge 4.77: n = 5
                      [5.0, 0.0, 0.0], [8.9, 0.0, 0.0], [6.0, 1e-3, 0.0],     # a sliver (height 1e-3), n = 4
                      [0.0, 0.0, 5.0], [1.0, 1.0, 6.0], [2.5, 2.5, 7.5]],     # collinear: zero area, n = 5
                     dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [2, 0, 1]], dtype=torch.int32)
    V = v.double()
    n = []
    for a, b, c in f.tolist():
        L = max(float((V[b] - V[a]).norm()), float((V[c] - V[a]).norm()), float((V[c] - V[b]).norm()))
        n.append(max(1, math.ceil(L)))
    assert {1, 2, 5} <= set(n)
    return v, f, 1.0, n


@functools.lru_cache(maxsize=None)
def sphere_mesh(n=16, r_over_h=5.3):
    """The marching-tetrahedra sphere of mesh_cases.sphere_field from the extraction's twin: (vertices, faces, r, h)."""
    import mesh_cases as C
    from gstex_amd import mesh as M

    tsdf, weight, origin, h, r = C.sphere_field(n, r_over_h)
    V, _, F = M.mesh_extract_eager(tsdf, weight, None, origin, h)
    return V, F, r, h


def mesh_area64(vertices, faces) -> float:
    V, F = vertices.double(), faces.long()
    return float(0.5 * torch.linalg.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]).norm(dim=1).sum())


def sphere_points(n, radius):
    """n points on the sphere of that radius: a Fibonacci spiral normalised in float64, rounded once."""
    i = torch.arange(n, dtype=torch.float64) + 0.5
    z = 1 - 2 * i / n
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    rxy = torch.sqrt(1 - z * z)
    p = torch.stack([rxy * torch.cos(phi), rxy * torch.sin(phi), z], -1)
    p = p / p.norm(dim=1, keepdim=True)
    return (radius * p).float().contiguous()
