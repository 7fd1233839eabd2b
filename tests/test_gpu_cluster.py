"""The clustering kernels (gstex_amd/csrc/cluster.hip) against the eager twins of gstex_amd.cluster run on the CPU:
labels, degree, core and the number of clusters exactly, the distance bit for bit; GStexTrainer.cluster; and the result's
independence of run, of the splats' order and of the cell size."""
import pytest
import torch

import cluster_cases as CC
from gstex_amd import cluster as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _splats(c, dev="cpu"):
    return c["means"].to(dev), c["scales"].to(dev), c["quats"].to(dev)


@pytest.fixture(scope="module")
def twins():
    """The CPU twin's result per (case, min_pts): computed once, shared, not modified."""
    cache = {}

    def get(name, min_pts):
        if (name, min_pts) not in cache:
            c = CC.cases()[name]
            cache[name, min_pts] = C.dbscan_eager(*_splats(c), c["eps"], min_pts)
        return cache[name, min_pts]

    return get


def _same(got, want, what):
    assert got.labels.is_cuda and got.labels.dtype == torch.int32 and got.degree.dtype == torch.int32
    assert got.core.dtype == torch.bool
    for name in ("degree", "core", "labels"):
        a, b = getattr(got, name).cpu(), getattr(want, name)
        assert a.shape == b.shape, (what, name)
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} of {a.numel()} splats"
    assert got.n_clusters == want.n_clusters, what


@pytest.mark.parametrize("name,min_pts,cell_size", CC.runs())
def test_kernels_match_twin(twins, name, min_pts, cell_size):
    c = CC.cases()[name]
    got = C.dbscan(*_splats(c, DEV), c["eps"], min_pts, cell_size=cell_size)
    _same(got, twins(name, min_pts), f"{name} min_pts={min_pts} cell={cell_size}")


def test_sizes_are_no_multiple_of_a_wave_or_a_block():
    for name in ("n=65", "n=4001"):
        n = CC.cases()[name]["means"].shape[0]
        assert n % 64 != 0 and n % 256 != 0


def test_pair_w2_matches_twin_bit_for_bit():
    c = CC.cases()["n=4001"]
    n = c["means"].shape[0]
    g = torch.Generator().manual_seed(31)
    near = C.neighbor_pairs_eager(*_splats(c), 4 * c["eps"])  # half of the pairs near the radius, half anywhere
    pick = torch.randperm(near[0].shape[0], generator=g)[:1000]
    pairs = torch.cat([torch.stack([near[0][pick], near[1][pick]], 1), torch.randint(0, n, (1000, 2), generator=g)])
    pairs[-1] = torch.tensor([7, 7])  # a splat against itself
    want = C.wasserstein2_eager(*_splats(c), pairs[:, 0], pairs[:, 1])
    got = C.pair_w2(*_splats(c, DEV), pairs.to(DEV))
    for a, b, name in zip(got, want, ("w2", "d2", "tr")):
        assert a.is_cuda and a.dtype == torch.float32 and a.shape == (2000,)
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), \
            f"{name} differs in {int((a.cpu() != b).sum())} of 2000 pairs"
    assert float(want[1][-1]) == 0.0
    bad = C.pair_w2(*_splats(c, DEV), torch.tensor([[0, n], [-1, 3]], device=DEV))  # outside [0, n): no distance
    assert bool(torch.isnan(bad[0]).all())


def test_trainer_cluster_equals_twin_on_its_activated_parameters():
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene

    scene = make_scene(n=600, n_texels=6000, seed=5)
    tr = GStexTrainer(scene, DEV, sh_degree=3)
    before = {k: [p.detach().clone() for p in ps] for k, ps in tr.param_groups().items()}
    means, scales, quats = (t.cpu() for t in tr.activated_splats())
    d = torch.cdist(means.double(), means.double())
    eps = float(d.topk(5, dim=1, largest=False).values[:, 4].median()) ** 2  # the median fourth neighbour's distance
    got = tr.cluster(eps, 3)
    want = C.dbscan_eager(means, scales, quats, eps, 3)
    assert want.n_clusters >= 2 and bool((want.labels == -1).any())
    _same(got, want, "trainer")
    for k, ps in tr.param_groups().items():
        for p, q in zip(ps, before[k]):
            assert torch.equal(p.detach(), q), k


def test_result_is_the_same_across_runs_and_orders(twins):
    """Twice on the same input, and with the splats permuted: degree and core map back through the permutation, and so
    do the labels once the ids are renumbered by each cluster's lowest ORIGINAL core index (the id rule)."""
    c = CC.cases()["n=4001"]
    want = twins("n=4001", 10)
    a = C.dbscan(*_splats(c, DEV), c["eps"], 10)
    b = C.dbscan(*_splats(c, DEV), c["eps"], 10)
    _same(a, want, "first run")
    _same(b, want, "second run")
    n = c["means"].shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(41))  # new position k holds splat perm[k]
    p = C.dbscan(*(t[perm].contiguous().to(DEV) for t in _splats(c)), c["eps"], 10)
    back = torch.empty(n, dtype=torch.int64)
    back[perm] = torch.arange(n)
    degree, core, lab = p.degree.cpu()[back], p.core.cpu()[back], p.labels.cpu()[back].long()
    assert torch.equal(degree, want.degree) and torch.equal(core, want.core) and p.n_clusters == want.n_clusters
    assert torch.equal(lab == -1, want.labels == -1)
    # renumber: a cluster's id = 1 + the rank of its lowest original core index
    K = p.n_clusters
    lowest = torch.full((K + 1,), n, dtype=torch.int64)
    cores = torch.nonzero(core)[:, 0]
    lowest.scatter_reduce_(0, lab[cores], cores, "amin")
    rank = torch.empty(K + 1, dtype=torch.int64)
    rank[torch.argsort(lowest[1:]) + 1] = torch.arange(1, K + 1)
    renumbered = torch.where(lab > 0, rank[lab.clamp(min=0)], lab)
    # a border splat takes the lowest id among its core neighbours, and which id is lowest depends on the numbering:
    # compare the cores exactly, and the border splats by membership in a neighbouring core's cluster
    assert torch.equal(renumbered[core], want.labels.long()[core])
    border = ~core & (lab > 0)
    src, dst = C.neighbor_pairs_eager(*_splats(c), c["eps"])
    ok = torch.zeros(n, dtype=torch.bool)
    hit = core[dst] & (renumbered[src] == want.labels.long()[dst])
    ok[src[hit]] = True
    assert bool(ok[border].all())
