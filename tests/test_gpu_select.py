"""Selecting splats on the GPU: gstex_select_plan / _dims / _texels against their eager twin (exactly: values are
copied, never rounded), and GStexTrainer.select across a render, a backward, further training, a rechart, paint,
evaluate, the NPZ round trip and a selection built from cluster labels (DESIGN.md "Selecting splats")."""
import pytest
import torch

from select_cases import GUARD_ROWS, MASK_NAMES, SENTINEL, chart_list, guarded_alloc, loop_select, masks, sources

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
H, W = 64, 80


# ---------------------------------------------------------------------------------------- kernels against the twin
def _kernels_match_the_twin(dims, T, keep, channels=3):
    from gstex_amd import select as sel

    src = sources(T, channels)
    want_dims, want, want_T = sel.select_texture_eager(dims, T, keep, src)
    got = []
    for sentinel in (SENTINEL, 777.0):  # the capacity rows are never read: their content does not show
        dev_src = [s.to(DEV) for s in sources(T, channels, sentinel=sentinel)]
        alloc, buffers = guarded_alloc(DEV)
        new_dims, new, T_new = sel.select_texture(dims.to(DEV), T, keep.to(DEV), dev_src, alloc)
        torch.cuda.synchronize()
        assert T_new == want_T and new_dims.dtype == torch.int32 and torch.equal(new_dims.cpu(), want_dims)
        assert len(new) == 3 and sorted(buffers) == [0, 1, 2]
        for k in range(3):
            assert tuple(new[k].shape) == (want_T, channels)
            assert want_T == 0 or new[k].data_ptr() == buffers[k].data_ptr()  # (an empty view has no address)
            assert torch.equal(new[k].cpu(), want[k]), (k, sentinel)
            guard = buffers[k][want_T:]
            assert guard.shape[0] == GUARD_ROWS and bool((guard == SENTINEL).all()), k  # nothing written past T_new
            assert torch.equal(dev_src[k][:T].cpu(), src[k][:T]) and bool((dev_src[k][T:] == sentinel).all())
        got.append([t.cpu() for t in new])
    assert all(torch.equal(a, b) for a, b in zip(*got))
    return want_T


@pytest.mark.parametrize("mask", MASK_NAMES)
def test_kernels_match_the_twin_on_the_standard_charts(mask):
    dims, T = chart_list(600)
    T_new = _kernels_match_the_twin(dims, T, masks(dims)[mask])
    assert (T_new == 0) == (mask in ("zero_texel_only", "first")) and (T_new == T) == (mask == "all")  # splat 0: (0, 0)


@pytest.mark.parametrize("case", ["reverse", "channels_1", "channels_8", "n_1", "n_1_zero_texels", "n_257", "dense"])
def test_kernels_match_the_twin_on_other_layouts(case):
    n, kw, channels = 600, {}, 3
    if case == "reverse":
        kw = dict(reverse=True)
    elif case.startswith("channels"):
        channels = int(case[-1])
    elif case == "n_1":
        n, kw = 1, dict(start=3)  # one (3, 5) chart
    elif case == "n_1_zero_texels":
        n = 1  # one (0, 0) chart
    elif case == "n_257":
        n = 257
    dims, T = chart_list(n, **kw)
    if case == "dense":
        # 3000 one-texel charts with a zero-texel chart after every third: more charts than texels in a workgroup's
        # run of 1024 texels, so the per-texel search runs over a wide chart range
        hw = torch.tensor([[1, 1], [1, 1], [1, 1], [0, 7]] * 1000, dtype=torch.int64)
        size = hw[:, 0] * hw[:, 1]
        dims = torch.cat([hw, (torch.cumsum(size, 0) - size)[:, None]], 1).to(torch.int32)
        T = int(size.sum())
    _kernels_match_the_twin(dims, T, masks(dims)["every_other"], channels)


def test_plan_matches_the_twin_and_flags_malformed_rows():
    from gstex_amd import select as sel

    dims, T = chart_list(600)
    for name in ("every_other", "bernoulli", "zero_texel_only", "all"):
        keep = masks(dims)[name]
        want = sel.select_plan_eager(dims, T, keep)
        got = sel.select_plan(dims.to(DEV), T, keep.to(DEV))
        for a, b, what in zip(got, want, ("rows", "texels", "row_off", "tex_off", "flag")):
            assert a.dtype == torch.int32 and torch.equal(a.cpu(), b), (name, what)
        plan = sel.plan_selection(dims.to(DEV), T, keep.to(DEV))
        assert (plan.n_new, plan.n_texels_new, plan.flagged) == (int(want[2][-1]), int(want[3][-1]), False)
    keep = masks(dims)["every_other"]
    for row, at in (((-1, 5, 0), 3), ((3, -5, 0), 3), ((3, 5, -1), 4), ((65536, 65536, 0), 599),
                    ((3, 5, T - 14), 0), ((1, 1, T), 301)):  # kept rows and dropped ones
        bad = dims.clone()
        bad[at] = torch.tensor(row, dtype=torch.int32)
        want = sel.select_plan_eager(bad, T, keep)
        got = sel.select_plan(bad.to(DEV), T, keep.to(DEV))
        assert int(got[4].cpu()) == 1 == int(want[4]), row
        assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[3].cpu(), want[3]), row
        with pytest.raises(ValueError, match="malformed"):
            sel.select_texture(bad.to(DEV), T, keep.to(DEV), [sources(T, count=1)[0].to(DEV)])
    ok = dims.clone()
    ok[3] = torch.tensor((3, 5, T - 15), dtype=torch.int32)  # the last block that still fits
    assert int(sel.select_plan(ok.to(DEV), T, keep.to(DEV))[4].cpu()) == 0


# ---------------------------------------------------------------------------------------- the trainer
def _textured_trainer(steps=3, seed=42, **kw):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    kw.setdefault("start_step", 3000)  # (every SH degree is active, so every group but features_dc has a gradient)
    tr = GStexTrainer(make_scene(400, 2e4, seed=seed), DEV, defer_texture=True, **kw)
    view = sphere_view(2, H, W).to(DEV)
    gt = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    for _ in range(steps):
        tr.zero_grad()
        tr.forward_backward(view, gt)
        tr.optimizer_step()
    tr.wait_texture()
    return tr, view, gt


def _state(tr):
    """name -> (parameter, exp_avg, exp_avg_sq, step) on the CPU (moments None where Adam holds nothing)."""
    out = {}
    for name, (p,) in tr.param_groups().items():
        st = tr.optimizer.state.get(p)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        out[name] = (c(p), c(st["exp_avg"]), c(st["exp_avg_sq"]), st["step"]) if st else (c(p), None, None, None)
    return out


def _count_fused(monkeypatch):
    from gstex_amd import fused

    calls = [0]
    inner = fused.train_render

    def counted(*a, **k):
        calls[0] += 1
        return inner(*a, **k)
    monkeypatch.setattr(fused, "train_render", counted)
    return calls


def test_render_is_unchanged_and_state_is_gathered():
    tr, view, _ = _textured_trainer()
    n, T = tr.means.shape[0], tr.n_texels
    dims = tr.texture_dims.cpu()
    assert n == 400 and int((dims[:, 0] * dims[:, 1]).max()) > 1 and tr.texture_dc.shape[0] >= T
    keep = torch.arange(n) % 2 == 0
    drop = (~keep).to(DEV)
    with torch.no_grad():  # the reference: the dropped splats made invisible (sigmoid(-100) is far below the 1/255 skip)
        logits = tr.opacities.detach().clone()
        tr.opacities[drop] = -100.0
        ref = {k: v.clone() for k, v in tr.eval_render(view).items() if k in ("rgb", "alpha", "depth")}
        tr.opacities.copy_(logits)
    assert float(ref["alpha"].max()) > 0.05
    before, mappings = _state(tr), tr.mappings.cpu().clone()
    assert all(v[3] == 3 and bool(v[2].any()) for k, v in before.items() if v[3] is not None) and before["texture_dc"][3] == 3

    res = tr.select(keep)  # (a CPU mask on a device trainer)
    kept = torch.nonzero(keep)[:, 0]
    tex = before["texture_dc"]
    want_dims, want_tex, want_T = loop_select(dims, keep, [tex[0], tex[1], tex[2]])
    assert tuple(res) == (n, 200, T, want_T) and tr.n_texels == want_T and tr.means.shape[0] == 200
    assert torch.equal(tr.texture_dims.cpu(), want_dims) and torch.equal(tr.mappings.cpu(), mappings[kept])
    for g in tr.optimizer.param_groups:
        name = g["name"]
        (p,) = tr.param_groups()[name]
        assert g["params"][0] is p
        val, ea, eas, step = before[name]
        want = (want_tex if name == "texture_dc" else [val[kept], None if ea is None else ea[kept],
                                                       None if eas is None else eas[kept]])
        assert torch.equal(p.detach().cpu(), want[0]), name
        if step is None:
            assert p not in tr.optimizer.state
            continue
        st = tr.optimizer.state[p]
        assert st["step"] == step
        assert torch.equal(st["exp_avg"].cpu(), want[1]) and torch.equal(st["exp_avg_sq"].cpu(), want[2]), name
    assert tuple(tr.texture_dc.shape) == (want_T, 3)
    base = tr.geometry_flat.data_ptr()
    for p in (tr.means, tr.scales, tr.quats, tr.opacities):
        assert (p.data_ptr() - base) % 16 == 0 and 0 <= p.data_ptr() - base < 4 * tr.geometry_flat.numel()
    with torch.no_grad():
        out = tr.eval_render(view)
    for key in ("rgb", "alpha", "depth"):
        err = float((out[key] - ref[key]).abs().max())
        print(f"select render invariance: max |{key} difference| = {err:.3e}")
        assert err <= 1e-5, key


def _norm_err(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_gradients_of_the_kept_splats_are_unchanged():
    a, view, gt = _textured_trainer(steps=0)
    b, _, _ = _textured_trainer(steps=0)
    n = 400
    keep = torch.arange(n) % 2 == 0
    dims, T = b.texture_dims.cpu(), b.n_texels
    a.select(keep.to(DEV))  # (a device mask)
    with torch.no_grad():
        b.opacities[(~keep).to(DEV)] = -100.0
    for tr in (a, b):
        tr.zero_grad()
        tr.forward_backward(view, gt)
    torch.cuda.synchronize()
    kept = torch.nonzero(keep)[:, 0]
    compared = 0
    for name in a.param_groups():
        ga, gb = a.param_groups()[name][0].grad, b.param_groups()[name][0].grad
        assert (ga is None) == (gb is None), name
        if ga is None:
            continue
        ga, gb = ga.detach().cpu(), gb.detach().cpu()
        want = loop_select(dims, keep, [gb])[1][0] if name == "texture_dc" else gb[kept]
        assert ga.shape == want.shape and float(want.abs().max()) > 0, name
        err = _norm_err(ga, want)
        print(f"select gradient invariance: {name}: norm-wise error {err:.3e}")
        assert err <= 2e-5, name
        compared += 1
    assert compared >= 6


def test_training_goes_on_after_select(monkeypatch, tmp_path):
    from gstex_amd.export import export_npz, trainer_from_npz

    calls = _count_fused(monkeypatch)
    tr, view, gt = _textured_trainer(fused_step=True)
    c0 = calls[0]
    assert c0 >= 2  # (the first step's render sizes the pair capacity on the per-op path)
    n = tr.means.shape[0]
    res = tr.select(torch.arange(n) % 2 == 0)
    assert res.n_after == 200 and tr._fused_ok(False, None, view)
    for k in range(2):
        tr.zero_grad()
        out = tr.forward_backward(view, gt)
        tr.optimizer_step()
        assert calls[0] == c0 + 1 + k and bool(torch.isfinite(out.loss))
    tr.wait_texture()
    assert tr.skipped_steps == [] and tr.optimizer.state[tr.texture_dc]["step"] == 5
    assert all(bool(torch.isfinite(p).all()) for p in tr.parameters())
    tr.recharge()
    dims = tr.texture_dims.cpu()
    assert tr.n_texels == int((dims[:, 0].long() * dims[:, 1].long()).sum())
    m = tr.means.shape[0]
    keep = torch.arange(m) % 3 != 0
    tex = tr.texels()[:tr.n_texels].cpu().clone()
    want_dims, (want_tex,), want_T = loop_select(dims, keep, [tex])
    res = tr.select(keep.to(DEV))
    assert tuple(res) == (m, int(keep.sum()), int(tex.shape[0]), want_T)
    assert torch.equal(tr.texture_dims.cpu(), want_dims) and torch.equal(tr.texels().cpu(), want_tex)
    stroke = torch.zeros((H, W, 4), device=DEV)
    stroke[24:36, 30:44] = torch.tensor([1.0, 0.0, 1.0, 1.0], device=DEV)
    painted = tr.paint(view, stroke)
    assert tuple(painted.shape) == (want_T, 3) and bool(torch.isfinite(painted).all())
    metrics = tr.evaluate(view, gt)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(metrics.metrics).all())
    path = tmp_path / "selected.npz"
    export_npz(tr, path)
    back = trainer_from_npz(path, DEV)
    assert back.means.shape[0] == tr.means.shape[0] == int(keep.sum()) and back.n_texels == tr.n_texels == want_T
    assert torch.equal(back.texels(), tr.texels()) and torch.equal(back.texture_dims, tr.texture_dims)
    assert torch.equal(back.means.detach(), tr.means.detach()) and torch.equal(back.mappings, tr.mappings)


def test_selection_from_cluster_labels():
    from gstex_amd.cluster import keep_mask
    from gstex_amd.init import _seeded_scene
    from gstex_amd.model import GStexTrainer

    g = torch.Generator().manual_seed(17)
    blobs = [c + 0.03 * torch.randn((150, 3), generator=g) for c in (torch.tensor([-0.8, 0.0, 0.0]),
                                                                     torch.tensor([0.8, 0.1, 0.0]))]
    outliers = (torch.rand((30, 3), generator=g) - 0.5) * 4.0
    means = torch.cat(blobs + [outliers])[torch.randperm(330, generator=g)]
    sc = _seeded_scene(means, torch.rand((330, 3), generator=g), 1, seed=17)
    tr = GStexTrainer(sc, DEV, sh_degree=1, defer_texture=True)
    eps, min_pts = 0.01, 5
    res = tr.cluster(eps, min_pts)
    noise = res.labels == -1
    assert res.n_clusters == 2 and 0 < int(noise.sum()) < 60
    mask = keep_mask(res)
    assert mask.device == res.labels.device and torch.equal(mask, ~noise)
    old_means = tr.means.detach().clone()
    out = tr.select(mask)
    assert out.n_after == int(mask.sum()) == tr.means.shape[0] and out.n_before == 330
    assert torch.equal(tr.means.detach(), old_means[mask])
    again = tr.cluster(eps, min_pts)
    # noise splats are no core's neighbours, so without them every core keeps its neighbours and every border splat
    # its core: the clustering of the selection is the old one, and no splat is noise
    assert int((again.labels == -1).sum()) == 0 and again.n_clusters == 2
    assert torch.equal(again.labels, res.labels[mask])
    one = keep_mask(again, labels=[2])
    out = tr.select(one)
    assert out.n_after == int(one.sum()) and tr.cluster(eps, min_pts).n_clusters == 1
