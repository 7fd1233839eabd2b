"""Painting on the GPU: gstex_paint_scatter against the CPU oracle and against gstex_texture_edit, gstex_paint_blend
bit for bit against its torch twin, and GStexTrainer.paint / edit_texture / bake_edits against the reference's
draw_from_view call sequence replayed through gstex_cuda."""
import dataclasses
import functools

import pytest
import torch

from helpers import make_case
from oracle import raster as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SH_C0 = 0.28209479177387814
EDIT = 1 << 13


def dv(t):
    return t.detach().to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def scatter_bound(ref):
    """The scatter tolerance of test_texture_edit_matches_oracle, per channel: float atomics differ from the exact
    sum by their summation order only."""
    return 1e-5 * ref.abs().max(0).values + 1e-9


def strokes(H, W, seed):
    """A random stroke with about 70 % of its pixels at alpha exactly 0, as float32 and as a uint8 canvas."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(H, W, 3, generator=g)
    a = (torch.rand(H, W, generator=g) > 0.7).float() * torch.rand(H, W, generator=g)
    f32 = torch.cat([rgb, a[..., None]], -1)
    canvas = torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8)
    canvas[..., 3] = torch.where(a > 0, canvas[..., 3].clamp(min=1), torch.zeros_like(canvas[..., 3]))
    return f32, canvas


@functools.lru_cache(maxsize=None)
def oracle_case(seed, H=64, W=80, n=400, n_texels=30000, opacity=0.1, aniso=1.0):
    """One seeded case with the oracle's depth and the oracle's edit sums for both strokes (computed once).  aniso: the
    scene through helpers.anisotropic (non-square texel blocks)."""
    case = make_case(n=n, n_texels=n_texels, H=H, W=W, seed=seed, settings=EDIT, opacity=opacity, aniso=aniso)
    inp = case.inp
    depth = O.rasterize(inp)[0]["depth"]  # the caller's depth render (gstex.py:567)
    f32, canvas = strokes(H, W, seed)
    lo, hi = depth - 1e-2, depth + 1e-2
    ref_f32 = O.texture_edit(inp, f32[..., :3], f32[..., 3], lo, hi)
    c = canvas.float() / 255.0  # numpy's and torch's true division: update_edit_texture's canvas / 255 (gstex.py:432)
    ref_u8 = O.texture_edit(inp, c[..., :3], c[..., 3], lo, hi)
    return case, depth, f32, canvas, ref_f32, ref_u8


def gpu_geometry(case, hp=False):
    """The binning and the records of a case on the device (records with or without the near-edge-on marks)."""
    from gstex_amd import ops

    inp, v = case.inp, case.view
    H, W = inp.cam.H, inp.cam.W
    centers, nth = dv(inp.centers), dv(case.nth)
    bins = ops.bin_gaussians(centers, dv(inp.extents), dv(inp.depths), nth, H, W)
    cam = (dv(v.viewmat), dv(v.c2w), v.fx, v.fy, v.cx, v.cy, H, W)
    records, _ = ops.depth_render(dv(inp.texture_dims), centers, nth, dv(inp.opacities), dv(inp.means),
                                  dv(inp.scales), 1.0, dv(inp.quats), dv(inp.uv0), dv(inp.umap), dv(inp.vmap), *cam,
                                  inp.settings, bins, render=False, hp=hp)
    return bins, records, cam


def gpu_scatter(case, stroke, depth, hp=False, acc=None):
    from gstex_amd import ops

    bins, records, cam = gpu_geometry(case, hp)
    T = case.inp.texture.shape[0]
    if acc is None:
        acc = torch.zeros((T, 5), device=DEV)
    return ops.paint_scatter(acc, dv(stroke), dv(depth), records, bins.tile_ranges, bins.order, bins.sorted_ids,
                             *cam, T, settings=EDIT, eps=1e-2)


def assert_same_sums(got, ref, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape
    assert float(ref[:, 4].sum()) > 1.0, "the stroke must reach texels"
    assert torch.equal(ref[:, 4] > 0, got[:, 4] > 0), f"{what}: the same texels are painted (integer decisions)"
    err, bound = (got - ref).abs().max(0).values, scatter_bound(ref)
    print(f"[paint] {what}: max error per channel {err.tolist()} bound {bound.tolist()}")
    assert bool((err <= bound).all()), (what, err, bound)


# ---------------------------------------------------------------- 1. scatter against the oracle
@pytest.mark.parametrize("variant", ["f32", "u8", "hp_records"])
@pytest.mark.parametrize("seed", [31, 32])
def test_scatter_matches_oracle(seed, variant):
    case, depth, f32, canvas, ref_f32, ref_u8 = oracle_case(seed)
    assert 0.6 < float((f32[..., 3] == 0).float().mean()) < 0.8
    if variant == "u8":
        got, ref = gpu_scatter(case, canvas, depth), ref_u8
    else:
        got, ref = gpu_scatter(case, f32, depth, hp=variant == "hp_records"), ref_f32
    assert_same_sums(got, ref, f"seed {seed} {variant} vs oracle")
    # a transparent pixel adds the weight channel only: texels reached by nothing else have wt > 0 and a == 0
    assert int(((ref[:, 4] > 0) & (ref[:, 3] == 0)).sum()) > 0
    assert torch.equal(got.cpu()[:, 3] > 0, ref[:, 3] > 0)


def test_scatter_matches_oracle_anisotropic():
    """s_u / s_v within [1/10, 10], h x w blocks up to 10 : 1: the scatter's texel addressing (off + i w + j, x against
    h, y against w) where h != w.  Random opacities (opacity=None): at the other cases' 0.1 this small scene's depth
    render lies within 1e-2 of almost no pair's depth and the stroke reaches 24 texels (total weight 0.16); here 574.
    One seed tried."""
    case, depth, f32, _, ref, _ = oracle_case(33, H=48, W=48, n=150, n_texels=6000, opacity=None, aniso=10.0)
    h, w = case.inp.texture_dims[:, 0].long(), case.inp.texture_dims[:, 1].long()
    seen = torch.zeros(h.numel(), dtype=torch.bool)
    inp = case.inp
    seen[torch.as_tensor(O.bin_and_sort(inp.centers, inp.extents, inp.depths, 48, 48)[2]).long()] = True
    assert int((h != w).sum()) * 2 >= h.numel() and bool((seen & ((h > 2 * w) | (w > 2 * h))).any())
    painted = ref[:, 4] > 0  # the stroke reaches texels of blocks beyond 2 : 1
    ids = torch.repeat_interleave(torch.arange(h.numel()), h * w)
    assert bool((painted & ((h > 2 * w) | (w > 2 * h))[ids]).any())
    assert_same_sums(gpu_scatter(case, f32, depth), ref, "anisotropic seed 33 f32 vs oracle")


def test_hp_marks_do_not_change_the_scatter_decisions():
    """Records with and without the near-edge-on marks differ only in the sign bit of the opacity word, and the
    traversal reads its magnitude: the same painted texels (the sums differ by atomic order alone)."""
    case, depth, f32, *_ = oracle_case(31)
    _, plain, _ = gpu_geometry(case, hp=False)
    _, marked, _ = gpu_geometry(case, hp=True)
    diff = bits(plain) ^ bits(marked)
    assert int((diff & 0x7FFFFFFF).count_nonzero()) == 0, "only sign bits may differ"


# ---------------------------------------------------------------- 2. scatter against gstex_texture_edit
@pytest.mark.parametrize("seed", [31, 32])
def test_scatter_matches_texture_edit_kernel(seed):
    import gstex_cuda

    case, depth, f32, *_ = oracle_case(seed)
    inp, v = case.inp, case.view
    H, W = inp.cam.H, inp.cam.W
    d = dv(depth)
    n = inp.means.shape[0]
    ref = gstex_cuda.texture_edit(
        (n, 1, 5), dv(inp.texture_dims), dv(f32[..., :3]), dv(f32[..., 3:]), d - 1e-2, d + 1e-2, dv(inp.centers),
        dv(inp.extents), dv(inp.depths), dv(case.nth), dv(inp.opacities), dv(inp.means), dv(inp.scales), 1.0,
        dv(inp.quats), dv(inp.uv0), dv(inp.umap), dv(inp.vmap), dv(v.viewmat), dv(v.c2w), v.fx, v.fy, v.cx, v.cy,
        H, W, 16, EDIT, background=torch.zeros(3, device=DEV))
    assert_same_sums(gpu_scatter(case, f32, depth), ref, f"seed {seed} vs gstex_texture_edit")


# ---------------------------------------------------------------- 3. blend
@pytest.mark.parametrize("transform", [(1.0, 0.0), (SH_C0, 0.5)])
def test_blend_is_bitwise_its_torch_twin(transform):
    from gstex_amd import ops

    case, depth, f32, _, ref_f32, _ = oracle_case(31)
    T = case.inp.texture.shape[0]
    acc = gpu_scatter(case, f32, depth)
    sums = acc.clone()
    g = torch.Generator().manual_seed(7)
    store = torch.randn(T + 5, 3, generator=g).to(DEV)  # (five rows past n_texels: a capacity store)
    if transform == (1.0, 0.0):
        store = store * SH_C0 + 0.5
    expect = ops.paint_blend_eager(sums, store, transform)
    before = store.clone()
    out = ops.paint_blend(acc, store, T, transform)
    assert out.data_ptr() == store.data_ptr()
    assert torch.equal(bits(out), bits(expect)), "paint_blend is bit for bit paint_blend_eager"
    painted = sums[:, 3] > 0
    assert 0 < int(painted.sum()) < T
    keep = torch.cat([~painted, torch.ones(5, dtype=torch.bool, device=DEV)])
    assert torch.equal(bits(out[keep]), bits(before[keep])), "texels with a == 0 keep their bits"
    assert not torch.equal(out[:T][painted], before[:T][painted])
    assert int(bits(acc).count_nonzero()) == 0, "the accumulator is all zero afterwards"
    # a second scatter into the same workspace reproduces a fresh-workspace run
    again = gpu_scatter(case, f32, depth, acc=acc)
    assert again.data_ptr() == acc.data_ptr()
    assert_same_sums(again, sums, "second scatter into the blended workspace vs a fresh workspace")
    ops.paint_blend(acc, store, T, transform)
    assert int(bits(acc).count_nonzero()) == 0


# ---------------------------------------------------------------- trainer-level helpers
def small_trainer(n=400, n_texels=30000, seed=11, opacity=None, dims_1x1=False, **kw):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene

    sc = make_scene(n, n_texels, seed=seed, opacity=opacity)
    if dims_1x1:  # every splat a 1x1 block: the four bilinear corners are one texel
        dims = torch.stack([torch.ones(n), torch.ones(n), torch.arange(n)], -1).to(torch.int32)
        g = torch.Generator().manual_seed(seed)
        sc = dataclasses.replace(sc, texture_dims=dims, texture=torch.rand((n, 3), generator=g))
    return GStexTrainer(sc, DEV, **kw)


def solid_stroke(H, W, colour=(1.0, 0.0, 1.0), box=None, alpha=1.0):
    """A filled box (y0, y1, x0, x1) of one colour, transparent elsewhere."""
    s = torch.zeros(H, W, 4)
    y0, y1, x0, x1 = box if box is not None else (H // 4, 3 * H // 4, W // 4, 3 * W // 4)
    s[y0:y1, x0:x1, :3] = torch.tensor(colour)
    s[y0:y1, x0:x1, 3] = alpha
    return s.to(DEV)


def geometry(tr, view):
    """The activations and preprocessing of the trainer's renders (eval_render's)."""
    from gstex_amd import ops
    from gstex_amd.activations import activate

    quats, scales, opacities, uv0, umap, vmap, _ = activate(tr.means, tr.quats, tr.scales, tr.opacities, tr.mappings,
                                                            view.campos)
    intr = (view.fx, view.fy, view.cx, view.cy)
    _, depths = ops.project_points(tr.means, view.viewmat, intr)
    centers, extents = ops.get_aabb_2d(tr.means, scales, 1, quats, view.viewmat, intr)
    nth = ops.get_num_tiles_hit_2d(centers, extents, view.H, view.W, 16)
    return dict(quats=quats, scales=scales, opacities=opacities, uv0=uv0, umap=umap, vmap=vmap, depths=depths,
                centers=centers, extents=extents, nth=nth)


@torch.no_grad()
def reference_draw(tr, view, cur_texture, change_img):
    """draw_from_view (gstex.py:489-606), its exact call sequence through gstex_cuda: texture_gaussians -> +-1e-2 ->
    texture_edit -> the three-line blend.  Returns (updated texture, the (T, 5) sums, the depth)."""
    import gstex_cuda

    g = geometry(tr, view)
    n = tr.means.shape[0]
    means = tr.means.detach()
    cam = (view.viewmat, view.c2w, view.fx, view.fy, view.cx, view.cy, view.H, view.W, 16)
    outputs = gstex_cuda.texture_gaussians(
        (n, 1, 3), tr.texture_dims, g["centers"], g["extents"], g["depths"], g["nth"], torch.sigmoid(means),
        g["opacities"], means, g["scales"], 1, g["quats"], g["uv0"], g["umap"], g["vmap"], cur_texture, *cam,
        tr.settings, background=torch.zeros(3, device=DEV))
    depth_output = outputs[1]
    depth_lower = depth_output - 1e-2
    depth_upper = depth_output + 1e-2
    updated = gstex_cuda.texture_edit(
        (n, 1, 5), tr.texture_dims, change_img[:, :, :3], change_img[:, :, 3:], depth_lower, depth_upper,
        g["centers"], g["extents"], g["depths"], g["nth"], g["opacities"], means, g["scales"], 1, g["quats"],
        g["uv0"], g["umap"], g["vmap"], *cam, EDIT, background=torch.zeros(3, device=DEV))
    sums = updated
    weight = updated[:, 3:4] / (updated[:, 4:] + 1e-6)
    edit_rgb_texture = updated[:, :3] / (updated[:, 3:4] + 1e-6)
    updated = edit_rgb_texture * weight + cur_texture * (1 - weight)
    return updated, sums, depth_output


def blend_bound(sums, cur):
    """Per texel and channel, in fp64: the scatter tolerance d on each of (c, a, wt) -- both sides are float-atomic sums
    within d of the exact sum, so they are within 2 d of each other -- propagated through the partial derivatives of
    out = c / (a + e) * a / (wt + e) + cur * (1 - a / (wt + e)), plus the blend's own fp32 roundings (seven operations
    on values of magnitude <= max(1, |out|, |cur|), half an ulp each)."""
    s, cur = sums.double().cpu(), cur.double().cpu()
    e = float(torch.tensor(1e-6, dtype=torch.float32))
    d = 2 * scatter_bound(s)
    c, a, wt = s[:, :3], s[:, 3:4], s[:, 4:5]
    W, rgb = a / (wt + e), c / (a + e)
    d_c = (W / (a + e)).abs()
    d_a = (-(rgb / (a + e)) * W + (rgb - cur) / (wt + e)).abs()
    d_wt = ((rgb - cur) * a / (wt + e) ** 2).abs()
    out = rgb * W + cur * (1 - W)
    rounding = 7 * 2.0 ** -24 * torch.maximum(torch.ones_like(out), torch.maximum(out.abs(), cur.abs()))
    return d_c * d[:3] + d_a * d[3] + d_wt * d[4] + rounding


def capture_sums(fn):
    """Run fn() with ops.paint_blend wrapped: -> (fn's result, the accumulators each blend was handed)."""
    from gstex_amd import ops

    real, seen = ops.paint_blend, []

    def wrapped(acc, *a, **kw):
        seen.append(acc.clone())
        return real(acc, *a, **kw)

    ops.paint_blend = wrapped
    try:
        return fn(), seen
    finally:
        ops.paint_blend = real


def assert_paint_matches_reference(tr, view, stroke_f32, stroke=None, what=""):
    """trainer.paint of `stroke` (default: stroke_f32) against the replayed reference on stroke_f32."""
    base = (tr.texture_dc.detach()[:tr.n_texels] * SH_C0 + 0.5).contiguous()
    ref, sums, _ = reference_draw(tr, view, base.clone(), stroke_f32)
    tex = base.clone()
    got, (acc,) = capture_sums(lambda: tr.paint(view, stroke_f32 if stroke is None else stroke, tex))
    assert got.data_ptr() == tex.data_ptr(), "the texture is edited in place and returned"
    # the depth is the same kernel's bits on both sides: the same texels are painted, the same sums
    assert_same_sums(acc, sums, f"{what}: trainer.paint's sums vs texture_edit's")
    assert torch.equal(acc[:, 3] > 0, sums[:, 3] > 0)
    painted = (sums[:, 3] > 0).cpu()
    assert not bool(((bits(got) != bits(base)).any(-1).cpu() & ~painted).any()), "an unpainted texel changed"
    err = (got.double().cpu() - ref.double().cpu()).abs()
    bound = blend_bound(sums, base)
    print(f"[paint] {what}: {int(painted.sum())} texels painted, largest bound {float(bound[painted].max()):.3e}, "
          f"median bound {float(bound[painted].median()):.3e}, largest error {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    assert int(bits(tr._paint_acc).count_nonzero()) == 0, "the workspace is left all zero"
    return got


# ---------------------------------------------------------------- 4. trainer.paint against draw_from_view
def test_trainer_paint_matches_replayed_draw_from_view():
    from gstex_amd.scene import sphere_view

    tr = small_trainer()
    view = sphere_view(1, 64, 80).to(DEV)
    f32, canvas = strokes(64, 80, 3)
    assert_paint_matches_reference(tr, view, f32.to(DEV), what="float32 stroke")
    c = (canvas.float() / 255.0).to(DEV)
    assert_paint_matches_reference(tr, view, c, stroke=canvas.to(DEV), what="uint8 canvas")
    # depth=: the given map replaces the depth render (here the reference's own render: the same sums)
    base = (tr.texture_dc.detach()[:tr.n_texels] * SH_C0 + 0.5).contiguous()
    _, sums, depth_output = reference_draw(tr, view, base, f32.to(DEV))
    _, (acc,) = capture_sums(lambda: tr.paint(view, f32.to(DEV), base.clone(), depth=depth_output))
    assert_same_sums(acc, sums, "depth passed in")
    far, (acc,) = capture_sums(lambda: tr.paint(view, f32.to(DEV), base.clone(), depth=depth_output + 1e6))
    assert int(bits(acc).count_nonzero()) == 0 and torch.equal(bits(far), bits(base)), "a window behind every splat"
    # texture=None: a fresh SH2RGB(texture_dc), the same result
    base = (tr.texture_dc.detach()[:tr.n_texels] * SH_C0 + 0.5).contiguous()
    bound = blend_bound(reference_draw(tr, view, base, f32.to(DEV))[1], base)
    a, b = tr.paint(view, f32.to(DEV)), tr.paint(view, f32.to(DEV), base.clone())
    assert a.shape == (tr.n_texels, 3) and a.data_ptr() != tr.texture_dc.data_ptr()
    assert bool(((a - b).abs().double().cpu() <= bound).all())


# ---------------------------------------------------------------- 5. replay, undo, bake, eval_render
def training_state(tr):
    st = {f"param {k}": p.detach().clone() for k, ps in tr.param_groups().items() for p in ps}
    st.update({f"grad {k}": (None if p.grad is None else p.grad.detach().clone())
               for k, ps in tr.param_groups().items() for p in ps})
    for p, s in tr.optimizer.state.items():
        for k, v in s.items():
            st[f"adam {id(p)} {k}"] = v.detach().clone() if isinstance(v, torch.Tensor) else v
    st["step"] = tr.step
    st["texel_grad"] = tr.texel_grad.state()
    st["sink"] = None if tr.texture_grad_sink is None else tr.texture_grad_sink.detach().clone()
    return st


def assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(bits(a[k]) if a[k].dtype == torch.float32 else a[k],
                               bits(b[k]) if b[k].dtype == torch.float32 else b[k]), k
        else:
            assert a[k] == b[k], k


def test_replay_undo_bake_and_eval_render():
    from gstex_amd import ops
    from gstex_amd.edit import Edit
    from gstex_amd.scene import sphere_view

    tr = small_trainer()
    H, W = 64, 80
    v1, v2 = sphere_view(1, H, W).to(DEV), sphere_view(3, H, W).to(DEV)
    gt = torch.rand(H, W, 3, device=DEV)
    for _ in range(2):  # two training steps: gradients, Adam moments and a step count exist
        tr.zero_grad()
        tr.forward_backward(v1, gt)
        tr.optimizer_step()
    tr.zero_grad()
    tr.forward_backward(v1, gt)  # gradients of a third step are pending
    tr.wait_texture()
    s1 = solid_stroke(H, W, (1.0, 0.0, 1.0))
    c2 = (solid_stroke(H, W, (0.0, 1.0, 0.0), box=(10, 30, 20, 70), alpha=0.5) * 255).to(torch.uint8)
    e1, e2 = Edit(v1, s1, "one.png"), Edit(v2, c2.cpu(), "two.png")

    before = training_state(tr)
    p1 = tr.paint(v1, s1)
    assert_same_state(before, training_state(tr))  # paint leaves the training state bit-identical
    p12 = tr.paint(v2, c2, p1.clone())
    # (float atomics: two runs of one edit agree within the blend's bound, not bit for bit)
    sums1 = reference_draw(tr, v1, p1.clone(), s1)[1]
    base = (tr.texture_dc.detach()[:tr.n_texels] * SH_C0 + 0.5).contiguous()
    tol1 = blend_bound(sums1, base)
    one = tr.edit_texture([e1])
    assert bool(((one - p1).abs().double().cpu() <= tol1).all()), "edit_texture([e1]) is the first paint"
    both = tr.edit_texture([e1, e2])
    sums2 = reference_draw(tr, v2, p1.clone(), c2.float() / 255.0)[1]
    tol2 = blend_bound(sums2, p1) + tol1  # (the first edit's difference carried through a blend of weight <= 1)
    assert bool(((both - p12).abs().double().cpu() <= tol2).all()), "edit_texture([e1, e2]) is paint twice"
    painted1, painted2 = sums1[:, 3] > 0, sums2[:, 3] > 0
    assert int(painted1.sum()) > 0 and int((painted2 & ~painted1).sum()) > 0, "the second edit paints more texels"
    assert not bool(((bits(one) != bits(base)).any(-1) & ~painted1).any())
    assert not bool(((bits(both) != bits(base)).any(-1) & ~(painted1 | painted2)).any())
    undo = tr.edit_texture([e1, e2][:-1])
    assert bool(((undo - p1).abs().double().cpu() <= tol1).all()), "undo: the replay of edits[:-1]"
    assert not bool(((bits(undo) != bits(base)).any(-1) & ~painted1).any())
    assert_same_state(before, training_state(tr))

    # eval_render shows the stroke: edit_img differs from rgb where painted texels are visible and nowhere else
    out = tr.eval_render(v1, edit_texture=one)
    g = geometry(tr, v1)
    n = tr.means.shape[0]

    def tex_image(texture):
        return ops.texture_gaussians(
            (n, 1, 3), tr.texture_dims, g["centers"], g["extents"], g["depths"], g["nth"], tr.test_colors,
            g["opacities"], tr.means.detach(), g["scales"], 1, g["quats"], g["uv0"], g["umap"], g["vmap"], texture,
            v1.viewmat, v1.c2w, v1.fx, v1.fy, v1.cx, v1.cy, H, W, 16, tr.settings | (1 << 15),
            background=torch.zeros(3, device=DEV))[4]

    sees_paint = (bits(tex_image(one)) != bits(tex_image(base))).any(-1)  # the same call on the two textures
    diff = (out["edit_img"] - out["rgb"]).abs().max(-1).values
    inside = s1[..., 3] > 0
    # where no painted texel is visible the two images differ by rounding alone: rgb reads the texels as
    # fma(texture_dc, C0, 0.5), edit_img the materialised texture_dc * C0 + 0.5 -- texture outputs within 1e-6 (1 + |x|)
    # of each other (test_texture_transform_equals_materialised_sh2rgb), |x| <= 1, then two sums of values <= 2
    # rounded once each (half an ulp of 2: 1.2e-7)
    quiet = 2e-6 + 2 * 1.2e-7
    assert int((~sees_paint & ~inside).sum()) > 0
    assert float(diff[~sees_paint].max()) <= quiet
    assert int((sees_paint & inside).sum()) > 0 and float(diff[sees_paint & inside].max()) > 1e-2
    assert_same_state(before, training_state(tr))

    # bake_edits: exactly the painted texels of the SH-DC store change, and to the edited colours
    dc_before = tr.texture_dc.detach().clone()
    tr.bake_edits([e1])
    dc_after = tr.texture_dc.detach()
    changed_dc = (bits(dc_after) != bits(dc_before)).any(-1)
    assert not bool(changed_dc[tr.n_texels:].any())
    changed_dc = changed_dc[:tr.n_texels]
    assert not bool((changed_dc & ~painted1).any()), "a texel no stroke reached changed"
    # a painted texel moves by weight * |colour - cur|: where that is >= 1e-5 -- a hundred ulps of a value <= 1.5, more
    # in SH-DC units -- its stored bits must change
    e = 1e-6
    weight = sums1[:, 3] / (sums1[:, 4] + e)
    move = weight[:, None] * (sums1[:, :3] / (sums1[:, 3:4] + e) - base).abs()
    must = painted1 & (move.max(-1).values >= 1e-5)
    assert int(must.sum()) > 0 and bool(changed_dc[must].all()), "the painted texels change"
    assert bool(((dc_after[:tr.n_texels] * SH_C0 + 0.5 - one).abs().double().cpu() <= tol1 + 2e-7).all())
    after = training_state(tr)
    after["param texture_dc"] = before["param texture_dc"]
    assert_same_state(before, after)  # Adam moments, gradients and the step are left alone


# ---------------------------------------------------------------- 6. smallest shapes that can go wrong
def test_partial_tiles_and_early_termination():
    """H = 40, W = 56: partial tiles on both edges; opacities U(0.05, 0.95): the early-termination branch runs."""
    from gstex_amd.scene import sphere_view

    tr = small_trainer(n=300, n_texels=20000, seed=12, opacity=None)
    view = sphere_view(2, 40, 56).to(DEV)
    f32, _ = strokes(40, 56, 4)
    assert_paint_matches_reference(tr, view, f32.to(DEV), what="40x56, random opacities")


def test_one_texel_blocks():
    from gstex_amd.scene import sphere_view

    tr = small_trainer(n=300, n_texels=300, seed=13, opacity=None, dims_1x1=True)
    assert tr.n_texels == 300
    view = sphere_view(0, 40, 56).to(DEV)
    got = assert_paint_matches_reference(tr, view, solid_stroke(40, 56, box=(0, 40, 0, 56)), what="1x1 blocks")
    assert got.shape == (300, 3)


def test_transparent_stroke_no_texels_and_no_tiles():
    from gstex_amd.scene import View, look_at, sphere_view

    tr = small_trainer(n=300, n_texels=20000, seed=12)
    view = sphere_view(2, 40, 56).to(DEV)
    base = (tr.texture_dc.detach()[:tr.n_texels] * SH_C0 + 0.5).contiguous()
    # an all-transparent stroke: weights only, no texel changes, the workspace comes back zero
    clear = torch.rand(40, 56, 4, device=DEV)
    clear[..., 3] = 0.0
    got = tr.paint(view, clear, base.clone())
    assert torch.equal(bits(got), bits(base))
    assert tr._paint_acc.shape == (tr.n_texels, 5) and int(bits(tr._paint_acc).count_nonzero()) == 0
    dc = tr.texture_dc.detach().clone()
    tr.bake_edits([(view, clear)])
    assert torch.equal(bits(tr.texture_dc.detach()), bits(dc))
    # a camera looking away from the scene: no tiles, the two kernels are not launched
    away = sphere_view(2, 40, 56)
    pos = away.c2w[:3, 3].double().numpy()
    vm, c2w = look_at(pos, target=2.0 * pos)
    away = View(vm, c2w, away.fx, away.fy, away.cx, away.cy, 40, 56).to(DEV)
    tr._paint_acc = None
    opaque = solid_stroke(40, 56, box=(0, 40, 0, 56))
    tex = base.clone()
    assert tr.paint(away, opaque, tex) is tex and torch.equal(bits(tex), bits(base)) and tr._paint_acc is None
    # T = 0 (2DGS mode)
    tr0 = small_trainer(n=300, n_texels=0, seed=12)
    assert tr0.n_texels == 0
    out = tr0.paint(view, opaque)
    assert out.shape == (0, 3) and tr0._paint_acc is None
    assert tr0.edit_texture([(view, opaque)]).shape == (0, 3)
    tr0.bake_edits([(view, opaque)])
