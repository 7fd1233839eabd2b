// raster_edit.hip — the paint path: a screen-space stroke splatted into the texels along the forward's traversal
// (gstex_texture_edit, the viewer's tool; gstex_paint_scatter + gstex_paint_blend, the fused edit of
// GStexTrainer.paint).  Same cull, termination and weights as raster_fwd.hip (the shared functions of
// raster_common.h); global float atomics, no aux and no checkpoints.
#include "raster_common.h"

using namespace gstex;

namespace {

// ------------------------------------------------------------------------------------------
// texture_edit (gstex.py:579-606, viewer paint tool): splat a screen-space RGBA stroke into the
// texel store.  Same front-to-back traversal as the forward (same cull, termination and weights
// w = alpha * T); a pair whose hit depth lies inside the pixel's [depth_lo, depth_hi] window (the
// caller passes the rendered depth +- 1e-2) adds, for each of its 4 bilinear texels with weight b,
//   out[texel] += b * w * (a * r, a * g, a * b, a, 1)
// so out[:, :3] / out[:, 3] is the stroke colour and out[:, 3] / out[:, 4] the blend weight the caller
// forms (gstex.py:602-605).  Viewer path: global float atomics, no LDS staging.
// ------------------------------------------------------------------------------------------
struct EditPixel { float r, g, b, a, lo, hi; };  // one pixel's stroke (straight alpha) and depth window
constexpr EditPixel kNoEdit = {0.f, 0.f, 0.f, 0.f, 1.0f, 0.0f};  // outside the image: an empty window

// One tile's traversal, shared by texture_edit_kernel and paint_scatter_kernel; pixel(pix) supplies the stroke and
// window of pixel pix = y W + x.  SKIP_CLEAR: a pixel whose stroke alpha is exactly 0 adds only the weight channel
// (its other four products are +-0, which leave the sums as they are: four of five atomics fewer on a thin stroke).
template <bool SKIP_CLEAR, typename PixelFn>
__device__ __forceinline__ void edit_tile(const Camera& cam, int tiles_x, int settings, float4* s_rec,
                                          const float4* __restrict__ records, const int2* __restrict__ tile_ranges,
                                          const int32_t* __restrict__ tile_order,
                                          const int32_t* __restrict__ sorted_ids, int n_texels,
                                          float* __restrict__ out, PixelFn pixel) {
    const int tile = tile_order ? tile_order[blockIdx.x] : (int)blockIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x;
    const WaveBlock wb = wave_block(tx, ty, tid);
    const int pxi = wb.px, pyi = wb.py;
    const bool inside = pxi < cam.W && pyi < cam.H;
    const float px = (float)pxi + 0.5f, py = (float)pyi + 0.5f;  // pixel centres (gstex_common.h)
    const bool aa = (settings & GSTEX_SETTING_AA_BLUR) != 0;
    const int2 rng = tile_ranges[tile];
    const EditPixel e = inside ? pixel((size_t)pyi * cam.W + pxi) : kNoEdit;
    const bool colour = !SKIP_CLEAR || e.a != 0.0f;
    float T = 1.0f;
    bool done = !inside;
    for (int b0 = rng.x; b0 < rng.y; b0 += kFwdBatch) {
        if (__syncthreads_count(done ? 1 : 0) == kThreads) break;
        for (int q = tid; q < kFwdBatch * kRecF4; q += kThreads) {
            const int j = q / kRecF4, k = q % kRecF4;
            if (b0 + j < rng.y) s_rec[k * kFwdBatch + j] = records[(size_t)sorted_ids[b0 + j] * kRecF4 + k];
        }
        __syncthreads();
        const int nb = min(kFwdBatch, rng.y - b0);
        for (int j = 0; j < nb && !done; ++j) {
            if (!wave_may_hit<kFwdBatch>(s_rec, j, wb.wx0, wb.wx1, wb.wy0, wb.wy1, aa)) continue;
            const Rec r = read_rec<kFwdBatch>(s_rec, j);
            Hit h;
            if (!eval_hit(r, px, py, aa, h)) continue;
            const float test_T = T * (1.0f - h.alpha);
            if (test_T < kTMin) {
                done = true;
                break;
            }
            const float w = h.alpha * T;
            if (r.h * r.w > 0 && r.off + r.h * r.w <= n_texels && h.z >= e.lo && h.z <= e.hi) {
                float tu, tv;
                tex_coords(r, h.u, h.v, tu, tv);
                const Bilerp bl = bilerp_xy(tu, tv, r.h, r.w, r.hm1, r.wm1);
                const float wc[4] = {(1.0f - bl.ax) * (1.0f - bl.ay), (1.0f - bl.ax) * bl.ay,
                                     bl.ax * (1.0f - bl.ay), bl.ax * bl.ay};
                const int tc[4] = {bl.i0 * r.w + bl.j0, bl.i0 * r.w + bl.j1, bl.i1 * r.w + bl.j0, bl.i1 * r.w + bl.j1};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float bw = wc[k] * w, baw = bw * e.a;
                    float* o = out + (size_t)(r.off + tc[k]) * 5;
                    if (colour) {
                        atomicAdd(o + 0, baw * e.r);
                        atomicAdd(o + 1, baw * e.g);
                        atomicAdd(o + 2, baw * e.b);
                        atomicAdd(o + 3, baw);
                    }
                    atomicAdd(o + 4, bw);
                }
            }
            T = test_T;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void texture_edit_kernel(
    CamArgs cam_args, int tiles_x, int settings, const float4* __restrict__ records,
    const int2* __restrict__ tile_ranges, const int32_t* __restrict__ tile_order, const int32_t* __restrict__ sorted_ids,
    const float* __restrict__ edit_rgb, const float* __restrict__ edit_a, const float* __restrict__ depth_lo,
    const float* __restrict__ depth_hi, int n_texels, float* __restrict__ out) {
    const Camera cam = load_camera(cam_args);
    __shared__ float4 s_rec[kRecF4 * kFwdBatch];
    edit_tile<false>(cam, tiles_x, settings, s_rec, records, tile_ranges, tile_order, sorted_ids, n_texels, out,
                     [&](size_t pix) {
                         return EditPixel{edit_rgb[3 * pix], edit_rgb[3 * pix + 1], edit_rgb[3 * pix + 2], edit_a[pix],
                                          depth_lo[pix], depth_hi[pix]};
                     });
}

// ------------------------------------------------------------------------------------------
// paint (GStexModel.draw_from_view, gstex.py:489-606, as two kernels; gstex_hip.h gstex_paint_scatter / _blend)
// ------------------------------------------------------------------------------------------
// The scatter: texture_edit_kernel's traversal (edit_tile) on the records and tile lists of the depth render, with
// the depth window formed here from the rendered depth (lo = depth - eps, hi = depth + eps: one rounded fp32
// operation each, the bits of the caller's depth_output -+ 1e-2 in torch), the stroke read as one RGBA image (U8:
// (float)v / 255.0f, a true division) and a transparent pixel adding its weight channel only.
template <bool U8>
__global__ __launch_bounds__(kThreads) void paint_scatter_kernel(
    CamArgs cam_args, int tiles_x, int settings, const float4* __restrict__ records,
    const int2* __restrict__ tile_ranges, const int32_t* __restrict__ tile_order, const int32_t* __restrict__ sorted_ids,
    const void* __restrict__ stroke, const float* __restrict__ depth, float eps, int n_texels,
    float* __restrict__ acc) {
    const Camera cam = load_camera(cam_args);
    __shared__ float4 s_rec[kRecF4 * kFwdBatch];
    edit_tile<true>(cam, tiles_x, settings, s_rec, records, tile_ranges, tile_order, sorted_ids, n_texels, acc,
                    [&](size_t pix) {
                        float4 c;
                        if constexpr (U8) {
                            const uchar4 q = static_cast<const uchar4*>(stroke)[pix];
                            c = float4{(float)q.x / 255.0f, (float)q.y / 255.0f, (float)q.z / 255.0f,
                                       (float)q.w / 255.0f};
                        } else {
                            c = static_cast<const float4*>(stroke)[pix];
                        }
                        const float d = depth[pix];
                        return EditPixel{c.x, c.y, c.z, c.w, d - eps, d + eps};
                    });
}

// The blend of gstex.py:603-605, one thread per texel, on the scatter's accumulator row (c0, c1, c2, a, wt); every
// line one rounded fp32 operation:
//   weight = a / (wt + 1e-6f),  rgb_k = c_k / (a + 1e-6f),  out_k = rgb_k * weight + cur_k * (1 - weight)
// written in place where a > 0 (a == 0: the reference's expression returns cur, nothing is written).  cur is the
// stored texel, or with a (scale, shift) other than (1, 0) the raster's texel value fma(stored, scale, shift) (the
// fused multiply-add of tex_accum), and the write is (out - shift) / scale: the kernel then edits the SH-DC store
// itself.  Rows that were not all zero are stored back as zeros: the workspace leaves the call zeroed again.
constexpr int kBlendBlock = 256;
__global__ __launch_bounds__(kBlendBlock) void paint_blend_kernel(int n_texels, float* __restrict__ acc,
                                                                  float* __restrict__ texture, float scale,
                                                                  float shift, bool identity) {
    const int t = blockIdx.x * kBlendBlock + threadIdx.x;
    if (t >= n_texels) return;
    float* row = acc + (size_t)t * 5;
    const float c[3] = {row[0], row[1], row[2]};
    const float a = row[3], wt = row[4];
    if (c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f && a == 0.0f && wt == 0.0f) return;
#pragma unroll
    for (int k = 0; k < 5; ++k) row[k] = 0.0f;
    if (!(a > 0.0f)) return;
    const float weight = a / (wt + 1e-6f);
    const float ia = a + 1e-6f, keep = 1.0f - weight;
    float* tx = texture + (size_t)t * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float cur = identity ? tx[k] : __builtin_fmaf(tx[k], scale, shift);
        const float rgb = c[k] / ia;
        const float o = rgb * weight + cur * keep;
        tx[k] = identity ? o : (o - shift) / scale;
    }
}

}  // namespace

extern "C" int gstex_texture_edit(const gstex_camera* cam, int32_t settings, const float* records,
                                  const int32_t* tile_ranges, const int32_t* tile_order, const int32_t* sorted_ids,
                                  const float* edit_rgb, const float* edit_alpha, const float* depth_lo,
                                  const float* depth_hi, int64_t n_texels, float* out, void* stream) {
    GSTEX_CHECK(check_camera("gstex_texture_edit", cam));
    GSTEX_CHECK(check_settings("texture_edit", settings, kEditSettings));
    GSTEX_REQUIRE(n_texels >= 0, "gstex_texture_edit: n_texels < 0");
    GSTEX_REQUIRE(tile_ranges && edit_rgb && edit_alpha && depth_lo && depth_hi && (out || n_texels == 0),
                  "gstex_texture_edit: null pointer");
    const int tiles_x = (cam->W + kTile - 1) / kTile, tiles_y = (cam->H + kTile - 1) / kTile;
    CamArgs dc = to_device_camera(*cam);
    texture_edit_kernel<<<tiles_x * tiles_y, kThreads, 0, as_stream(stream)>>>(
        dc, tiles_x, settings, (const float4*)records, (const int2*)tile_ranges, tile_order, sorted_ids, edit_rgb,
        edit_alpha, depth_lo, depth_hi, (int)n_texels, out);
    return launch_status("gstex_texture_edit");
}

extern "C" int gstex_paint_scatter(const gstex_paint_scatter_args* a, void* stream) {
    GSTEX_REQUIRE(a, "gstex_paint_scatter: null args");
    const gstex_camera* cam = &a->cam;
    GSTEX_CHECK(check_camera("gstex_paint_scatter", cam));
    GSTEX_CHECK(check_settings("gstex_paint_scatter", a->settings, kEditSettings));
    GSTEX_CHECK(check_n_texels("gstex_paint_scatter", a->n_texels, 1));
    GSTEX_REQUIRE(a->eps >= 0.0f && a->eps <= FLT_MAX, "gstex_paint_scatter: eps must be a finite value >= 0");
    GSTEX_REQUIRE(a->stroke_dtype == GSTEX_GT_F32 || a->stroke_dtype == GSTEX_GT_U8,
                  "gstex_paint_scatter: unknown stroke_dtype %d", a->stroke_dtype);
    GSTEX_REQUIRE(a->tile_ranges && a->stroke && a->depth && (a->acc || a->n_texels == 0),
                  "gstex_paint_scatter: null pointer");
    // one RGBA pixel is one load
    GSTEX_REQUIRE((reinterpret_cast<uintptr_t>(a->stroke) & (a->stroke_dtype == GSTEX_GT_U8 ? 3 : 15)) == 0,
                  "gstex_paint_scatter: stroke must be 4-byte (U8) or 16-byte (F32) aligned");
    const int tiles_x = (cam->W + kTile - 1) / kTile, tiles_y = (cam->H + kTile - 1) / kTile;
    const CamArgs dc = to_device_camera(*cam);
    hipStream_t st = as_stream(stream);
#define GSTEX_SCATTER(U8)                                                                                       \
    paint_scatter_kernel<U8><<<tiles_x * tiles_y, kThreads, 0, st>>>(                                           \
        dc, tiles_x, a->settings, (const float4*)a->records, (const int2*)a->tile_ranges, a->tile_order,        \
        a->sorted_ids, a->stroke, a->depth, a->eps, (int)a->n_texels, a->acc)
    if (a->stroke_dtype == GSTEX_GT_U8) GSTEX_SCATTER(true);
    else GSTEX_SCATTER(false);
#undef GSTEX_SCATTER
    return launch_status("gstex_paint_scatter");
}

extern "C" int gstex_paint_blend(const gstex_paint_blend_args* a, void* stream) {
    GSTEX_REQUIRE(a, "gstex_paint_blend: null args");
    GSTEX_REQUIRE(a->n_texels >= 0 && a->n_texels < (int64_t)INT32_MAX,
                  "gstex_paint_blend: n_texels out of range (%lld)", (long long)a->n_texels);
    GSTEX_REQUIRE(a->scale != 0.0f && fabsf(a->scale) <= FLT_MAX && fabsf(a->shift) <= FLT_MAX,
                  "gstex_paint_blend: scale must be finite and not 0, shift finite");
    if (a->n_texels == 0) return GSTEX_OK;
    GSTEX_REQUIRE(a->acc && a->texture, "gstex_paint_blend: null pointer");
    paint_blend_kernel<<<div_up((int)a->n_texels, kBlendBlock), kBlendBlock, 0, as_stream(stream)>>>(
        (int)a->n_texels, a->acc, a->texture, a->scale, a->shift, a->scale == 1.0f && a->shift == 0.0f);
    return launch_status("gstex_paint_blend");
}
