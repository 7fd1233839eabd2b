// raster_setup_bwd.hip — the raster's setup backward (gstex_raster_setup_bwd): the per-splat partials the raster
// backward (raster_bwd.hip) left -- (pair, quadrant) rows in the deterministic mode, one accumulator row per splat
// otherwise -- summed per splat and chained through the record (raster_chain.h) to the splat parameters' gradients.
#include "gstex_common.h"
#include "gstex_error.h"
#include "raster_chain.h"

using namespace gstex;

namespace {

// ------------------------------------------------------------------------------------------
// setup backward: sum partials per splat, chain to parameters
// ------------------------------------------------------------------------------------------
constexpr int kSetupBwdRows = 8;  // splats summed per 256-thread workgroup (32 lanes each)
#ifndef GSTEX_SUM_SLOTS
#define GSTEX_SUM_SLOTS 8
#endif
constexpr int kSumSlots = GSTEX_SUM_SLOTS;  // slots whose rows one lane group has in flight at once (16: equal; 4: slower)
// Deterministic mode: setup_bwd_sum_kernel, 32 lanes per splat, sums the splat's flagged rows in (slot, quadrant)
// order and writes the 32 sums over the splat's first row (slot offsets[g], quadrant 0), whose values it has already
// read -- no other splat reads that row; then setup_bwd_chain_kernel, one thread per splat, chains the sums to the
// parameters.  (One fused kernel, 40 splats per workgroup, measured 120 vs 102 us in round 2.)
// Capacity mode (n_rows >= 0, GSTEX_BIN_CAPPED): a total offsets[n] above the row capacity means the binning
// left every tile empty and no row was written; both kernels then treat every splat as pair-free (zero gradients)
// instead of addressing rows past the buffers.
// 32 lanes per splat: lane 8 q + m reads float4 m (columns 4m .. 4m+3) of the quadrant-q rows, kSumSlots slots at a
// time, and sums them in slot order; the 4 quadrant sums are then combined (q0 + q1) + (q2 + q3) across lanes.
// Deterministic (fixed order), like the fused kernel's slot-major quadrant-minor order it replaces.
// rs = floats between rows: kPartRow (24) when the backward had no depth / normal / distortion gradient, else
// kPartRowGeo (32).  The sums (32 values, the last 8 zero for 24-value rows) go over the splat's first row; with rs =
// 24 they reach into its second row, which only this splat's lanes read, before (program order) the store.
__global__ __launch_bounds__(256) void setup_bwd_sum_kernel(int n, const int32_t* __restrict__ nth,
                                                           const int32_t* __restrict__ offsets,
                                                           float* __restrict__ partials,
                                                           const uint32_t* __restrict__ row_flags, int rs,
                                                           int64_t n_rows) {
    const int l = threadIdx.x & 31, q = l >> 3, m = l & 7;
    const int g = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = g < n && !(n_rows >= 0 && (int64_t)offsets[n] > n_rows);  // over capacity: no rows exist
    const int cnt = live ? nth[g] : 0;
    const size_t s0 = live ? (size_t)offsets[g] : 0;
    // columns 24.. exist only in 32-value rows (flag 2: backward with depth / normal gradients)
    const uint32_t need = m < kPartRow / 4 ? 0xFFu : 0x02u;
    const float4* rows = reinterpret_cast<const float4*>(partials + s0 * 4 * rs) + q * (rs / 4) + m;
    const uint32_t* fl = row_flags + s0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = 0; e < cnt; e += kSumSlots) {
        uint32_t f[kSumSlots];
#pragma unroll
        for (int u = 0; u < kSumSlots; ++u) f[u] = e + u < cnt ? fl[e + u] : 0u;
        float4 r[kSumSlots];
#pragma unroll
        for (int u = 0; u < kSumSlots; ++u)
            r[u] = (f[u] >> (8 * q)) & need ? rows[(size_t)(e + u) * rs] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < kSumSlots; ++u) {
            if ((f[u] >> (8 * q)) & need) {
                acc.x += r[u].x;
                acc.y += r[u].y;
                acc.z += r[u].z;
                acc.w += r[u].w;
            }
        }
    }
    // (q0 + q1) + (q2 + q3): lane l adds lane l ^ 8, then lane l ^ 16 (inside the 32-lane splat group)
    auto xadd = [](float4 a, int mask) {
        return make_float4(a.x + __shfl_xor(a.x, mask, 32), a.y + __shfl_xor(a.y, mask, 32),
                           a.z + __shfl_xor(a.z, mask, 32), a.w + __shfl_xor(a.w, mask, 32));
    };
    acc = xadd(acc, 8);
    acc = xadd(acc, 16);
    // the sums over the splat's first row, whose values every lane has read above: no other splat reads it
    if (live && cnt > 0 && q == 0)
        reinterpret_cast<float4*>(partials + s0 * 4 * rs)[m] = acc;
}

template <bool FOLD_AABB>
__global__ __launch_bounds__(256) void setup_bwd_chain_kernel(
    int n, const float* __restrict__ means, const float* __restrict__ scales, float glob,
    const float* __restrict__ quats, const float* __restrict__ umap, const float* __restrict__ vmap,
    const int32_t* __restrict__ nth, const int32_t* __restrict__ offsets, const float* __restrict__ partials, int rs,
    bool per_splat, int64_t n_rows, CamArgs cam_args, float* __restrict__ v_means, float* __restrict__ v_scales,
    float* __restrict__ v_quats, float* __restrict__ v_rgbs, float* __restrict__ v_opac, float* __restrict__ v_centers,
    float* __restrict__ v_uv0) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const Camera cam = load_camera(cam_args);
    // deterministic mode over capacity (n_rows >= 0): the binning left every tile empty and no row exists
    const bool over = !per_splat && n_rows >= 0 && (int64_t)offsets[n] > n_rows;
    const int cnt = over ? 0 : nth[g];
    float S[kPartRowGeo];
    if (per_splat) {
        // the backward's (N, rs) accumulator rows (zero for a splat without pairs): all eight 16-B loads issued at
        // once, in bounds (a 24-value row re-reads its last vector), independent of the pair count's load
        const float4* src = reinterpret_cast<const float4*>(partials + (size_t)g * rs);
        const int n4 = rs / 4;
#pragma unroll
        for (int i = 0; i < kPartRowGeo / 4; ++i) {
            const float4 v = src[i < n4 ? i : n4 - 1];
            const bool use = i < n4 && cnt > 0;
            S[4 * i] = use ? v.x : 0.f; S[4 * i + 1] = use ? v.y : 0.f;
            S[4 * i + 2] = use ? v.z : 0.f; S[4 * i + 3] = use ? v.w : 0.f;
        }
    } else if (cnt > 0) {
        // the sums setup_bwd_sum wrote over the splat's first partial row (32 values, the last 8 zero for 24-value
        // rows)
        const float4* src = reinterpret_cast<const float4*>(partials + (size_t)offsets[g] * 4 * rs);
#pragma unroll
        for (int i = 0; i < kPartRowGeo / 4; ++i) {
            const float4 v = src[i];
            S[4 * i] = v.x; S[4 * i + 1] = v.y; S[4 * i + 2] = v.z; S[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kPartRowGeo; ++i) S[i] = 0.f;
    }
    setup_bwd_chain<FOLD_AABB>(g, S, cnt, cam, means, scales, glob, quats, umap, vmap, v_means, v_scales, v_quats,
                               v_rgbs, v_opac, v_centers, v_uv0);
}

}  // namespace

extern "C" int gstex_raster_setup_bwd(const gstex_raster_setup_bwd_args* a, void* stream) {
    GSTEX_REQUIRE(a && a->n >= 0, "gstex_raster_setup_bwd: invalid arguments");
    if (a->n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(a->means && a->scales && a->quats && a->umap && a->vmap && a->num_tiles_hit && a->offsets &&
                      a->partials && a->v_means && a->v_scales && a->v_quats && a->v_rgbs && a->v_opacities &&
                      a->v_centers && a->v_uv0,
                  "gstex_raster_setup_bwd: null pointer");
    GSTEX_REQUIRE(a->row_floats == kPartRow || a->row_floats == kPartRowGeo,
                  "gstex_raster_setup_bwd: row_floats must be %d or %d (got %d)", kPartRow, kPartRowGeo, a->row_floats);
    hipStream_t st = as_stream(stream);
    // no row_flags: the backward accumulated per splat (atomic mode), nothing to sum
    if (a->row_flags)
        setup_bwd_sum_kernel<<<div_up(a->n, kSetupBwdRows), 256, 0, st>>>(a->n, a->num_tiles_hit, a->offsets,
                                                                           a->partials, a->row_flags, a->row_floats,
                                                                           a->n_rows);
#define GSTEX_CHAIN(FOLD)                                                                                      \
    setup_bwd_chain_kernel<FOLD><<<div_up(a->n, 256), 256, 0, st>>>(                                          \
        a->n, a->means, a->scales, a->glob_scale, a->quats, a->umap, a->vmap, a->num_tiles_hit, a->offsets,   \
        a->partials, a->row_floats, a->row_flags == nullptr, a->n_rows, to_device_camera(a->cam), a->v_means, \
        a->v_scales, a->v_quats, a->v_rgbs, a->v_opacities, a->v_centers, a->v_uv0)
    if (!a->fold_aabb) GSTEX_CHAIN(false);
    else GSTEX_CHAIN(true);
#undef GSTEX_CHAIN
    return launch_status("gstex_raster_setup_bwd");
}
