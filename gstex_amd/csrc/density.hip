// density.hip — adaptive density control (3DGS §5.2 as 2DGS uses it; not in the reference, which disables it).
//
//   gstex_density_accum  one thread per splat, once per training step: the screen-space gradient statistics
//   gstex_density_plan   one thread per splat, once per event: rows[i] in {0, 1, 2} and kind[i]
//   gstex_density_apply  once per event: every per-splat tensor scattered to its rows in source order
//
// Between plan and apply the caller runs gstex_scan_offsets over rows and reads offsets[n] back (the event's only
// synchronisation).  Every operation below is one individually rounded fp32 + - * / sqrt in a fixed order
// (-ffp-contract=off), and every decision compares against thresholds the host formed (no transcendental here), so
// gstex_amd.density's eager twins reproduce all three kernels bit for bit (DESIGN.md "Density control").
#include "gstex_common.h"
#include "gstex_error.h"

using namespace gstex;

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void density_accum_kernel(
    int n, const float* __restrict__ means, const float* __restrict__ v_means, const float* __restrict__ viewmat,
    float fx, float fy, float hw, float hh, const int32_t* __restrict__ num_tiles_hit,
    const float* __restrict__ extents, const float* __restrict__ skip, float* __restrict__ grad_sum,
    float* __restrict__ count, float* __restrict__ max_extent) {
    if (skip && *skip != 0.0f) return;  // an overflowed step (pair-capacity guard): its gradient is not a gradient
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (num_tiles_hit[i] <= 0) return;
    const float* V = viewmat;  // row-major (3, 4), wave-uniform loads
    const float x = means[3 * (size_t)i], y = means[3 * (size_t)i + 1], zw = means[3 * (size_t)i + 2];
    const float gx = v_means[3 * (size_t)i], gy = v_means[3 * (size_t)i + 1], gz = v_means[3 * (size_t)i + 2];
    const float z = ((V[8] * x + V[9] * y) + V[10] * zw) + V[11];
    const float gcx = (V[0] * gx + V[1] * gy) + V[2] * gz;
    const float gcy = (V[4] * gx + V[5] * gy) + V[6] * gz;
    const float ax = ((gcx * z) / fx) * hw;
    const float ay = ((gcy * z) / fy) * hh;
    grad_sum[i] = grad_sum[i] + sqrtf(ax * ax + ay * ay);
    count[i] = count[i] + 1.0f;
    max_extent[i] = fmaxf(max_extent[i], fmaxf(extents[2 * (size_t)i], extents[2 * (size_t)i + 1]));
}

struct PlanArgs {
    int n, size_prune, prune_only;
    float grad_threshold, log_big, logit_faint, max_screen_px, log_world, log_split;
    const float *log_scales, *opac_logits, *grad_sum, *count, *max_extent;
    int32_t *rows, *kind;
};

__global__ __launch_bounds__(kThreads) void density_plan_kernel(const PlanArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const float m = fmaxf(a.log_scales[3 * (size_t)i], a.log_scales[3 * (size_t)i + 1]);
    const float c = a.count[i];
    const bool hot = !a.prune_only && c > 0.0f && a.grad_sum[i] >= a.grad_threshold * c;
    const bool big = m > a.log_big;
    const bool faint = a.opac_logits[i] < a.logit_faint;
    int rows, kind;
    if (faint) {
        rows = 0; kind = GSTEX_DENSITY_PRUNE;
    } else if (hot && big) {
        // the children carry a fresh screen record: only the world-size test applies to them
        const bool child_too_big = a.size_prune && (m - a.log_split) > a.log_world;
        rows = child_too_big ? 0 : 2;
        kind = child_too_big ? GSTEX_DENSITY_PRUNE : GSTEX_DENSITY_SPLIT;
    } else if (a.size_prune && (a.max_extent[i] > a.max_screen_px || m > a.log_world)) {
        rows = 0; kind = GSTEX_DENSITY_PRUNE;
    } else if (hot) {
        rows = 2; kind = GSTEX_DENSITY_CLONE;
    } else {
        rows = 1; kind = GSTEX_DENSITY_KEEP;
    }
    a.rows[i] = rows;
    a.kind[i] = kind;
}

constexpr int kMaxTensors = GSTEX_DENSITY_MAX_TENSORS;

struct ApplyArgs {
    gstex_density_tensor t[kMaxTensors];
    long long block_start[kMaxTensors + 1];  // each block covers kThreads consecutive SOURCE elements of one tensor
    int n_tensors, n;
    long long n_new;
    float log_split;
    const int32_t *rows, *kind, *offsets;
    const float *scales, *quats_n, *noise;
};

// Rotation columns R[c][0], R[c][1] of splat i: gstex_common.h quat_frame on the normalised quaternion.
__device__ __forceinline__ void frame_row(const float* quats_n, size_t i, int c, float& r0, float& r1) {
    const Frame f = quat_frame(quats_n + 4 * i);
    r0 = c == 0 ? f.tu.x : (c == 1 ? f.tu.y : f.tu.z);
    r1 = c == 0 ? f.tv.x : (c == 1 ? f.tv.y : f.tv.z);
}

// One thread per source element (splat i, column c) of one tensor: consecutive lanes read consecutive source words
// and, the rows being laid out in source order, write consecutive words of each output row; a run of kept splats
// is one contiguous span on both sides.
__global__ __launch_bounds__(kThreads) void density_apply_kernel(const ApplyArgs a) {
    const long long b = blockIdx.x;
    int k = 0;
    while (k + 1 < a.n_tensors && a.block_start[k + 1] <= b) ++k;
    const gstex_density_tensor& t = a.t[k];
    const long long e = (b - a.block_start[k]) * kThreads + threadIdx.x;
    const int w = t.width;
    if (e >= (long long)a.n * w) return;
    const int i = (int)(e / w), c = (int)(e - (long long)i * w);
    const int rows = a.rows[i];
    if (rows <= 0) return;
    const long long row0 = a.offsets[i];
    if (rows > 2 || row0 < 0 || row0 + rows > a.n_new) return;  // never past the n_new rows the caller allocated
    const int kind = a.kind[i];
    const float v = t.src[e];
    float out0 = v, out1 = v;
    if (t.role == GSTEX_DENSITY_ROLE_MOMENT) {  // kept rows keep their moments; clone rows and children start at zero
        if (kind == GSTEX_DENSITY_SPLIT) out0 = 0.0f;
        out1 = 0.0f;
    } else if (kind == GSTEX_DENSITY_SPLIT) {
        if (t.role == GSTEX_DENSITY_ROLE_MEANS) {
            float r0, r1;
            frame_row(a.quats_n, (size_t)i, c, r0, r1);
            const float su = a.scales[3 * (size_t)i], sv = a.scales[3 * (size_t)i + 1];
            const float* z = a.noise + 4 * (size_t)i;  // (n, 2, 2): child k's (z_k0, z_k1)
            const float a0 = su * z[0], b0 = sv * z[1], a1 = su * z[2], b1 = sv * z[3];
            out0 = v + ((r0 * a0) + (r1 * b0));
            out1 = v + ((r0 * a1) + (r1 * b1));
        } else if (t.role == GSTEX_DENSITY_ROLE_LOG_SCALES && c < 2) {
            out0 = out1 = v - a.log_split;
        }
    }
    t.dst[row0 * w + c] = out0;
    if (rows == 2) t.dst[(row0 + 1) * w + c] = out1;
}

}  // namespace

extern "C" int gstex_density_accum(int32_t n, const float* means, const float* v_means, const gstex_camera* cam,
                                   const int32_t* num_tiles_hit, const float* extents, const float* skip,
                                   float* grad_sum, float* count, float* max_extent, void* stream) {
    GSTEX_REQUIRE(n >= 0, "gstex_density_accum: n < 0 (got %d)", n);
    GSTEX_REQUIRE(cam, "gstex_density_accum: null camera");
    GSTEX_REQUIRE(cam->H > 0 && cam->W > 0, "gstex_density_accum: invalid image size (H=%d, W=%d)", cam->H, cam->W);
    GSTEX_REQUIRE(finite_f(cam->fx) && finite_f(cam->fy) && cam->fx > 0.0f && cam->fy > 0.0f,
                  "gstex_density_accum: fx, fy must be finite and > 0 (got %g, %g)", (double)cam->fx, (double)cam->fy);
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(means && v_means && cam->viewmat && num_tiles_hit && extents && grad_sum && count && max_extent,
                  "gstex_density_accum: null pointer");
    GSTEX_REQUIRE(aligned(means, 4) && aligned(v_means, 4) && aligned(cam->viewmat, 4) && aligned(num_tiles_hit, 4) &&
                      aligned(extents, 4) && aligned(skip, 4) && aligned(grad_sum, 4) && aligned(count, 4) &&
                      aligned(max_extent, 4),
                  "gstex_density_accum: misaligned pointer (4-byte words)");
    const float hw = 0.5f * (float)cam->W, hh = 0.5f * (float)cam->H;
    density_accum_kernel<<<div_up(n, kThreads), kThreads, 0, as_stream(stream)>>>(
        n, means, v_means, cam->viewmat, cam->fx, cam->fy, hw, hh, num_tiles_hit, extents, skip, grad_sum, count,
        max_extent);
    return launch_status("gstex_density_accum");
}

extern "C" int gstex_density_plan(const gstex_density_plan_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_density_plan: null args");
    const gstex_density_plan_args& p = *args;
    GSTEX_REQUIRE(p.n >= 0, "gstex_density_plan: n < 0 (got %d)", p.n);
    GSTEX_REQUIRE(finite_f(p.grad_threshold) && finite_f(p.log_big) && finite_f(p.logit_faint) &&
                      finite_f(p.max_screen_px) && finite_f(p.log_world) && finite_f(p.log_split),
                  "gstex_density_plan: non-finite threshold");
    GSTEX_REQUIRE(p.grad_threshold >= 0.0f, "gstex_density_plan: grad_threshold < 0 (got %g)",
                  (double)p.grad_threshold);
    if (p.n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.log_scales && p.opac_logits && p.grad_sum && p.count && p.max_extent && p.rows && p.kind,
                  "gstex_density_plan: null pointer");
    GSTEX_REQUIRE(aligned(p.log_scales, 4) && aligned(p.opac_logits, 4) && aligned(p.grad_sum, 4) &&
                      aligned(p.count, 4) && aligned(p.max_extent, 4) && aligned(p.rows, 4) && aligned(p.kind, 4),
                  "gstex_density_plan: misaligned pointer (4-byte words)");
    PlanArgs a;
    a.n = p.n; a.size_prune = p.size_prune ? 1 : 0; a.prune_only = p.prune_only ? 1 : 0;
    a.grad_threshold = p.grad_threshold; a.log_big = p.log_big; a.logit_faint = p.logit_faint;
    a.max_screen_px = p.max_screen_px; a.log_world = p.log_world; a.log_split = p.log_split;
    a.log_scales = p.log_scales; a.opac_logits = p.opac_logits; a.grad_sum = p.grad_sum; a.count = p.count;
    a.max_extent = p.max_extent; a.rows = p.rows; a.kind = p.kind;
    density_plan_kernel<<<div_up(p.n, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_density_plan");
}

extern "C" int gstex_density_apply(const gstex_density_apply_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_density_apply: null args");
    const gstex_density_apply_args& p = *args;
    GSTEX_REQUIRE(p.n >= 0 && p.n_new >= 0 && p.n_new <= 2 * (int64_t)p.n && p.n_new < (1ll << 31),
                  "gstex_density_apply: invalid sizes (n=%d, n_new=%lld)", p.n, (long long)p.n_new);
    GSTEX_REQUIRE(p.n_tensors >= 0 && p.n_tensors <= kMaxTensors,
                  "gstex_density_apply: n_tensors must be in [0, %d] (got %d)", kMaxTensors, p.n_tensors);
    GSTEX_REQUIRE(finite_f(p.log_split), "gstex_density_apply: non-finite log_split");
    GSTEX_REQUIRE(p.n_tensors == 0 || p.tensors, "gstex_density_apply: null tensor table");
    if (p.n == 0 || p.n_new == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.rows && p.kind && p.offsets, "gstex_density_apply: null pointer (rows / kind / offsets)");
    GSTEX_REQUIRE(aligned(p.rows, 4) && aligned(p.kind, 4) && aligned(p.offsets, 4) && aligned(p.scales, 4) &&
                      aligned(p.quats_n, 4) && aligned(p.noise, 4),
                  "gstex_density_apply: misaligned pointer (4-byte words)");
    ApplyArgs a{};
    long long blocks = 0;
    int k = 0;
    for (int i = 0; i < p.n_tensors; ++i) {
        const gstex_density_tensor& t = p.tensors[i];
        GSTEX_REQUIRE(t.width >= 0, "gstex_density_apply: tensor %d has width < 0", i);
        GSTEX_REQUIRE(t.role >= GSTEX_DENSITY_ROLE_COPY && t.role <= GSTEX_DENSITY_ROLE_LOG_SCALES,
                      "gstex_density_apply: tensor %d has an unknown role %d", i, t.role);
        if (t.width == 0) continue;
        GSTEX_REQUIRE(t.src && t.dst, "gstex_density_apply: tensor %d: null pointer", i);
        GSTEX_REQUIRE(aligned(t.src, 4) && aligned(t.dst, 4), "gstex_density_apply: tensor %d: misaligned pointer", i);
        GSTEX_REQUIRE(t.src != t.dst, "gstex_density_apply: tensor %d: src and dst must differ", i);
        GSTEX_REQUIRE(t.role != GSTEX_DENSITY_ROLE_MEANS || (t.width == 3 && p.scales && p.quats_n && p.noise),
                      "gstex_density_apply: tensor %d: the means need width 3 and scales, quats_n and noise", i);
        GSTEX_REQUIRE(t.role != GSTEX_DENSITY_ROLE_LOG_SCALES || t.width >= 2,
                      "gstex_density_apply: tensor %d: the log-scales need width >= 2", i);
        a.t[k] = t;
        a.block_start[k] = blocks;
        blocks += ((long long)p.n * t.width + kThreads - 1) / kThreads;
        ++k;
    }
    if (k == 0) return GSTEX_OK;
    GSTEX_REQUIRE(blocks < (1ll << 31), "gstex_density_apply: too many elements for one launch");
    a.block_start[k] = blocks;
    a.n_tensors = k;
    a.n = p.n;
    a.n_new = p.n_new;
    a.log_split = p.log_split;
    a.rows = p.rows; a.kind = p.kind; a.offsets = p.offsets;
    a.scales = p.scales; a.quats_n = p.quats_n; a.noise = p.noise;
    density_apply_kernel<<<(unsigned)blocks, kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_density_apply");
}
