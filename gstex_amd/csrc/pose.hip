// pose.hip — the camera pose gradient of the raster: dL/d(viewmat), the 12 entries of V = [R|t] (3x4) as free variables
// (gsplat's v_viewmat convention; the caller's autograd carries it to whatever parametrises the pose).
//
// The render depends on V only through the per-splat camera-space vectors (gstex_common.h splat_anchored /
// splat_homography)
//   W0 = R a,  W1 = R b,  W2 = R mu + t,      a = su t_u,  b = sv t_v
// so with dW[r][k] = dL/dWk[r] (what splat_anchored_vjp / splat_homography_vjp form before they apply R^T)
//   dL/dV[r][:3] = sum_splats dW[r][0] a + dW[r][1] b + dW[r][2] mu,      dL/dV[r][3] = sum_splats dW[r][2].
// Excluded, because they do not depend on V: the texture-affine sums (P_AUU..P_AVV: umap / vmap are world-space and
// detached) and the normal sum (P_NRM: the normal is world-space; its orientation sign is a decision).
//
// gstex_raster_viewmat_bwd runs after gstex_raster_setup_bwd on the same buffers: the per-splat sums are still in
// `partials` (accumulator mode: row g; deterministic mode: written over the splat's first row).  It repeats the chain
// of setup_bwd_chain (raster_chain.h) as far as the camera-space stage, in fp64, one thread per splat, and reduces the 12
// values in two deterministic stages: each 256-thread block reduces in fp64 (wave butterfly, then LDS, fixed order)
// into its workspace row; one final block sums the rows in a fixed order.  No atomics: two calls on the same inputs
// give the same bits.
#include "gstex_common.h"
#include "gstex_error.h"

using namespace gstex;

namespace {

constexpr int kPoseBlock = 256;
constexpr int kPoseVals = 12;

// Sum of v over the block's threads, for each of the 12 values, in a fixed order: xor butterfly inside each wave64
// (every lane ends with the wave's sum), then the waves' sums in wave order.  Thread k < 12 returns value k's sum.
__device__ __forceinline__ double pose_block_sum(double (&v)[kPoseVals], double (*s_w)[kPoseVals]) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < kPoseVals; ++k) v[k] = v[k] + __shfl_xor(v[k], o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kPoseVals; ++k) s_w[wave][k] = v[k];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < kPoseVals) {
#pragma unroll
        for (int w = 0; w < kPoseBlock / 64; ++w) r = r + s_w[w][threadIdx.x];
    }
    return r;
}

// dL/d(AABB centre) -> dL/d(homography rows), aabb_centre_vjp (gstex_common.h) in fp64 with the centre re-evaluated in
// fp64: c = (9 (T.x Tw.x + T.y Tw.y) - T.z Tw.z) / d for T = Tu (x) and Tv (y).
__device__ __forceinline__ void aabb_centre_vjp_d(const HomogT<double>& h, double gcx, double gcy, d3& dTu, d3& dTv,
                                                  d3& dTw) {
    const d3 Tu = h.Tu, Tv = h.Tv, Tw = h.Tw;
    const double c2 = (double)kCutoff2;
    const double d = (c2 * (Tw.x * Tw.x) + c2 * (Tw.y * Tw.y)) - Tw.z * Tw.z;
    const double invd = 1.0 / d;
    const double cx = ((c2 * (Tu.x * Tw.x) + c2 * (Tu.y * Tw.y)) - Tu.z * Tw.z) * invd;
    const double cy = ((c2 * (Tv.x * Tw.x) + c2 * (Tv.y * Tw.y)) - Tv.z * Tw.z) * invd;
    const d3 n = d3{c2 * Tw.x, c2 * Tw.y, -Tw.z};
    dTu = scale3(n, gcx * invd);
    dTv = scale3(n, gcy * invd);
    const d3 dd = scale3(n, 2.0);
    dTw = add3(scale3(add3(d3{c2 * Tu.x, c2 * Tu.y, -Tu.z}, scale3(dd, -cx)), gcx * invd),
               scale3(add3(d3{c2 * Tv.x, c2 * Tv.y, -Tv.z}, scale3(dd, -cy)), gcy * invd));
}

// RASTER: the rows' sums are chained (partials given); else centre-only (the viewmat gradient of gstex_aabb_2d).
// centre gradient: RASTER ? (fold ? the rows' P_XY sums : none) : v_centers.
template <bool RASTER>
__global__ __launch_bounds__(kPoseBlock) void viewmat_bwd_kernel(
    int n, const float* __restrict__ means, const float* __restrict__ scales, float glob,
    const float* __restrict__ quats, const int32_t* __restrict__ nth, const int32_t* __restrict__ offsets,
    const float* __restrict__ partials, int rs, bool per_splat, bool fold, int64_t n_rows,
    const float* __restrict__ v_centers, CamArgs cam_args, double* __restrict__ workspace) {
    __shared__ double s_w[kPoseBlock / 64][kPoseVals];
    const int g = blockIdx.x * kPoseBlock + threadIdx.x;
    const Camera cam = load_camera(cam_args);
    double acc[kPoseVals];
#pragma unroll
    for (int k = 0; k < kPoseVals; ++k) acc[k] = 0.0;
    if (g < n) {
        // dW[r][k] = dL/dWk[r] (k = 0: a, 1: b, 2: mu column)
        double dW[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        bool any = false;
        float gcx = 0.f, gcy = 0.f;
        if (RASTER) {
            // deterministic mode over capacity (n_rows >= 0): the binning left every tile empty and no row exists
            const bool over = !per_splat && n_rows >= 0 && (int64_t)offsets[n] > n_rows;
            const int cnt = over ? 0 : nth[g];
            if (cnt > 0) {
                // accumulator mode: row g of the (n, rs) buffer; deterministic mode: the sums gstex_raster_setup_bwd
                // wrote over the splat's first row.  Columns [0, 12) and, in 32-value rows only, P_TW.
                const float* S = per_splat ? partials + (size_t)g * rs : partials + (size_t)offsets[g] * 4 * rs;
                auto sd = [&](int i) { return d3{(double)S[i], (double)S[i + 1], (double)S[i + 2]}; };
                const FrameT<double> fr = quat_frame_t<double>(quats + 4 * g);
                const double su = (double)scales[3 * g] * (double)glob, sv = (double)scales[3 * g + 1] * (double)glob;
                const d3 mu = d3{(double)means[3 * g], (double)means[3 * g + 1], (double)means[3 * g + 2]};
                const AnchoredT<double> an = splat_anchored(cam, mu, su, sv, fr);
                d3 A, B, Pw;
                affine_homog_vjp(an.Tu, an.Tv, an.Tw, sd(P_A), sd(P_B), sd(P_P0), A, B, Pw);
                if (rs == kPartRowGeo) Pw = add3(Pw, sd(P_TW));
                // splat_anchored_vjp's camera-space stage
                const d3 r0 = scale3(A, (double)cam.fx), r1 = scale3(B, (double)cam.fy);
                dW[0][0] = r0.x; dW[0][1] = r0.y; dW[0][2] = r0.z;
                dW[1][0] = r1.x; dW[1][1] = r1.y; dW[1][2] = r1.z;
                dW[2][0] = (Pw.x - an.xn * r0.x) - an.yn * r1.x;
                dW[2][1] = (Pw.y - an.xn * r0.y) - an.yn * r1.y;
                dW[2][2] = (Pw.z - an.xn * r0.z) - an.yn * r1.z;
                any = true;
                if (fold) { gcx = S[P_XY + 0]; gcy = S[P_XY + 1]; }
            }
        } else {
            gcx = v_centers[2 * g];
            gcy = v_centers[2 * g + 1];
        }
        if (!(gcx == 0.0f && gcy == 0.0f)) {
            // the cull decision is the forward's (fp32, aabb_from_homog); the chain is fp64
            float acx, acy, aex, aey;
            const Frame frf = quat_frame(quats + 4 * g);
            const Homog hf = splat_homography(cam, mk3(means[3 * g], means[3 * g + 1], means[3 * g + 2]),
                                              scales[3 * g] * glob, scales[3 * g + 1] * glob, frf);
            if (aabb_from_homog(hf, acx, acy, aex, aey)) {
                const FrameT<double> fr = quat_frame_t<double>(quats + 4 * g);
                const double su = (double)scales[3 * g] * (double)glob, sv = (double)scales[3 * g + 1] * (double)glob;
                const d3 mu = d3{(double)means[3 * g], (double)means[3 * g + 1], (double)means[3 * g + 2]};
                const HomogT<double> h = splat_homography(cam, mu, su, sv, fr);
                d3 dTu, dTv, dTw;
                aabb_centre_vjp_d(h, (double)gcx, (double)gcy, dTu, dTv, dTw);
                // splat_homography_vjp's camera-space stage
                const double fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
                dW[0][0] += fx * dTu.x; dW[0][1] += fx * dTu.y; dW[0][2] += fx * dTu.z;
                dW[1][0] += fy * dTv.x; dW[1][1] += fy * dTv.y; dW[1][2] += fy * dTv.z;
                dW[2][0] += (cx * dTu.x + cy * dTv.x) + dTw.x;
                dW[2][1] += (cx * dTu.y + cy * dTv.y) + dTw.y;
                dW[2][2] += (cx * dTu.z + cy * dTv.z) + dTw.z;
                any = true;
            }
        }
        if (any) {
            const FrameT<double> fr = quat_frame_t<double>(quats + 4 * g);
            const double su = (double)scales[3 * g] * (double)glob, sv = (double)scales[3 * g + 1] * (double)glob;
            const d3 a = scale3(fr.tu, su), b = scale3(fr.tv, sv);
            const d3 mu = d3{(double)means[3 * g], (double)means[3 * g + 1], (double)means[3 * g + 2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                acc[4 * r + 0] = (dW[r][0] * a.x + dW[r][1] * b.x) + dW[r][2] * mu.x;
                acc[4 * r + 1] = (dW[r][0] * a.y + dW[r][1] * b.y) + dW[r][2] * mu.y;
                acc[4 * r + 2] = (dW[r][0] * a.z + dW[r][1] * b.z) + dW[r][2] * mu.z;
                acc[4 * r + 3] = dW[r][2];
            }
        }
    }
    const double r = pose_block_sum(acc, s_w);
    if (threadIdx.x < kPoseVals) workspace[(size_t)blockIdx.x * kPoseVals + threadIdx.x] = r;
}

// One block: thread t sums rows t, t + 256, ... in order, then the block sum -> 12 floats.
__global__ __launch_bounds__(kPoseBlock) void viewmat_bwd_final_kernel(int n_rows, const double* __restrict__ workspace,
                                                                      float* __restrict__ v_viewmat) {
    __shared__ double s_w[kPoseBlock / 64][kPoseVals];
    double acc[kPoseVals];
#pragma unroll
    for (int k = 0; k < kPoseVals; ++k) acc[k] = 0.0;
    for (int row = threadIdx.x; row < n_rows; row += kPoseBlock) {
#pragma unroll
        for (int k = 0; k < kPoseVals; ++k) acc[k] = acc[k] + workspace[(size_t)row * kPoseVals + k];
    }
    const double r = pose_block_sum(acc, s_w);
    if (threadIdx.x < kPoseVals) v_viewmat[threadIdx.x] = (float)r;
}

__global__ void viewmat_zero_kernel(float* __restrict__ v_viewmat) {
    if (threadIdx.x < kPoseVals) v_viewmat[threadIdx.x] = 0.f;
}

}  // namespace

extern "C" size_t gstex_raster_viewmat_bwd_workspace(int32_t n) {
    if (n <= 0) return 0;
    return (size_t)div_up(n, kPoseBlock) * kPoseVals * sizeof(double);
}

extern "C" int gstex_raster_viewmat_bwd(const gstex_raster_viewmat_bwd_args* a, void* stream) {
    GSTEX_REQUIRE(a && a->n >= 0, "gstex_raster_viewmat_bwd: invalid arguments");
    GSTEX_REQUIRE(a->v_viewmat && a->cam.viewmat, "gstex_raster_viewmat_bwd: null pointer");
    hipStream_t st = as_stream(stream);
    if (a->n == 0) {
        viewmat_zero_kernel<<<1, 64, 0, st>>>(a->v_viewmat);
        return launch_status("gstex_raster_viewmat_bwd");
    }
    GSTEX_REQUIRE(a->means && a->scales && a->quats && a->workspace, "gstex_raster_viewmat_bwd: null pointer");
    const int blocks = div_up(a->n, kPoseBlock);
    if (a->partials) {
        GSTEX_REQUIRE(a->num_tiles_hit && a->offsets, "gstex_raster_viewmat_bwd: null pointer");
        GSTEX_REQUIRE(!a->v_centers,
                      "gstex_raster_viewmat_bwd: v_centers is the centre-only mode's input (partials == NULL); with "
                      "partials the centre gradient is the rows' own (fold_aabb)");
        GSTEX_REQUIRE(a->row_floats == kPartRow || a->row_floats == kPartRowGeo,
                      "gstex_raster_viewmat_bwd: row_floats must be %d or %d (got %d)", kPartRow, kPartRowGeo,
                      a->row_floats);
        viewmat_bwd_kernel<true><<<blocks, kPoseBlock, 0, st>>>(
            a->n, a->means, a->scales, a->glob_scale, a->quats, a->num_tiles_hit, a->offsets, a->partials,
            a->row_floats, a->row_flags == nullptr, a->fold_aabb != 0, a->n_rows, nullptr, to_device_camera(a->cam),
            a->workspace);
    } else {
        GSTEX_REQUIRE(a->v_centers, "gstex_raster_viewmat_bwd: neither partials nor v_centers");
        viewmat_bwd_kernel<false><<<blocks, kPoseBlock, 0, st>>>(
            a->n, a->means, a->scales, a->glob_scale, a->quats, nullptr, nullptr, nullptr, 0, true, false, -1,
            a->v_centers, to_device_camera(a->cam), a->workspace);
    }
    viewmat_bwd_final_kernel<<<1, kPoseBlock, 0, st>>>(blocks, a->workspace, a->v_viewmat);
    return launch_status("gstex_raster_viewmat_bwd");
}
