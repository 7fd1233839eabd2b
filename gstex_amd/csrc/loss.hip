// loss.hip — the GStex photometric loss, fused: background composite, clamp, 0.8 L1 + 0.2 (1 - SSIM).
//
//   gstex_loss_fwd / gstex_loss_bwd  <- gstex.py:1204-1205 (rgb = clamp(img + tex + (1-alpha) bg))
//                                       and gstex.py:1301-1322 (0.8 * L1 + 0.2 * (1 - SSIM)),
//                                       SSIM with pytorch_msssim semantics (gstex.py:351): 11-tap
//                                       gaussian window (sigma 1.5, weights supplied by the caller),
//                                       VALID filtering, C1 = 0.01^2, C2 = 0.03^2, mean over the map.
//     X = gt, Y = rgb; only Y is differentiated.
//
// Forward, one 16x16 workgroup tile per image block and channel: the 26x26 input window is
// staged in LDS, filtered separably (rows, then columns) into mu1, mu2, E[X^2], E[Y^2], E[XY];
// every valid position p writes s(p) into a per-workgroup partial sum and the three partials the
// backward needs, dS/d mu2, dS/d E[Y^2], dS/d E[XY] (gmaps).  A one-workgroup kernel then reduces
// the partial sums in a fixed order (deterministic loss).
// Backward: dS/dY(q) = sum over the windows containing q of w * (G_mu2 + 2 Y(q) G_yy + X(q) G_xy),
// the transposed separable filter of the gmaps, evaluated the same tiled way, channel by channel; the
// composite's backward (d_img, d_tex, d_alpha) is written by the same workgroup once a pixel's three channels are
// done (no dL/drgb buffer, no separate scatter launch).
//
//   gstex_loss_target_fwd / _bwd     <- the same loss on the target a dataset delivers (gstex.py:1238-1260, 1294-1299):
//                                       both kernels are templates over a target-load policy <dtype, channels, mask>;
//                                       uint8 -> v / 255, RGBA -> a * g + (1 - a) * bg and the mask multiply happen in
//                                       the staging loop, once per staged pixel.  gstex_loss_fwd / _bwd are the trivial
//                                       instantiation (fp32, 3 channels, no mask, no MSE partial): same arithmetic.
//
//   gstex_eval_metrics               <- the evaluation protocol of get_image_metrics_and_images (gstex.py:1337-1403) on
//                                       one view: the render quantised to uint8 (:1379-1381) in the staging loop, PSNR
//                                       and SSIM against the composited target.  Forward only (metrics_fwd_kernel): no
//                                       gmaps, no mask, no L1.
//
// Stated once, for both forwards: the row and column filters, the SSIM point and the workgroup's partial sums
// (ssim_rows, ssim_columns, ssim_point, block_sums); the fp64 reduction of the partial records (reduce_kernel); and on
// the host the argument checks, the launch description and the dtype x channels x mask dispatch of all five entry
// points.  The two forward kernels differ in their staging loops only.
#include "gstex_common.h"
#include "gstex_error.h"

namespace {

constexpr int kLT = 16;            // output tile side
constexpr int kWin = 11;           // gaussian window
constexpr int kHalo = kWin - 1;    // 10
constexpr int kReg = kLT + kHalo;  // 26: staged window side
constexpr float kC1 = 0.01f * 0.01f;
constexpr float kC2 = 0.03f * 0.03f;

struct Win {
    float w[kWin];
};

// rgb = clamp((img + tex) + (1 - alpha) * bg, 0, 1) exactly as gstex.py:1204 evaluates it; `pre`
// returns the unclamped value (the clamp's gradient mask).
__device__ __forceinline__ float composite(const float* img, const float* tex, const float* alpha, const float* bg,
                                           int C, size_t pix, int c, float& pre) {
    const float v = (img[3 * pix + c] + tex[(size_t)C * pix + c]) + (1.0f - alpha[pix]) * bg[c];
    pre = v;
    return fminf(fmaxf(v, 0.0f), 1.0f);
}

// ---- target-load policy -------------------------------------------------------------------------------------------
// DT: GSTEX_GT_F32 / GSTEX_GT_U8; CH: 3 or 4 (straight alpha in channel 3); MK: kMaskNone / kMaskF32 / kMaskBool.
// Every operation below is one individually rounded fp32 operation (no contraction: outside the filters' blocks).
constexpr int kMaskNone = 0, kMaskF32 = 1, kMaskBool = 2;

// the target image's element type
template <int DT>
struct GtElem {
    using type = float;
};
template <>
struct GtElem<GSTEX_GT_U8> {
    using type = unsigned char;
};

template <int DT>
using GtPtr = const typename GtElem<DT>::type*;

template <int DT>
__device__ __forceinline__ float gt_scalar(GtPtr<DT> gt, size_t i) {
    if constexpr (DT == GSTEX_GT_U8) return (float)gt[i] / 255.0f;
    else return gt[i];
}

// an RGBA pixel in one load: a 32-bit word (uint8) or a float4 (fp32)
template <int DT>
__device__ __forceinline__ void gt_rgba(GtPtr<DT> gt, size_t pix, float v[4]) {
    if constexpr (DT == GSTEX_GT_U8) {
        const unsigned w = ((const unsigned*)gt)[pix];
        v[0] = (float)(w & 255u) / 255.0f;
        v[1] = (float)((w >> 8) & 255u) / 255.0f;
        v[2] = (float)((w >> 16) & 255u) / 255.0f;
        v[3] = (float)(w >> 24) / 255.0f;
    } else {
        const float4 p = ((const float4*)gt)[pix];
        v[0] = p.x, v[1] = p.y, v[2] = p.z, v[3] = p.w;
    }
}

// gt = a * g + (1 - a) * bg as the eager expression (gstex.py:1258) evaluates it: two rounded products, then the sum
__device__ __forceinline__ float over_background(float g, float a, float bgc) {
    const float p = a * g;
    const float q = (1.0f - a) * bgc;
    return p + q;
}

// the target's channel c at one pixel (c is uniform over the workgroup)
template <int DT, int CH>
__device__ __forceinline__ float gt_channel(GtPtr<DT> gt, const float* bg, size_t pix, int c) {
    if constexpr (CH == 4) {
        float v[4];
        gt_rgba<DT>(gt, pix, v);
        return over_background(c == 0 ? v[0] : (c == 1 ? v[1] : v[2]), v[3], bg[c]);
    } else {
        return gt_scalar<DT>(gt, 3 * pix + c);
    }
}

template <int MK>
__device__ __forceinline__ float mask_value(const void* mask, size_t pix) {
    if constexpr (MK == kMaskF32) return ((const float*)mask)[pix];
    else if constexpr (MK == kMaskBool) return ((const unsigned char*)mask)[pix] != 0 ? 1.0f : 0.0f;
    else return 1.0f;
}

#ifndef GSTEX_LOSS_XCD
#define GSTEX_LOSS_XCD 1
#endif
// XCD-aware tile order: workgroups are dispatched round-robin over the 8 XCDs, each with its own L2, so
// in launch order neighbouring tiles (which share their 10-pixel halos) land on different XCDs and the
// halos come from HBM again.  Launch slot L goes to XCD L % 8; giving XCD x the contiguous run of tiles
// [x * n/8, ...) in (bx, by, c) order keeps neighbours on one L2.  A bijection of the launch slots.
struct LossTile {
    int bx, by, c;
};
__device__ __forceinline__ LossTile loss_tile() {
    if (!GSTEX_LOSS_XCD) return LossTile{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
    const int gx = gridDim.x, gy = gridDim.y;
    const int n = gx * gy * gridDim.z;
    const int L = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int per = n / 8, rem = n % 8, xcd = L % 8;
    const int t = xcd * per + min(xcd, rem) + L / 8;
    return LossTile{t % gx, (t / gx) % gy, t / (gx * gy)};
}

// ---- the SSIM tile pipeline of both forward kernels -------------------------------------------------------------
// Each piece carries its own contraction pragma (fused multiply-adds: the window sums need no fixed operation order --
// the loss and its gradient are compared with tolerances, only the composite bit for bit).  The staging loops that fill
// s_x / s_y stay in the kernels, outside it.

// rows: 26 x 16 horizontal filters of the five window moments of the staged X and Y
__device__ __forceinline__ void ssim_rows(const Win& win, const float (&s_x)[kReg][kReg + 1],
                                          const float (&s_y)[kReg][kReg + 1], float (&s_h)[5][kReg][kLT + 1]) {
    for (int i = threadIdx.x; i < kReg * kLT; i += 256) {
#pragma clang fp contract(fast)
        const int ry = i / kLT, cx = i % kLT;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float xv = s_x[ry][cx + k], yv = s_y[ry][cx + k];
            a += win.w[k] * xv;
            b += win.w[k] * yv;
            aa += win.w[k] * (xv * xv);
            bb += win.w[k] * (yv * yv);
            ab += win.w[k] * (xv * yv);
        }
        s_h[0][ry][cx] = a;
        s_h[1][ry][cx] = b;
        s_h[2][ry][cx] = aa;
        s_h[3][ry][cx] = bb;
        s_h[4][ry][cx] = ab;
    }
}

// columns: q = {mu1, mu2, E[X^2], E[Y^2], E[XY]} at tile position (cy, cx)
__device__ __forceinline__ void ssim_columns(const Win& win, const float (&s_h)[5][kReg][kLT + 1], int cy, int cx,
                                             float (&q)[5]) {
#pragma clang fp contract(fast)
#pragma unroll
    for (int m = 0; m < 5; ++m) q[m] = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k)
#pragma unroll
        for (int m = 0; m < 5; ++m) q[m] += win.w[k] * s_h[m][cy + k][cx];
}

// the SSIM map's value s at one position, with the terms its derivatives are made of
struct SsimPoint {
    float mu1, mu2, A, B, Cc, D, s;
};
__device__ __forceinline__ SsimPoint ssim_point(const float (&q)[5]) {
#pragma clang fp contract(fast)
    const float mu1 = q[0], mu2 = q[1];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const float s11 = q[2] - mu1_sq, s22 = q[3] - mu2_sq, s12 = q[4] - mu1_mu2;
    const float A = 2.0f * mu1_mu2 + kC1, B = 2.0f * s12 + kC2;
    const float Cc = mu1_sq + mu2_sq + kC1, D = s11 + s22 + kC2;
    const float cs = B / D;
    return SsimPoint{mu1, mu2, A, B, Cc, D, (A / Cc) * cs};
}

// what the backward filters (the loss forward only): g = {dS/d mu2 in full, dS/dE[Y^2], dS/dE[XY]}
__device__ __forceinline__ void ssim_point_gmaps(const SsimPoint& p, float (&g)[3]) {
#pragma clang fp contract(fast)
    // dS/d mu2 (through mu2, sigma2^2 = E[Y^2] - mu2^2, sigma12 = E[XY] - mu1 mu2), dS/dE[Y^2], dS/dE[XY]
    const float ds_dmu2 = p.s * (2.0f * p.mu1 / p.A - 2.0f * p.mu2 / p.Cc);
    const float ds_ds22 = -p.s / p.D;
    const float ds_ds12 = 2.0f * p.s / p.B;
    g[0] = ds_dmu2 - 2.0f * p.mu2 * ds_ds22 - p.mu1 * ds_ds12;
    g[1] = ds_ds22;
    g[2] = ds_ds12;
}

// The workgroup's sums of N per-thread values, stored as partial record b = part[N * b ..] with b the tile index (not
// the launch slot): wave reduce, then the 4 waves in order, so the reduction order is fixed.  Every thread calls it.
template <int N>
__device__ __forceinline__ void block_sums(float (&v)[N], const LossTile& lt, float* __restrict__ part) {
    __shared__ float s_red[N][4];
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int m = 0; m < N; ++m) v[m] += __shfl_xor(v[m], off, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int m = 0; m < N; ++m) s_red[m][tid >> 6] = v[m];
    }
    __syncthreads();
    if (tid == 0) {
        const int b = (lt.c * gridDim.y + lt.by) * gridDim.x + lt.bx;
#pragma unroll
        for (int m = 0; m < N; ++m) part[N * b + m] = ((s_red[m][0] + s_red[m][1]) + s_red[m][2]) + s_red[m][3];
    }
}

// What only the dataset-target instantiations take, as a trailing kernel argument: empty for gstex_loss_fwd / _bwd,
// whose kernels keep the argument layout (and so the code) they had before the policy.
template <bool EXT>
struct FwdExtra {};
template <>
struct FwdExtra<true> {
    const void* mask;
    float* gt_out;  // nullable: the composited target image
};
template <int MK>
struct BwdExtra {
    const void* mask;
};
template <>
struct BwdExtra<kMaskNone> {};

// EXT: the dataset-target entry point -- also the unmasked MSE partial (three floats per workgroup instead of two) and
// the composited target image.
template <int DT, int CH, int MK, bool EXT>
__global__ __launch_bounds__(256) void loss_fwd_kernel(int H, int W, int C, const float* __restrict__ img,
                                                       const float* __restrict__ tex,
                                                       const float* __restrict__ alpha,
                                                       const float* __restrict__ bg,
                                                       GtPtr<DT> __restrict__ gt, Win win,
                                                       float* __restrict__ rgb_out,
                                                       float* __restrict__ gmaps, float* __restrict__ part,
                                                       FwdExtra<EXT> ex) {
    __shared__ float s_x[kReg][kReg + 1], s_y[kReg][kReg + 1];
    __shared__ float s_h[5][kReg][kLT + 1];
    const LossTile lt = loss_tile();
    const int c = lt.c;
    const int x0 = lt.bx * kLT, y0 = lt.by * kLT;
    const int tid = threadIdx.x;
    const int Hv = H - kHalo, Wv = W - kHalo;
    float l1 = 0.f;
    [[maybe_unused]] float mse = 0.f;
    for (int i = tid; i < kReg * kReg; i += 256) {
        const int ry = i / kReg, rx = i % kReg;
        const int y = y0 + ry, x = x0 + rx;
        float xv = 0.f, yv = 0.f;
        if (y < H && x < W) {
            const size_t pix = (size_t)y * W + x;
            float pre;
            yv = composite(img, tex, alpha, bg, C, pix, c, pre);
            xv = gt_channel<DT, CH>(gt, bg, pix, c);
            [[maybe_unused]] const float gtv = xv, rgbv = yv;  // the unmasked values: outputs["rgb"], the MSE's terms
            if constexpr (MK != kMaskNone) {  // X = gt * m, Y = rgb * m (gstex.py:1298-1299)
                const float m = mask_value<MK>(ex.mask, pix);
                xv = xv * m;
                yv = yv * m;
            }
            if (rx < kLT && ry < kLT) {  // each pixel's L1 term and rgb belong to the tile whose core holds it
                l1 += fabsf(xv - yv);
                if constexpr (MK != kMaskNone) {
                    if (rgb_out) rgb_out[3 * pix + c] = rgbv;
                } else {
                    if (rgb_out) rgb_out[3 * pix + c] = yv;
                }
                if constexpr (EXT) {
                    const float d = rgbv - gtv;  // unmasked, as get_metrics_dict computes it
                    mse += d * d;
                    if (ex.gt_out) ex.gt_out[3 * pix + c] = gtv;
                }
            }
        }
        s_x[ry][rx] = xv;
        s_y[ry][rx] = yv;
    }
    __syncthreads();
    // a local copy: the compiler then issues the window's kernel-argument loads with the others at entry, ahead of the
    // first wait, and keeps 8 SGPRs fewer (measured: 0.3-0.4 us of the 800x800 forward + backward pair, EXPERIMENTS.md
    // "loss.hip refactor"; metrics_fwd_kernel loads everything at entry without one)
    const Win w = win;
    ssim_rows(w, s_x, s_y, s_h);
    __syncthreads();
    // columns + the SSIM map at this thread's position
    const int cy = tid >> 4, cx = tid & 15;
    const int py = y0 + cy, px = x0 + cx;
    constexpr int N = EXT ? 3 : 2;  // the partial record: {sum s, sum |X - Y|} (+ sum (rgb - gt)^2)
    float sums[N] = {};
    if (py < Hv && px < Wv) {
        float q[5], g[3];
        ssim_columns(w, s_h, cy, cx, q);
        const SsimPoint p = ssim_point(q);
        ssim_point_gmaps(p, g);
        sums[0] = p.s;
        const size_t o = ((size_t)c * Hv + py) * Wv + px;
        const size_t plane = (size_t)3 * Hv * Wv;
        gmaps[o] = g[0];
        gmaps[plane + o] = g[1];
        gmaps[2 * plane + o] = g[2];
    }
    sums[1] = l1;
    if constexpr (EXT) sums[2] = mse;
    block_sums<N>(sums, lt, part);
}

// The partial records' sums: one workgroup, fp64, a strided accumulation and a 512 -> 1 tree (one fixed order), then
// `finish` turns the N sums into the output floats.
template <int N, class Finish>
__global__ __launch_bounds__(1024) void reduce_kernel(int nparts, const float* __restrict__ part, Finish finish,
                                                      float* __restrict__ out) {
    __shared__ double s_sum[N][1024];
    double acc[N] = {};
    for (int i = threadIdx.x; i < nparts; i += 1024) {
#pragma unroll
        for (int m = 0; m < N; ++m) acc[m] += (double)part[N * i + m];
    }
#pragma unroll
    for (int m = 0; m < N; ++m) s_sum[m][threadIdx.x] = acc[m];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int m = 0; m < N; ++m) s_sum[m][threadIdx.x] += s_sum[m][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double sums[N];
#pragma unroll
        for (int m = 0; m < N; ++m) sums[m] = s_sum[m][0];
        finish(sums, out);
    }
}

// {loss, L1, SSIM} from {sum s, sum |X - Y|}; with the target path's third partial also the MSE
struct LossFinish {
    double inv_n1, inv_np;
    float w_l1, w_ssim;
    template <int N>
    __device__ void operator()(const double (&sums)[N], float* out) const {
        const float l1 = (float)(sums[1] * inv_n1);
        const float ssim = (float)(sums[0] * inv_np);
        out[0] = w_l1 * l1 + w_ssim * (1.0f - ssim);
        out[1] = l1;
        out[2] = ssim;
        if constexpr (N == 3) out[3] = (float)(sums[2] * inv_n1);
    }
};

// {PSNR, SSIM, MSE, MSE_raw} from {sum s, sum (y - gt)^2, sum (rgb - gt)^2}; PSNR = -10 log10(MSE) (+inf when every
// byte equals its target)
struct MetricsFinish {
    double inv_n1, inv_np;
    __device__ void operator()(const double (&sums)[3], float* out) const {
        const float mse = (float)(sums[1] * inv_n1);
        out[0] = -10.0f * log10f(mse);
        out[1] = (float)(sums[0] * inv_np);
        out[2] = mse;
        out[3] = (float)(sums[2] * inv_n1);
    }
};

template <int DT, int CH, int MK>
__global__ __launch_bounds__(256) void loss_bwd_kernel(int H, int W, int C, const float* __restrict__ img,
                                                       const float* __restrict__ tex,
                                                       const float* __restrict__ alpha,
                                                       const float* __restrict__ bg,
                                                       GtPtr<DT> __restrict__ gt, Win win,
                                                       const float* __restrict__ gmaps,
                                                       const float* __restrict__ grad_loss, float k_l1,
                                                       float k_ssim, float* __restrict__ d_img,
                                                       float* __restrict__ d_tex, float* __restrict__ d_alpha,
                                                       BwdExtra<MK> ex) {
    // one workgroup per 16x16 tile, the three channels in turn; the composite's backward (d_img, d_tex, d_alpha)
    // written at the end, once every channel's dL/drgb of the pixel is known
    __shared__ float s_g[3][kReg][kReg + 1];
    __shared__ float s_h[3][kReg][kLT + 1];
    const LossTile lt = loss_tile();
    const int x0 = lt.bx * kLT, y0 = lt.by * kLT;  // output pixels [x0, x0+16)
    const int tid = threadIdx.x;
    const int Hv = H - kHalo, Wv = W - kHalo;
    const size_t plane = (size_t)3 * Hv * Wv;
    const int cy = tid >> 4, cx = tid & 15;
    const int qy = y0 + cy, qx = x0 + cx;
    const bool out = qy < H && qx < W;
    const size_t pix = (size_t)qy * W + qx;
    const float gl = grad_loss[0];
    float gch[3];
    // an RGBA target pixel and the mask are read once per pixel, before the channel loop
    [[maybe_unused]] float tv[4] = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] float m = 1.0f;
    if (out) {
        if constexpr (CH == 4) gt_rgba<DT>(gt, pix, tv);
        if constexpr (MK != kMaskNone) m = mask_value<MK>(ex.mask, pix);
    }
    for (int c = 0; c < 3; ++c) {
        if (c > 0) __syncthreads();  // the previous channel's passes are done with s_g / s_h
        // gmaps over positions [x0 - 10, x0 + 16)
        for (int i = tid; i < kReg * kReg; i += 256) {
            const int ry = i / kReg, rx = i % kReg;
            const int gy = y0 - kHalo + ry, gx = x0 - kHalo + rx;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (gy >= 0 && gx >= 0 && gy < Hv && gx < Wv) {
                const size_t o = ((size_t)c * Hv + gy) * Wv + gx;
                g0 = gmaps[o];
                g1 = gmaps[plane + o];
                g2 = gmaps[2 * plane + o];
            }
            s_g[0][ry][rx] = g0;
            s_g[1][ry][rx] = g1;
            s_g[2][ry][rx] = g2;
        }
        __syncthreads();
        // transposed rows: for output column hx, sum_k w[k] G(position hx + 10 - k)
        for (int i = tid; i < kReg * kLT; i += 256) {
#pragma clang fp contract(fast)
            const int ry = i / kLT, hx = i % kLT;
            float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                a += win.w[k] * s_g[0][ry][hx + kHalo - k];
                b += win.w[k] * s_g[1][ry][hx + kHalo - k];
                d += win.w[k] * s_g[2][ry][hx + kHalo - k];
            }
            s_h[0][ry][hx] = a;
            s_h[1][ry][hx] = b;
            s_h[2][ry][hx] = d;
        }
        __syncthreads();
        gch[c] = 0.f;
        if (out) {
#pragma clang fp contract(fast)
            float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                t0 += win.w[k] * s_h[0][cy + kHalo - k][cx];
                t1 += win.w[k] * s_h[1][cy + kHalo - k][cx];
                t2 += win.w[k] * s_h[2][cy + kHalo - k][cx];
            }
            float pre;
            float yv = composite(img, tex, alpha, bg, C, pix, c, pre);
            float xv;
            if constexpr (CH == 4) xv = over_background(c == 0 ? tv[0] : (c == 1 ? tv[1] : tv[2]), tv[3], bg[c]);
            else xv = gt_scalar<DT>(gt, 3 * pix + c);
            if constexpr (MK != kMaskNone) {
                xv = xv * m;
                yv = yv * m;
            }
            const float dS = (t0 + 2.0f * yv * t1) + xv * t2;
            const float diff = xv - yv;
            const float sgn = diff > 0.f ? 1.0f : (diff < 0.f ? -1.0f : 0.0f);
            // L = w1 * mean|X - Y| + w2 * (1 - mean s): dL/dY = -w1 sign(X - Y) / N1 - w2 dS / Np
            float g = -(k_l1 * sgn) - k_ssim * dS;
            g *= gl;
            if constexpr (MK != kMaskNone) g = m * g;  // dL/drgb = m * dL/dY
            gch[c] = (pre >= 0.0f && pre <= 1.0f) ? g : 0.0f;
        }
    }
    if (!out) return;
    // rgb = clamp((img + tex) + (1 - alpha) bg): d_img = d_tex[0..2] = dL/drgb, channels >= 3 get zero,
    // d_alpha = -sum_c dL/drgb_c bg_c
    d_img[3 * pix] = gch[0];
    d_img[3 * pix + 1] = gch[1];
    d_img[3 * pix + 2] = gch[2];
    // (d_tex NULL: the caller's d_tex is d_img, C = 3, the same image, already written)
    if (d_tex)
        for (int c = 0; c < C; ++c) d_tex[(size_t)C * pix + c] = c == 0 ? gch[0] : (c == 1 ? gch[1] : (c == 2 ? gch[2] : 0.0f));
    d_alpha[pix] = -((gch[0] * bg[0] + gch[1] * bg[1]) + gch[2] * bg[2]);
}

// ---- evaluation metrics (uint8-quantised PSNR / SSIM, forward only) ----------------------------------------------
constexpr int kMetricParts = 3;  // per workgroup: {sum s, sum (y - gt)^2, sum (rgb - gt)^2}

// The loss forward's tiling (one workgroup per 16x16 tile and channel, XCD-aware order) with the reference's uint8
// quantisation of the render in the staging loop: Y = (float)(uint8)(255 rgb) * (1 / 255), X = gt.  No gmaps and no
// L1; the quantised bytes, the unquantised render and the composited target are optional outputs.  The three channels
// of a pixel belong to three workgroups, so the rgb_u8_out stores are single bytes three apart.
template <int DT, int CH>
__global__ __launch_bounds__(256) void metrics_fwd_kernel(int H, int W, int C, const float* __restrict__ img,
                                                          const float* __restrict__ tex,
                                                          const float* __restrict__ alpha,
                                                          const float* __restrict__ bg, GtPtr<DT> __restrict__ gt,
                                                          Win win, float* __restrict__ rgb_out,
                                                          unsigned char* __restrict__ rgb_u8_out,
                                                          float* __restrict__ gt_out, float* __restrict__ part) {
    __shared__ float s_x[kReg][kReg + 1], s_y[kReg][kReg + 1];
    __shared__ float s_h[5][kReg][kLT + 1];
    const LossTile lt = loss_tile();
    const int c = lt.c;
    const int x0 = lt.bx * kLT, y0 = lt.by * kLT;
    const int tid = threadIdx.x;
    const int Hv = H - kHalo, Wv = W - kHalo;
    float mse = 0.f, mse_raw = 0.f;
    for (int i = tid; i < kReg * kReg; i += 256) {
        const int ry = i / kReg, rx = i % kReg;
        const int y = y0 + ry, x = x0 + rx;
        float xv = 0.f, yv = 0.f;
        if (y < H && x < W) {
            const size_t pix = (size_t)y * W + x;
            float pre;
            const float rgbv = composite(img, tex, alpha, bg, C, pix, c, pre);
            xv = gt_channel<DT, CH>(gt, bg, pix, c);
            // (255.0 * rgb).to(uint8).to(float32) / 255.0 (gstex.py:1380-1381): the conversion truncates, and the
            // device divides by a scalar as a multiplication by its rounded reciprocal
            const float scaled = 255.0f * rgbv;
            const unsigned char q = (unsigned char)scaled;
            yv = (float)q * (1.0f / 255.0f);
            if (rx < kLT && ry < kLT) {  // each pixel's outputs and MSE terms belong to the tile whose core holds it
                const float d = yv - xv;
                mse += d * d;
                const float dr = rgbv - xv;  // unquantised, as get_metrics_dict computes it
                mse_raw += dr * dr;
                if (rgb_out) rgb_out[3 * pix + c] = rgbv;
                if (rgb_u8_out) rgb_u8_out[3 * pix + c] = q;
                if (gt_out) gt_out[3 * pix + c] = xv;
            }
        }
        s_x[ry][rx] = xv;
        s_y[ry][rx] = yv;
    }
    __syncthreads();
    ssim_rows(win, s_x, s_y, s_h);
    __syncthreads();
    const int cy = tid >> 4, cx = tid & 15;
    const int py = y0 + cy, px = x0 + cx;
    float sums[kMetricParts] = {0.f, mse, mse_raw};
    if (py < Hv && px < Wv) {
        float q[5];
        ssim_columns(win, s_h, cy, cx, q);
        sums[0] = ssim_point(q).s;
    }
    block_sums<kMetricParts>(sums, lt, part);
}

}  // namespace

using namespace gstex;

// forward: one workgroup per (tile, channel); backward: one per tile (its three channels in turn)
static dim3 loss_grid(int H, int W, int channels = 3) {
    return dim3((unsigned)((W + kLT - 1) / kLT), (unsigned)((H + kLT - 1) / kLT), (unsigned)channels);
}

// the forward's workgroups = its partial records
static int loss_nparts(int H, int W) {
    const dim3 g = loss_grid(H, W);
    return (int)(g.x * g.y * g.z);
}

// workspace: the forward's partial records (part_floats each), padded to 256 bytes, then the gmaps
static size_t loss_parts_bytes(int H, int W, int part_floats) {
    return ((size_t)loss_nparts(H, W) * part_floats * sizeof(float) + 255) & ~(size_t)255;
}

static size_t loss_ws_size(int H, int W, int part_floats) {
    if (H <= kHalo || W <= kHalo) return 0;
    return loss_parts_bytes(H, W, part_floats) + (size_t)3 * 3 * (H - kHalo) * (W - kHalo) * sizeof(float);
}

extern "C" size_t gstex_loss_workspace_size(int32_t H, int32_t W) { return loss_ws_size(H, W, 2); }

extern "C" size_t gstex_loss_target_workspace_size(int32_t H, int32_t W) { return loss_ws_size(H, W, 3); }

// the partial records, nothing else (no gmaps)
extern "C" size_t gstex_eval_metrics_workspace_size(int32_t H, int32_t W) {
    if (H <= kHalo || W <= kHalo) return 0;
    return (size_t)loss_nparts(H, W) * kMetricParts * sizeof(float);
}

namespace {

// The checks every entry point makes, in the order they are reported.  `dims`: the message names the size (the
// forwards); `pointers`: the entry point's own non-null test; `need`: its workspace size.
int loss_check(const char* fn, bool dims, int H, int W, int C, bool pointers, const void* ws, size_t ws_bytes,
               size_t need) {
    const bool fits = H > kHalo && W > kHalo;
    if (dims) GSTEX_REQUIRE(fits, "%s: image must be larger than the %d-tap window (%dx%d)", fn, kWin, H, W);
    else GSTEX_REQUIRE(fits, "%s: image must be larger than the %d-tap window", fn, kWin);
    GSTEX_REQUIRE(C >= 3 && C <= 8, "%s: tex channels must be in [3, 8] (got %d)", fn, C);
    GSTEX_REQUIRE(pointers, "%s: null pointer", fn);
    GSTEX_REQUIRE(ws && ws_bytes >= need, "%s: workspace too small", fn);
    return GSTEX_OK;
}

// What the launches of every entry point take: the inputs, the workspace's two regions, and the scale factors of the
// reduction (inv_*, w_*) and of the backward (k_*).
struct LossLaunch {
    hipStream_t st;
    int H, W, C;
    const float *img, *tex, *alpha, *bg;
    const void *gt, *mask;
    Win win;
    float *part, *gmaps;
    double inv_n1, inv_np;  // 1 / (3 H W), 1 / (3 (H - 10) (W - 10))
    float w_l1, w_ssim;     // L = w_l1 L1 + w_ssim (1 - SSIM)
    float k_l1, k_ssim;     // w_l1 / (3 H W), w_ssim / (3 (H - 10) (W - 10))
};

LossLaunch loss_launch(int H, int W, int C, const float* img, const float* tex, const float* alpha, const float* bg,
                       const void* gt, const void* mask, const float* window, float ssim_lambda, void* workspace,
                       int part_floats, void* stream) {
    LossLaunch a;
    a.st = as_stream(stream);
    a.H = H, a.W = W, a.C = C;
    a.img = img, a.tex = tex, a.alpha = alpha, a.bg = bg;
    a.gt = gt, a.mask = mask;
    for (int k = 0; k < kWin; ++k) a.win.w[k] = window[k];  // host array
    a.part = (float*)workspace;
    a.gmaps = (float*)((char*)workspace + loss_parts_bytes(H, W, part_floats));
    a.inv_n1 = 1.0 / (3.0 * H * W);
    a.inv_np = 1.0 / (3.0 * (H - kHalo) * (W - kHalo));
    a.w_l1 = 1.0f - ssim_lambda, a.w_ssim = ssim_lambda;
    a.k_l1 = (float)((1.0 - ssim_lambda) / (3.0 * H * W));
    a.k_ssim = (float)(ssim_lambda / (3.0 * (H - kHalo) * (W - kHalo)));
    return a;
}

// what only one kind of launch takes
struct FwdOut {
    float *rgb_out, *gt_out;
};
struct BwdArgs {
    const float* grad_loss;
    float *d_img, *d_tex, *d_alpha;  // d_tex NULL: not stored (the caller passed d_tex == d_img)
};
// One gradient image for both outputs (d_tex == d_img, C = 3): the kernel writes it once
BwdArgs bwd_args(const float* grad_loss, float* d_img, float* d_tex, float* d_alpha) {
    return BwdArgs{grad_loss, d_img, d_tex == d_img ? nullptr : d_tex, d_alpha};
}
struct MetricsOut {
    float* rgb_out;
    unsigned char* rgb_u8_out;
    float* gt_out;
};

template <int DT, int CH, int MK, bool EXT = true>
void launch(const LossLaunch& a, const FwdOut& o) {
    FwdExtra<EXT> ex;
    if constexpr (EXT) ex = FwdExtra<true>{a.mask, o.gt_out};
    loss_fwd_kernel<DT, CH, MK, EXT><<<loss_grid(a.H, a.W), 256, 0, a.st>>>(
        a.H, a.W, a.C, a.img, a.tex, a.alpha, a.bg, (GtPtr<DT>)a.gt, a.win, o.rgb_out, a.gmaps, a.part, ex);
}

template <int DT, int CH, int MK>
void launch(const LossLaunch& a, const BwdArgs& o) {
    BwdExtra<MK> ex;
    if constexpr (MK != kMaskNone) ex.mask = a.mask;
    loss_bwd_kernel<DT, CH, MK><<<loss_grid(a.H, a.W, 1), 256, 0, a.st>>>(
        a.H, a.W, a.C, a.img, a.tex, a.alpha, a.bg, (GtPtr<DT>)a.gt, a.win, a.gmaps, o.grad_loss, a.k_l1, a.k_ssim,
        o.d_img, o.d_tex, o.d_alpha, ex);
}

template <int DT, int CH, int MK>  // (MK: always kMaskNone, gstex_eval_metrics refuses a mask)
void launch(const LossLaunch& a, const MetricsOut& o) {
    metrics_fwd_kernel<DT, CH><<<loss_grid(a.H, a.W), 256, 0, a.st>>>(
        a.H, a.W, a.C, a.img, a.tex, a.alpha, a.bg, (GtPtr<DT>)a.gt, a.win, o.rgb_out, o.rgb_u8_out, o.gt_out, a.part);
}

// the forward's partial records -> the output floats
template <int N, class Finish>
void launch_reduce(const LossLaunch& a, const Finish& finish, float* out) {
    reduce_kernel<N, Finish><<<1, 1024, 0, a.st>>>(loss_nparts(a.H, a.W), a.part, finish, out);
}

template <int DT, int CH, class Op>
void dispatch_mask(int mk, const LossLaunch& a, const Op& o) {
    if (mk == kMaskNone) launch<DT, CH, kMaskNone>(a, o);
    else if (mk == kMaskF32) launch<DT, CH, kMaskF32>(a, o);
    else launch<DT, CH, kMaskBool>(a, o);
}

// the policy instantiation of a (validated) target descriptor
template <class Op>
void dispatch_target(const gstex_loss_target& t, const LossLaunch& a, const Op& o) {
    const int mk = !t.mask ? kMaskNone : (t.mask_dtype == GSTEX_MASK_BOOL ? kMaskBool : kMaskF32);
    if (t.gt_dtype == GSTEX_GT_U8) {
        if (t.gt_channels == 4) dispatch_mask<GSTEX_GT_U8, 4>(mk, a, o);
        else dispatch_mask<GSTEX_GT_U8, 3>(mk, a, o);
    } else {
        if (t.gt_channels == 4) dispatch_mask<GSTEX_GT_F32, 4>(mk, a, o);
        else dispatch_mask<GSTEX_GT_F32, 3>(mk, a, o);
    }
}

// 0, or the message of the first invalid field (nothing is launched for an invalid descriptor)
const char* target_error(const gstex_loss_target* t) {
    if (!t) return "null target";
    if (!t->gt) return "null target gt";
    if (t->gt_dtype != GSTEX_GT_F32 && t->gt_dtype != GSTEX_GT_U8) return "gt_dtype out of range";
    if (t->gt_channels != 3 && t->gt_channels != 4) return "gt_channels must be 3 or 4";
    if (t->mask && t->mask_dtype != GSTEX_MASK_F32 && t->mask_dtype != GSTEX_MASK_BOOL)
        return "mask_dtype out of range";
    if (t->reserved != 0) return "reserved must be 0";
    // an RGBA pixel is read as one word / one float4; fp32 values and masks as floats
    const size_t align = t->gt_dtype == GSTEX_GT_F32 ? (t->gt_channels == 4 ? 16 : 4) : (t->gt_channels == 4 ? 4 : 1);
    if ((uintptr_t)t->gt % align != 0) return "target gt is not aligned to its pixel load";
    if (t->mask && t->mask_dtype == GSTEX_MASK_F32 && (uintptr_t)t->mask % 4 != 0) return "mask is not aligned";
    return nullptr;
}

}  // namespace

// gstex_loss_fwd / _bwd: the fp32, three-channel, unmasked instantiation without the MSE partial
extern "C" int gstex_loss_fwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                              const float* alpha, const float* background, const float* gt, const float* window,
                              float ssim_lambda, float* rgb_out, float* loss_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    const char* fn = "gstex_loss_fwd";
    if (int rc = loss_check(fn, true, H, W, C, img && tex && alpha && background && gt && window && loss_out,
                            workspace, workspace_bytes, gstex_loss_workspace_size(H, W)))
        return rc;
    const LossLaunch a = loss_launch(H, W, C, img, tex, alpha, background, gt, nullptr, window, ssim_lambda, workspace,
                                     2, stream);
    launch<GSTEX_GT_F32, 3, kMaskNone, false>(a, FwdOut{rgb_out, nullptr});
    launch_reduce<2>(a, LossFinish{a.inv_n1, a.inv_np, a.w_l1, a.w_ssim}, loss_out);
    return launch_status(fn);
}

extern "C" int gstex_loss_bwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                              const float* alpha, const float* background, const float* gt, const float* window,
                              float ssim_lambda, const float* grad_loss, float* d_img, float* d_tex, float* d_alpha,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "gstex_loss_bwd";
    if (int rc = loss_check(fn, false, H, W, C,
                            img && tex && alpha && background && gt && window && grad_loss && d_img && d_tex && d_alpha,
                            workspace, workspace_bytes, gstex_loss_workspace_size(H, W)))
        return rc;
    GSTEX_REQUIRE(d_tex != d_img || C == 3, "%s: d_tex may be d_img only with C == 3 (got %d)", fn, C);
    const LossLaunch a = loss_launch(H, W, C, img, tex, alpha, background, gt, nullptr, window, ssim_lambda, workspace,
                                     2, stream);
    launch<GSTEX_GT_F32, 3, kMaskNone>(a, bwd_args(grad_loss, d_img, d_tex, d_alpha));
    return launch_status(fn);
}

// ---- dataset targets (uint8 / RGBA / mask) ---------------------------------------------------------------------
extern "C" int gstex_loss_target_fwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                                     const float* alpha, const float* background, const gstex_loss_target* target,
                                     const float* window, float ssim_lambda, float* rgb_out, float* gt_out,
                                     float* terms_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "gstex_loss_target_fwd";
    const char* bad = target_error(target);
    GSTEX_REQUIRE(!bad, "%s: %s", fn, bad);
    if (int rc = loss_check(fn, true, H, W, C, img && tex && alpha && background && window && terms_out, workspace,
                            workspace_bytes, gstex_loss_target_workspace_size(H, W)))
        return rc;
    const LossLaunch a = loss_launch(H, W, C, img, tex, alpha, background, target->gt, target->mask, window,
                                     ssim_lambda, workspace, 3, stream);
    dispatch_target(*target, a, FwdOut{rgb_out, gt_out});
    launch_reduce<3>(a, LossFinish{a.inv_n1, a.inv_np, a.w_l1, a.w_ssim}, terms_out);
    return launch_status(fn);
}

extern "C" int gstex_loss_target_bwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                                     const float* alpha, const float* background, const gstex_loss_target* target,
                                     const float* window, float ssim_lambda, const float* grad_loss, float* d_img,
                                     float* d_tex, float* d_alpha, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const char* fn = "gstex_loss_target_bwd";
    const char* bad = target_error(target);
    GSTEX_REQUIRE(!bad, "%s: %s", fn, bad);
    if (int rc = loss_check(fn, false, H, W, C,
                            img && tex && alpha && background && window && grad_loss && d_img && d_tex && d_alpha,
                            workspace, workspace_bytes, gstex_loss_target_workspace_size(H, W)))
        return rc;
    GSTEX_REQUIRE(d_tex != d_img || C == 3, "%s: d_tex may be d_img only with C == 3 (got %d)", fn, C);
    const LossLaunch a = loss_launch(H, W, C, img, tex, alpha, background, target->gt, target->mask, window,
                                     ssim_lambda, workspace, 3, stream);
    dispatch_target(*target, a, bwd_args(grad_loss, d_img, d_tex, d_alpha));
    return launch_status(fn);
}

// ---- evaluation metrics ----------------------------------------------------------------------------------------
extern "C" int gstex_eval_metrics(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                                  const float* alpha, const float* background, const gstex_loss_target* target,
                                  const float* window, float* rgb_out, uint8_t* rgb_u8_out, float* gt_out,
                                  float* metrics_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "gstex_eval_metrics";
    // the reference's evaluation applies no mask: a descriptor that carries one is a caller's mistake, not ignored
    const char* bad = target && target->gt && target->mask ? "a mask is not supported (the evaluation applies none)"
                                                           : target_error(target);
    GSTEX_REQUIRE(!bad, "%s: %s", fn, bad);
    if (int rc = loss_check(fn, true, H, W, C, img && tex && alpha && background && window && metrics_out, workspace,
                            workspace_bytes, gstex_eval_metrics_workspace_size(H, W)))
        return rc;
    LossLaunch a = loss_launch(H, W, C, img, tex, alpha, background, target->gt, nullptr, window, 0.0f, workspace,
                               kMetricParts, stream);
    a.gmaps = nullptr;  // its workspace ends with the partial records
    dispatch_target(*target, a, MetricsOut{rgb_out, rgb_u8_out, gt_out});
    launch_reduce<kMetricParts>(a, MetricsFinish{a.inv_n1, a.inv_np}, metrics_out);
    return launch_status(fn);
}
