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
//                                       and SSIM against the composited target.  A forward-only sibling of the loss
//                                       forward (metrics_fwd_kernel, at the end of this file): no gmaps, no mask, no L1.
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

// the forward's partial record: {sum s, sum |X - Y|} or, for the dataset targets, three floats (+ sum (rgb - gt)^2)
template <bool EXT>
struct PartRecord {
    using type = float2;
};
template <>
struct PartRecord<true> {
    using type = float;
};

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
                                                       float* __restrict__ gmaps,
                                                       typename PartRecord<EXT>::type* __restrict__ part,
                                                       FwdExtra<EXT> ex) {
    __shared__ float s_x[kReg][kReg + 1], s_y[kReg][kReg + 1];
    __shared__ float s_h[5][kReg][kLT + 1];
    __shared__ float s_red[EXT ? 3 : 2][8];
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
    // rows: 26 x 16 horizontal filters of the five quantities (fused multiply-adds: the window sums need no fixed
    // operation order -- the loss and its gradient are compared with tolerances, only the composite bit for bit)
    for (int i = tid; i < kReg * kLT; i += 256) {
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
    __syncthreads();
    // columns + the SSIM map at this thread's position
    const int cy = tid >> 4, cx = tid & 15;
    const int py = y0 + cy, px = x0 + cx;
    float ssum = 0.f;
    if (py < Hv && px < Wv) {
#pragma clang fp contract(fast)
        float q[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k)
#pragma unroll
            for (int m = 0; m < 5; ++m) q[m] += win.w[k] * s_h[m][cy + k][cx];
        const float mu1 = q[0], mu2 = q[1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float s11 = q[2] - mu1_sq, s22 = q[3] - mu2_sq, s12 = q[4] - mu1_mu2;
        const float A = 2.0f * mu1_mu2 + kC1, B = 2.0f * s12 + kC2;
        const float Cc = mu1_sq + mu2_sq + kC1, D = s11 + s22 + kC2;
        const float cs = B / D;
        const float s = (A / Cc) * cs;
        ssum = s;
        // dS/d mu2 (through mu2, sigma2^2 = E[Y^2] - mu2^2, sigma12 = E[XY] - mu1 mu2), dS/dE[Y^2], dS/dE[XY]
        const float ds_dmu2 = s * (2.0f * mu1 / A - 2.0f * mu2 / Cc);
        const float ds_ds22 = -s / D;
        const float ds_ds12 = 2.0f * s / B;
        const size_t o = ((size_t)c * Hv + py) * Wv + px;
        const size_t plane = (size_t)3 * Hv * Wv;
        gmaps[o] = ds_dmu2 - 2.0f * mu2 * ds_ds22 - mu1 * ds_ds12;
        gmaps[plane + o] = ds_ds22;
        gmaps[2 * plane + o] = ds_ds12;
    }
    // workgroup sums (fixed order: wave reduce, then the 4 waves in order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ssum += __shfl_xor(ssum, off, 64);
        l1 += __shfl_xor(l1, off, 64);
        if constexpr (EXT) mse += __shfl_xor(mse, off, 64);
    }
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = ssum;
        s_red[1][tid >> 6] = l1;
        if constexpr (EXT) s_red[2][tid >> 6] = mse;
    }
    __syncthreads();
    if (tid == 0) {
        const int b = (lt.c * gridDim.y + lt.by) * gridDim.x + lt.bx;  // tile index: fixed reduction order
        const float ps = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
        const float pl = ((s_red[1][0] + s_red[1][1]) + s_red[1][2]) + s_red[1][3];
        if constexpr (EXT) {
            part[3 * b] = ps;
            part[3 * b + 1] = pl;
            part[3 * b + 2] = ((s_red[2][0] + s_red[2][1]) + s_red[2][2]) + s_red[2][3];
        } else {
            part[b] = make_float2(ps, pl);
        }
    }
}

__global__ __launch_bounds__(1024) void loss_reduce_kernel(int nparts, const float2* __restrict__ part, double inv_n1,
                                                           double inv_np, float w_l1, float w_ssim,
                                                           float* __restrict__ loss) {
    __shared__ double s_s[1024], s_l[1024];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 1024) {
        a += (double)part[i].x;
        b += (double)part[i].y;
    }
    s_s[threadIdx.x] = a;
    s_l[threadIdx.x] = b;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_s[threadIdx.x] += s_s[threadIdx.x + o];
            s_l[threadIdx.x] += s_l[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l1 = (float)(s_l[0] * inv_n1);
        const float ssim = (float)(s_s[0] * inv_np);
        loss[0] = w_l1 * l1 + w_ssim * (1.0f - ssim);
        loss[1] = l1;
        loss[2] = ssim;
    }
}

// the target path's reduction: three partials per workgroup, terms = {loss, L1, SSIM, MSE}
__global__ __launch_bounds__(1024) void loss_target_reduce_kernel(int nparts, const float* __restrict__ part,
                                                                  double inv_n1, double inv_np, float w_l1,
                                                                  float w_ssim, float* __restrict__ terms) {
    __shared__ double s_s[1024], s_l[1024], s_m[1024];
    double a = 0.0, b = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 1024) {
        a += (double)part[3 * i];
        b += (double)part[3 * i + 1];
        m += (double)part[3 * i + 2];
    }
    s_s[threadIdx.x] = a;
    s_l[threadIdx.x] = b;
    s_m[threadIdx.x] = m;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_s[threadIdx.x] += s_s[threadIdx.x + o];
            s_l[threadIdx.x] += s_l[threadIdx.x + o];
            s_m[threadIdx.x] += s_m[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l1 = (float)(s_l[0] * inv_n1);
        const float ssim = (float)(s_s[0] * inv_np);
        terms[0] = w_l1 * l1 + w_ssim * (1.0f - ssim);
        terms[1] = l1;
        terms[2] = ssim;
        terms[3] = (float)(s_m[0] * inv_n1);
    }
}

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
    for (int c = 0; c < C; ++c) d_tex[(size_t)C * pix + c] = c == 0 ? gch[0] : (c == 1 ? gch[1] : (c == 2 ? gch[2] : 0.0f));
    d_alpha[pix] = -((gch[0] * bg[0] + gch[1] * bg[1]) + gch[2] * bg[2]);
}

}  // namespace

using namespace gstex;

// forward: one workgroup per (tile, channel); backward: one per tile (its three channels in turn)
static int loss_grid(int H, int W, dim3& grid, int channels = 3) {
    grid = dim3((unsigned)((W + kLT - 1) / kLT), (unsigned)((H + kLT - 1) / kLT), (unsigned)channels);
    return (int)(grid.x * grid.y * grid.z);
}

// workspace: the forward's per-workgroup partial records (part_floats each), then the gmaps
static size_t loss_ws_size(int H, int W, int part_floats) {
    if (H <= kHalo || W <= kHalo) return 0;
    dim3 g;
    const size_t parts = (size_t)loss_grid(H, W, g) * part_floats * sizeof(float);
    const size_t gm = (size_t)3 * 3 * (H - kHalo) * (W - kHalo) * sizeof(float);
    return ((parts + 255) & ~(size_t)255) + gm;
}

static void loss_ws(int H, int W, int part_floats, void* ws, float** part, float** gmaps) {
    dim3 g;
    const size_t parts = (size_t)loss_grid(H, W, g) * part_floats * sizeof(float);
    char* b = (char*)ws;
    *part = (float*)b;
    b += (parts + 255) & ~(size_t)255;
    *gmaps = (float*)b;
}

extern "C" size_t gstex_loss_workspace_size(int32_t H, int32_t W) { return loss_ws_size(H, W, 2); }

extern "C" size_t gstex_loss_target_workspace_size(int32_t H, int32_t W) { return loss_ws_size(H, W, 3); }

extern "C" int gstex_loss_fwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                              const float* alpha, const float* background, const float* gt, const float* window,
                              float ssim_lambda, float* rgb_out, float* loss_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    GSTEX_REQUIRE(H > kHalo && W > kHalo, "gstex_loss_fwd: image must be larger than the %d-tap window (%dx%d)",
                  kWin, H, W);
    GSTEX_REQUIRE(C >= 3 && C <= 8, "gstex_loss_fwd: tex channels must be in [3, 8] (got %d)", C);
    GSTEX_REQUIRE(img && tex && alpha && background && gt && window && loss_out, "gstex_loss_fwd: null pointer");
    GSTEX_REQUIRE(workspace && workspace_bytes >= gstex_loss_workspace_size(H, W),
                  "gstex_loss_fwd: workspace too small");
    Win win;
    for (int k = 0; k < kWin; ++k) win.w[k] = window[k];  // host array
    float *part, *gmaps;
    loss_ws(H, W, 2, workspace, &part, &gmaps);
    dim3 grid;
    const int nparts = loss_grid(H, W, grid);
    hipStream_t st = as_stream(stream);
    loss_fwd_kernel<GSTEX_GT_F32, 3, kMaskNone, false><<<grid, 256, 0, st>>>(
        H, W, C, img, tex, alpha, background, gt, win, rgb_out, gmaps, (float2*)part, FwdExtra<false>{});
    loss_reduce_kernel<<<1, 1024, 0, st>>>(nparts, (const float2*)part, 1.0 / (3.0 * H * W),
                                           1.0 / (3.0 * (H - kHalo) * (W - kHalo)), 1.0f - ssim_lambda, ssim_lambda,
                                           loss_out);
    return launch_status("gstex_loss_fwd");
}

extern "C" int gstex_loss_bwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                              const float* alpha, const float* background, const float* gt, const float* window,
                              float ssim_lambda, const float* grad_loss, float* d_img, float* d_tex, float* d_alpha,
                              void* workspace, size_t workspace_bytes, void* stream) {
    GSTEX_REQUIRE(H > kHalo && W > kHalo, "gstex_loss_bwd: image must be larger than the %d-tap window", kWin);
    GSTEX_REQUIRE(C >= 3 && C <= 8, "gstex_loss_bwd: tex channels must be in [3, 8] (got %d)", C);
    GSTEX_REQUIRE(img && tex && alpha && background && gt && window && grad_loss && d_img && d_tex && d_alpha,
                  "gstex_loss_bwd: null pointer");
    GSTEX_REQUIRE(workspace && workspace_bytes >= gstex_loss_workspace_size(H, W),
                  "gstex_loss_bwd: workspace too small");
    Win win;
    for (int k = 0; k < kWin; ++k) win.w[k] = window[k];
    float *part, *gmaps;
    loss_ws(H, W, 2, workspace, &part, &gmaps);
    dim3 grid;
    loss_grid(H, W, grid, 1);
    hipStream_t st = as_stream(stream);
    const float k_l1 = (float)((1.0 - ssim_lambda) / (3.0 * H * W));
    const float k_ssim = (float)(ssim_lambda / (3.0 * (H - kHalo) * (W - kHalo)));
    loss_bwd_kernel<GSTEX_GT_F32, 3, kMaskNone><<<grid, 256, 0, st>>>(
        H, W, C, img, tex, alpha, background, gt, win, gmaps, grad_loss, k_l1, k_ssim, d_img, d_tex, d_alpha,
        BwdExtra<kMaskNone>{});
    return launch_status("gstex_loss_bwd");
}

// ---- dataset targets (uint8 / RGBA / mask) ---------------------------------------------------------------------
namespace {

struct FwdLaunch {
    dim3 grid;
    hipStream_t st;
    int H, W, C;
    const float *img, *tex, *alpha, *bg;
    const void *gt, *mask;
    Win win;
    float *rgb_out, *gt_out, *gmaps, *part;
};

struct BwdLaunch {
    dim3 grid;
    hipStream_t st;
    int H, W, C;
    const float *img, *tex, *alpha, *bg;
    const void *gt, *mask;
    Win win;
    const float *gmaps, *grad_loss;
    float k_l1, k_ssim;
    float *d_img, *d_tex, *d_alpha;
};

template <int DT, int CH, int MK>
void launch(const FwdLaunch& a) {
    loss_fwd_kernel<DT, CH, MK, true><<<a.grid, 256, 0, a.st>>>(a.H, a.W, a.C, a.img, a.tex, a.alpha, a.bg,
                                                                (GtPtr<DT>)a.gt, a.win,
                                                                a.rgb_out, a.gmaps, a.part,
                                                                FwdExtra<true>{a.mask, a.gt_out});
}

template <int DT, int CH, int MK>
void launch(const BwdLaunch& a) {
    BwdExtra<MK> ex;
    if constexpr (MK != kMaskNone) ex.mask = a.mask;
    loss_bwd_kernel<DT, CH, MK><<<a.grid, 256, 0, a.st>>>(a.H, a.W, a.C, a.img, a.tex, a.alpha, a.bg,
                                                          (GtPtr<DT>)a.gt, a.win,
                                                          a.gmaps, a.grad_loss, a.k_l1, a.k_ssim, a.d_img, a.d_tex,
                                                          a.d_alpha, ex);
}

template <int DT, int CH, class Args>
void dispatch_mask(int mk, const Args& a) {
    if (mk == kMaskNone) launch<DT, CH, kMaskNone>(a);
    else if (mk == kMaskF32) launch<DT, CH, kMaskF32>(a);
    else launch<DT, CH, kMaskBool>(a);
}

// the policy instantiation of a (validated) target descriptor
template <class Args>
void dispatch_target(const gstex_loss_target& t, const Args& a) {
    const int mk = !t.mask ? kMaskNone : (t.mask_dtype == GSTEX_MASK_BOOL ? kMaskBool : kMaskF32);
    if (t.gt_dtype == GSTEX_GT_U8) {
        if (t.gt_channels == 4) dispatch_mask<GSTEX_GT_U8, 4>(mk, a);
        else dispatch_mask<GSTEX_GT_U8, 3>(mk, a);
    } else {
        if (t.gt_channels == 4) dispatch_mask<GSTEX_GT_F32, 4>(mk, a);
        else dispatch_mask<GSTEX_GT_F32, 3>(mk, a);
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

extern "C" int gstex_loss_target_fwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                                     const float* alpha, const float* background, const gstex_loss_target* target,
                                     const float* window, float ssim_lambda, float* rgb_out, float* gt_out,
                                     float* terms_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* bad = target_error(target);
    GSTEX_REQUIRE(!bad, "gstex_loss_target_fwd: %s", bad);
    GSTEX_REQUIRE(H > kHalo && W > kHalo,
                  "gstex_loss_target_fwd: image must be larger than the %d-tap window (%dx%d)", kWin, H, W);
    GSTEX_REQUIRE(C >= 3 && C <= 8, "gstex_loss_target_fwd: tex channels must be in [3, 8] (got %d)", C);
    GSTEX_REQUIRE(img && tex && alpha && background && window && terms_out, "gstex_loss_target_fwd: null pointer");
    GSTEX_REQUIRE(workspace && workspace_bytes >= gstex_loss_target_workspace_size(H, W),
                  "gstex_loss_target_fwd: workspace too small");
    FwdLaunch a;
    a.st = as_stream(stream);
    a.H = H, a.W = W, a.C = C;
    a.img = img, a.tex = tex, a.alpha = alpha, a.bg = background;
    a.gt = target->gt, a.mask = target->mask;
    for (int k = 0; k < kWin; ++k) a.win.w[k] = window[k];  // host array
    a.rgb_out = rgb_out, a.gt_out = gt_out;
    loss_ws(H, W, 3, workspace, &a.part, &a.gmaps);
    const int nparts = loss_grid(H, W, a.grid);
    dispatch_target(*target, a);
    loss_target_reduce_kernel<<<1, 1024, 0, a.st>>>(nparts, a.part, 1.0 / (3.0 * H * W),
                                                    1.0 / (3.0 * (H - kHalo) * (W - kHalo)), 1.0f - ssim_lambda,
                                                    ssim_lambda, terms_out);
    return launch_status("gstex_loss_target_fwd");
}

extern "C" int gstex_loss_target_bwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                                     const float* alpha, const float* background, const gstex_loss_target* target,
                                     const float* window, float ssim_lambda, const float* grad_loss, float* d_img,
                                     float* d_tex, float* d_alpha, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const char* bad = target_error(target);
    GSTEX_REQUIRE(!bad, "gstex_loss_target_bwd: %s", bad);
    GSTEX_REQUIRE(H > kHalo && W > kHalo, "gstex_loss_target_bwd: image must be larger than the %d-tap window", kWin);
    GSTEX_REQUIRE(C >= 3 && C <= 8, "gstex_loss_target_bwd: tex channels must be in [3, 8] (got %d)", C);
    GSTEX_REQUIRE(img && tex && alpha && background && window && grad_loss && d_img && d_tex && d_alpha,
                  "gstex_loss_target_bwd: null pointer");
    GSTEX_REQUIRE(workspace && workspace_bytes >= gstex_loss_target_workspace_size(H, W),
                  "gstex_loss_target_bwd: workspace too small");
    BwdLaunch a;
    a.st = as_stream(stream);
    a.H = H, a.W = W, a.C = C;
    a.img = img, a.tex = tex, a.alpha = alpha, a.bg = background;
    a.gt = target->gt, a.mask = target->mask;
    for (int k = 0; k < kWin; ++k) a.win.w[k] = window[k];
    float* part;
    float* gmaps;
    loss_ws(H, W, 3, workspace, &part, &gmaps);
    a.gmaps = gmaps;
    a.grad_loss = grad_loss;
    a.k_l1 = (float)((1.0 - ssim_lambda) / (3.0 * H * W));
    a.k_ssim = (float)(ssim_lambda / (3.0 * (H - kHalo) * (W - kHalo)));
    a.d_img = d_img, a.d_tex = d_tex, a.d_alpha = d_alpha;
    loss_grid(H, W, a.grid, 1);
    dispatch_target(*target, a);
    return launch_status("gstex_loss_target_bwd");
}

// ---- evaluation metrics (uint8-quantised PSNR / SSIM, forward only) ----------------------------------------------
namespace {

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
    __shared__ float s_red[kMetricParts][4];
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
    // rows, then columns: the loss forward's filters (fused multiply-adds: SSIM is compared with a tolerance)
    for (int i = tid; i < kReg * kLT; i += 256) {
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
    __syncthreads();
    const int cy = tid >> 4, cx = tid & 15;
    const int py = y0 + cy, px = x0 + cx;
    float ssum = 0.f;
    if (py < Hv && px < Wv) {
#pragma clang fp contract(fast)
        float q[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k)
#pragma unroll
            for (int m = 0; m < 5; ++m) q[m] += win.w[k] * s_h[m][cy + k][cx];
        const float mu1 = q[0], mu2 = q[1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float s11 = q[2] - mu1_sq, s22 = q[3] - mu2_sq, s12 = q[4] - mu1_mu2;
        const float A = 2.0f * mu1_mu2 + kC1, B = 2.0f * s12 + kC2;
        const float Cc = mu1_sq + mu2_sq + kC1, D = s11 + s22 + kC2;
        ssum = (A / Cc) * (B / D);
    }
    // workgroup sums (fixed order: wave reduce, then the 4 waves in order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ssum += __shfl_xor(ssum, off, 64);
        mse += __shfl_xor(mse, off, 64);
        mse_raw += __shfl_xor(mse_raw, off, 64);
    }
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = ssum;
        s_red[1][tid >> 6] = mse;
        s_red[2][tid >> 6] = mse_raw;
    }
    __syncthreads();
    if (tid == 0) {
        const int b = (lt.c * gridDim.y + lt.by) * gridDim.x + lt.bx;  // tile index: fixed reduction order
#pragma unroll
        for (int m = 0; m < kMetricParts; ++m)
            part[kMetricParts * b + m] = ((s_red[m][0] + s_red[m][1]) + s_red[m][2]) + s_red[m][3];
    }
}

// metrics = {PSNR, SSIM, MSE, MSE_raw}; PSNR = -10 log10(MSE) (+inf when every byte equals its target)
__global__ __launch_bounds__(1024) void metrics_reduce_kernel(int nparts, const float* __restrict__ part,
                                                              double inv_n1, double inv_np,
                                                              float* __restrict__ metrics) {
    __shared__ double s_s[1024], s_m[1024], s_r[1024];
    double a = 0.0, m = 0.0, r = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 1024) {
        a += (double)part[kMetricParts * i];
        m += (double)part[kMetricParts * i + 1];
        r += (double)part[kMetricParts * i + 2];
    }
    s_s[threadIdx.x] = a;
    s_m[threadIdx.x] = m;
    s_r[threadIdx.x] = r;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_s[threadIdx.x] += s_s[threadIdx.x + o];
            s_m[threadIdx.x] += s_m[threadIdx.x + o];
            s_r[threadIdx.x] += s_r[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float mse = (float)(s_m[0] * inv_n1);
        metrics[0] = -10.0f * log10f(mse);
        metrics[1] = (float)(s_s[0] * inv_np);
        metrics[2] = mse;
        metrics[3] = (float)(s_r[0] * inv_n1);
    }
}

template <int DT, int CH>
void launch_metrics(const FwdLaunch& a, unsigned char* rgb_u8_out) {
    metrics_fwd_kernel<DT, CH><<<a.grid, 256, 0, a.st>>>(a.H, a.W, a.C, a.img, a.tex, a.alpha, a.bg, (GtPtr<DT>)a.gt,
                                                         a.win, a.rgb_out, rgb_u8_out, a.gt_out, a.part);
}

}  // namespace

// workspace: the forward's per-workgroup partial records, nothing else
extern "C" size_t gstex_eval_metrics_workspace_size(int32_t H, int32_t W) {
    if (H <= kHalo || W <= kHalo) return 0;
    dim3 g;
    return (size_t)loss_grid(H, W, g) * kMetricParts * sizeof(float);
}

extern "C" int gstex_eval_metrics(int32_t H, int32_t W, int32_t C, const float* img, const float* tex,
                                  const float* alpha, const float* background, const gstex_loss_target* target,
                                  const float* window, float* rgb_out, uint8_t* rgb_u8_out, float* gt_out,
                                  float* metrics_out, void* workspace, size_t workspace_bytes, void* stream) {
    // the reference's evaluation applies no mask: a descriptor that carries one is a caller's mistake, not ignored
    const char* bad = target && target->gt && target->mask ? "a mask is not supported (the evaluation applies none)"
                                                           : target_error(target);
    GSTEX_REQUIRE(!bad, "gstex_eval_metrics: %s", bad);
    GSTEX_REQUIRE(H > kHalo && W > kHalo, "gstex_eval_metrics: image must be larger than the %d-tap window (%dx%d)",
                  kWin, H, W);
    GSTEX_REQUIRE(C >= 3 && C <= 8, "gstex_eval_metrics: tex channels must be in [3, 8] (got %d)", C);
    GSTEX_REQUIRE(img && tex && alpha && background && window && metrics_out, "gstex_eval_metrics: null pointer");
    GSTEX_REQUIRE(workspace && workspace_bytes >= gstex_eval_metrics_workspace_size(H, W),
                  "gstex_eval_metrics: workspace too small");
    FwdLaunch a;
    a.st = as_stream(stream);
    a.H = H, a.W = W, a.C = C;
    a.img = img, a.tex = tex, a.alpha = alpha, a.bg = background;
    a.gt = target->gt, a.mask = nullptr;
    for (int k = 0; k < kWin; ++k) a.win.w[k] = window[k];  // host array
    a.rgb_out = rgb_out, a.gt_out = gt_out;
    a.gmaps = nullptr;
    a.part = (float*)workspace;
    const int nparts = loss_grid(H, W, a.grid);
    if (target->gt_dtype == GSTEX_GT_U8) {
        if (target->gt_channels == 4) launch_metrics<GSTEX_GT_U8, 4>(a, rgb_u8_out);
        else launch_metrics<GSTEX_GT_U8, 3>(a, rgb_u8_out);
    } else {
        if (target->gt_channels == 4) launch_metrics<GSTEX_GT_F32, 4>(a, rgb_u8_out);
        else launch_metrics<GSTEX_GT_F32, 3>(a, rgb_u8_out);
    }
    metrics_reduce_kernel<<<1, 1024, 0, a.st>>>(nparts, a.part, 1.0 / (3.0 * H * W),
                                                1.0 / (3.0 * (H - kHalo) * (W - kHalo)), metrics_out);
    return launch_status("gstex_eval_metrics");
}
