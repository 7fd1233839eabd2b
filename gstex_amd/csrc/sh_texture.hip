// sh_texture.hip — spherical-harmonics colour and jagged-texture resampling.
//
//   gstex_sh_fwd / gstex_sh_bwd      <- gstex_cuda.sh.spherical_harmonics (gstex.py:1109,1111;
//                                       exporter.py:40).  Real SH basis of the gsplat-0.1 lineage,
//                                       degree <= 4, result WITHOUT the +0.5 offset (the caller
//                                       zeroes the DC term, gstex.py:1100).  gstex_sh_bwd: the gradient
//                                       w.r.t. the coefficients (the reference detaches viewdirs).
//   gstex_sh_dirs_bwd                   the gradient w.r.t. viewdirs, for camera pose refinement
//                                       (both coefficient layouts).
//   gstex_texture_sample(_bwd)       <- gstex_cuda.texture_sample.texture_sample
//                                       (models/jagged_texture.py:138): bilinear resample of each
//                                       splat's old texel block at new texel-centre UVs, with the
//                                       same sampler the rasterizer uses (gstex_common.h).
#include "gstex_common.h"
#include "gstex_error.h"
#include "splat_math.h"  // sh_basis, sh_colour

using namespace gstex;

namespace {

// coeffs[i][k - k0] holds basis k (k0 = 1: the DC coefficient is implicitly zero, gstex.py:1100 zeroes it;
// starting the sum at +0 without the zero DC product gives the same bits as with it)
__global__ __launch_bounds__(256) void sh_fwd_kernel(int n, int degree, int k0, int K, const float* __restrict__ dirs,
                                                     const float* __restrict__ coeffs, float* __restrict__ out) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float b[25];
    sh_basis(degree, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], b);
    const int nb = (degree + 1) * (degree + 1);
    const float* c = coeffs + (size_t)i * K * 3 - 3 * k0;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int k = k0; k < nb; ++k) {
        r0 = r0 + b[k] * c[3 * k];
        r1 = r1 + b[k] * c[3 * k + 1];
        r2 = r2 + b[k] * c[3 * k + 2];
    }
    out[3 * i] = r0;
    out[3 * i + 1] = r1;
    out[3 * i + 2] = r2;
}

__global__ __launch_bounds__(256) void sh_bwd_kernel(int n, int degree, int k0, int K, const float* __restrict__ dirs,
                                                     const float* __restrict__ v_out, float* __restrict__ v_coeffs) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    sh_grad_row(degree, k0, K, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], v_out[3 * i], v_out[3 * i + 1],
                v_out[3 * i + 2], v_coeffs + (size_t)i * K * 3);
}

// The same two kernels with the coefficient rows staged through LDS: a workgroup's 128 splats own one
// contiguous span of coefficients, read (forward) or written (backward) with consecutive lanes on
// consecutive words; the per-thread strided rows (180 B apart at K = 15) made every load instruction
// touch 64 cache lines.  Same arithmetic and order as above.  Used for K <= kShStagedMaxK.  The span is
// copied whole (rows of 3K words, also when the degree uses fewer) as 16-B vectors, several in flight per
// thread, when it is 16-B aligned (the scalar copy with a division per word was the kernels' latency chain).
constexpr int kShBlock = 128;
constexpr int kShStagedMaxK = 25;

__global__ __launch_bounds__(kShBlock) void sh_fwd_staged_kernel(int n, int degree, int k0, int K,
                                                                const float* __restrict__ dirs,
                                                                const float* __restrict__ coeffs,
                                                                float* __restrict__ out) {
    extern __shared__ float s_c[];
    const int t = threadIdx.x;
    const int i0 = blockIdx.x * kShBlock;
    const int cnt = min(kShBlock, n - i0);
    const int kw = K * 3;  // words per splat row
    sh_copy_span<kShBlock>(s_c, coeffs + (size_t)i0 * kw, cnt * kw);
    __syncthreads();
    if (t >= cnt) return;
    const int i = i0 + t;
    float r0, r1, r2;
    sh_colour(degree, k0, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], s_c + t * kw - 3 * k0, r0, r1, r2);
    out[3 * i] = r0;
    out[3 * i + 1] = r1;
    out[3 * i + 2] = r2;
}

__global__ __launch_bounds__(kShBlock) void sh_bwd_staged_kernel(int n, int degree, int k0, int K,
                                                                const float* __restrict__ dirs,
                                                                const float* __restrict__ v_out,
                                                                float* __restrict__ v_coeffs) {
    extern __shared__ float s_c[];
    const int t = threadIdx.x;
    const int i0 = blockIdx.x * kShBlock;
    const int cnt = min(kShBlock, n - i0);
    const int kw = K * 3;
    if (t < cnt) {
        const int i = i0 + t;
        sh_grad_row(degree, k0, K, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], v_out[3 * i], v_out[3 * i + 1],
                    v_out[3 * i + 2], s_c + t * kw);
    }
    __syncthreads();
    sh_copy_span<kShBlock>(v_coeffs + (size_t)i0 * kw, s_c, cnt * kw);
}

// The view-direction gradient (gstex_sh_dirs_bwd): G = sum_k (sum_c g_c coeffs[k][c]) dY_k/d(x, y, z) at the unit
// direction the forward evaluates the basis at, then through the normalisation d = dir / |dir|: (G - d (d . G)) / |dir|.
// fp64 per splat: the polynomial gradient is mostly radial, and the projection cancels that part.
constexpr double kC1 = 0.4886025119029199;
constexpr double kC2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                           0.5462742152960396};
constexpr double kC3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                           -0.4570457994644658, 1.445305721320277, -0.5900435899266435};
constexpr double kC4[9] = {2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892,
                           0.10578554691520431, -0.6690465435572892, 0.47308734787878004, -1.7701307697799304,
                           0.6258357354491761};

__global__ __launch_bounds__(256) void sh_dirs_bwd_kernel(int n, int degree, int k0, int K,
                                                          const float* __restrict__ dirs,
                                                          const float* __restrict__ coeffs,
                                                          const float* __restrict__ v_out,
                                                          float* __restrict__ v_dirs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (degree < 1) {  // the DC basis is constant
        v_dirs[3 * i] = v_dirs[3 * i + 1] = v_dirs[3 * i + 2] = 0.f;
        return;
    }
    const double dx = dirs[3 * i], dy = dirs[3 * i + 1], dz = dirs[3 * i + 2];
    const double nrm = sqrt((dx * dx + dy * dy) + dz * dz);
    const double x = dx / nrm, y = dy / nrm, z = dz / nrm;
    const double g0 = v_out[3 * i], g1 = v_out[3 * i + 1], g2 = v_out[3 * i + 2];
    const float* c = coeffs + (size_t)i * K * 3 - 3 * k0;  // indexed from basis 0 (k >= 1 only is read)
    double Gx = 0.0, Gy = 0.0, Gz = 0.0;
    // basis k's weight s = sum_c g_c coeffs[k][c] times its gradient (ax, ay, az)
    auto add = [&](int k, double ax, double ay, double az) {
        const double s = (g0 * (double)c[3 * k] + g1 * (double)c[3 * k + 1]) + g2 * (double)c[3 * k + 2];
        Gx += s * ax; Gy += s * ay; Gz += s * az;
    };
    add(1, 0.0, -kC1, 0.0);
    add(2, 0.0, 0.0, kC1);
    add(3, -kC1, 0.0, 0.0);
    if (degree >= 2) {
        add(4, kC2[0] * y, kC2[0] * x, 0.0);
        add(5, 0.0, kC2[1] * z, kC2[1] * y);
        add(6, kC2[2] * (-2.0 * x), kC2[2] * (-2.0 * y), kC2[2] * (4.0 * z));
        add(7, kC2[3] * z, 0.0, kC2[3] * x);
        add(8, kC2[4] * (2.0 * x), kC2[4] * (-2.0 * y), 0.0);
    }
    if (degree >= 3) {
        const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        add(9, kC3[0] * (6.0 * xy), kC3[0] * (3.0 * xx - 3.0 * yy), 0.0);
        add(10, kC3[1] * yz, kC3[1] * xz, kC3[1] * xy);
        add(11, kC3[2] * (-2.0 * xy), kC3[2] * ((4.0 * zz - xx) - 3.0 * yy), kC3[2] * (8.0 * yz));
        add(12, kC3[3] * (-6.0 * xz), kC3[3] * (-6.0 * yz), kC3[3] * ((6.0 * zz - 3.0 * xx) - 3.0 * yy));
        add(13, kC3[4] * ((4.0 * zz - 3.0 * xx) - yy), kC3[4] * (-2.0 * xy), kC3[4] * (8.0 * xz));
        add(14, kC3[5] * (2.0 * xz), kC3[5] * (-2.0 * yz), kC3[5] * (xx - yy));
        add(15, kC3[6] * (3.0 * xx - 3.0 * yy), kC3[6] * (-6.0 * xy), 0.0);
    }
    if (degree >= 4) {
        const double xx = x * x, yy = y * y, zz = z * z, xy = x * y;
        const double s71 = 7.0 * zz - 1.0, s73 = 7.0 * zz - 3.0;
        add(16, kC4[0] * y * (3.0 * xx - yy), kC4[0] * x * (xx - 3.0 * yy), 0.0);
        add(17, kC4[1] * (6.0 * xy * z), kC4[1] * z * (3.0 * xx - 3.0 * yy), kC4[1] * y * (3.0 * xx - yy));
        add(18, kC4[2] * y * s71, kC4[2] * x * s71, kC4[2] * (14.0 * xy * z));
        add(19, 0.0, kC4[3] * z * s73, kC4[3] * y * (21.0 * zz - 3.0));
        add(20, 0.0, 0.0, kC4[4] * z * (140.0 * zz - 60.0));
        add(21, kC4[5] * z * s73, 0.0, kC4[5] * x * (21.0 * zz - 3.0));
        add(22, kC4[6] * (2.0 * x) * s71, kC4[6] * (-2.0 * y) * s71, kC4[6] * (14.0 * z) * (xx - yy));
        add(23, kC4[7] * z * (3.0 * xx - 3.0 * yy), kC4[7] * (-6.0 * xy * z), kC4[7] * x * (xx - 3.0 * yy));
        add(24, kC4[8] * x * (4.0 * xx - 12.0 * yy), kC4[8] * y * (4.0 * yy - 12.0 * xx), 0.0);
    }
    const double rad = (x * Gx + y * Gy) + z * Gz;
    v_dirs[3 * i] = (float)((Gx - x * rad) / nrm);
    v_dirs[3 * i + 1] = (float)((Gy - y * rad) / nrm);
    v_dirs[3 * i + 2] = (float)((Gz - z * rad) / nrm);
}

// One thread per (query, channel-group): query q reads its 4 corner texels.
__global__ __launch_bounds__(256) void texture_sample_kernel(long long nq, int C, const int32_t* __restrict__ qd,
                                                             const float* __restrict__ tex,
                                                             const float* __restrict__ uv, float* __restrict__ out) {
    long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const int h = qd[3 * q], w = qd[3 * q + 1], off = qd[3 * q + 2];
    float* o = out + q * C;
    if (h * w <= 0) {
        for (int c = 0; c < C; ++c) o[c] = 0.0f;
        return;
    }
    const Bilerp b = bilerp_coords(uv[2 * q], uv[2 * q + 1], h, w);
    const size_t o00 = (size_t)(off + b.i0 * w + b.j0) * C, o01 = (size_t)(off + b.i0 * w + b.j1) * C;
    const size_t o10 = (size_t)(off + b.i1 * w + b.j0) * C, o11 = (size_t)(off + b.i1 * w + b.j1) * C;
    for (int c = 0; c < C; ++c) o[c] = bilerp_mix(tex[o00 + c], tex[o01 + c], tex[o10 + c], tex[o11 + c], b.ax, b.ay);
}

__global__ __launch_bounds__(256) void texture_sample_bwd_kernel(long long nq, int C, const int32_t* __restrict__ qd,
                                                                 const float* __restrict__ uv,
                                                                 const float* __restrict__ v_out,
                                                                 float* __restrict__ v_tex) {
    long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const int h = qd[3 * q], w = qd[3 * q + 1], off = qd[3 * q + 2];
    if (h * w <= 0) return;
    const Bilerp b = bilerp_coords(uv[2 * q], uv[2 * q + 1], h, w);
    const size_t o00 = (size_t)(off + b.i0 * w + b.j0) * C, o01 = (size_t)(off + b.i0 * w + b.j1) * C;
    const size_t o10 = (size_t)(off + b.i1 * w + b.j0) * C, o11 = (size_t)(off + b.i1 * w + b.j1) * C;
    const float w00 = (1.0f - b.ax) * (1.0f - b.ay), w01 = (1.0f - b.ax) * b.ay;
    const float w10 = b.ax * (1.0f - b.ay), w11 = b.ax * b.ay;
    for (int c = 0; c < C; ++c) {
        const float g = v_out[q * C + c];
        atomicAdd(v_tex + o00 + c, g * w00);
        atomicAdd(v_tex + o01 + c, g * w01);
        atomicAdd(v_tex + o10 + c, g * w10);
        atomicAdd(v_tex + o11 + c, g * w11);
    }
}

}  // namespace

extern "C" int gstex_sh_fwd(int32_t n, int32_t degree, int32_t n_coeffs, const float* viewdirs, const float* coeffs,
                            float* colors, void* stream) {
    GSTEX_REQUIRE(n >= 0 && degree >= 0 && degree <= 4, "gstex_sh_fwd: degree must be in [0, 4] (got %d)", degree);
    GSTEX_REQUIRE(n_coeffs >= (degree + 1) * (degree + 1), "gstex_sh_fwd: %d coefficients < (degree+1)^2 = %d",
                  n_coeffs, (degree + 1) * (degree + 1));
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(viewdirs && coeffs && colors, "gstex_sh_fwd: null pointer");
    if (n_coeffs <= kShStagedMaxK)
        sh_fwd_staged_kernel<<<div_up(n, kShBlock), kShBlock, (size_t)kShBlock * n_coeffs * 3 * sizeof(float),
                               as_stream(stream)>>>(n, degree, 0, n_coeffs, viewdirs, coeffs, colors);
    else
        sh_fwd_kernel<<<div_up(n, 256), 256, 0, as_stream(stream)>>>(n, degree, 0, n_coeffs, viewdirs, coeffs, colors);
    return launch_status("gstex_sh_fwd");
}

extern "C" int gstex_sh_bwd(int32_t n, int32_t degree, int32_t n_coeffs, const float* viewdirs,
                            const float* v_colors, float* v_coeffs, void* stream) {
    GSTEX_REQUIRE(n >= 0 && degree >= 0 && degree <= 4, "gstex_sh_bwd: degree must be in [0, 4]");
    GSTEX_REQUIRE(n_coeffs >= (degree + 1) * (degree + 1), "gstex_sh_bwd: too few coefficients");
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(viewdirs && v_colors && v_coeffs, "gstex_sh_bwd: null pointer");
    if (n_coeffs <= kShStagedMaxK)
        sh_bwd_staged_kernel<<<div_up(n, kShBlock), kShBlock, (size_t)kShBlock * n_coeffs * 3 * sizeof(float),
                               as_stream(stream)>>>(n, degree, 0, n_coeffs, viewdirs, v_colors, v_coeffs);
    else
        sh_bwd_kernel<<<div_up(n, 256), 256, 0, as_stream(stream)>>>(n, degree, 0, n_coeffs, viewdirs, v_colors, v_coeffs);
    return launch_status("gstex_sh_bwd");
}

extern "C" int gstex_sh_rest_fwd(int32_t n, int32_t degree, int32_t n_rest, const float* viewdirs,
                                 const float* coeffs_rest, float* colors, void* stream) {
    GSTEX_REQUIRE(n >= 0 && degree >= 0 && degree <= 4, "gstex_sh_rest_fwd: degree must be in [0, 4] (got %d)", degree);
    GSTEX_REQUIRE(n_rest >= (degree + 1) * (degree + 1) - 1, "gstex_sh_rest_fwd: %d coefficients < (degree+1)^2 - 1",
                  n_rest);
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(viewdirs && colors && (coeffs_rest || n_rest == 0), "gstex_sh_rest_fwd: null pointer");
    if (n_rest <= kShStagedMaxK)
        sh_fwd_staged_kernel<<<div_up(n, kShBlock), kShBlock, (size_t)kShBlock * n_rest * 3 * sizeof(float),
                               as_stream(stream)>>>(n, degree, 1, n_rest, viewdirs, coeffs_rest, colors);
    else
        sh_fwd_kernel<<<div_up(n, 256), 256, 0, as_stream(stream)>>>(n, degree, 1, n_rest, viewdirs, coeffs_rest, colors);
    return launch_status("gstex_sh_rest_fwd");
}

extern "C" int gstex_sh_rest_bwd(int32_t n, int32_t degree, int32_t n_rest, const float* viewdirs,
                                 const float* v_colors, float* v_coeffs_rest, void* stream) {
    GSTEX_REQUIRE(n >= 0 && degree >= 0 && degree <= 4, "gstex_sh_rest_bwd: degree must be in [0, 4]");
    GSTEX_REQUIRE(n_rest >= 0, "gstex_sh_rest_bwd: n_rest < 0");
    if (n == 0 || n_rest == 0) return GSTEX_OK;
    GSTEX_REQUIRE(viewdirs && v_colors && v_coeffs_rest, "gstex_sh_rest_bwd: null pointer");
    if (n_rest <= kShStagedMaxK)
        sh_bwd_staged_kernel<<<div_up(n, kShBlock), kShBlock, (size_t)kShBlock * n_rest * 3 * sizeof(float),
                               as_stream(stream)>>>(n, degree, 1, n_rest, viewdirs, v_colors, v_coeffs_rest);
    else
        sh_bwd_kernel<<<div_up(n, 256), 256, 0, as_stream(stream)>>>(n, degree, 1, n_rest, viewdirs, v_colors, v_coeffs_rest);
    return launch_status("gstex_sh_rest_bwd");
}

extern "C" int gstex_sh_dirs_bwd(int32_t n, int32_t degree, int32_t k0, int32_t n_coeffs, const float* viewdirs,
                                 const float* coeffs, const float* v_colors, float* v_viewdirs, void* stream) {
    GSTEX_REQUIRE(n >= 0 && degree >= 0 && degree <= 4, "gstex_sh_dirs_bwd: n < 0 or degree outside [0, 4]");
    GSTEX_REQUIRE(k0 == 0 || k0 == 1, "gstex_sh_dirs_bwd: k0 must be 0 (full layout) or 1 (rest layout) (got %d)", k0);
    GSTEX_REQUIRE(n_coeffs >= (degree + 1) * (degree + 1) - k0, "gstex_sh_dirs_bwd: %d coefficients < (degree+1)^2 - k0",
                  n_coeffs);
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(viewdirs && v_colors && v_viewdirs && (coeffs || degree == 0), "gstex_sh_dirs_bwd: null pointer");
    sh_dirs_bwd_kernel<<<div_up(n, 256), 256, 0, as_stream(stream)>>>(n, degree, k0, n_coeffs, viewdirs, coeffs,
                                                                       v_colors, v_viewdirs);
    return launch_status("gstex_sh_dirs_bwd");
}

extern "C" int gstex_texture_sample(int64_t n_query, int32_t channels, const int32_t* query_dims,
                                    const float* texture, int64_t n_texels, const float* uv, float* out,
                                    void* stream) {
    (void)n_texels;
    GSTEX_REQUIRE(n_query >= 0 && channels >= 1, "gstex_texture_sample: invalid arguments");
    if (n_query == 0) return GSTEX_OK;
    GSTEX_REQUIRE(query_dims && uv && out, "gstex_texture_sample: null pointer");
    texture_sample_kernel<<<div_up(n_query, 256), 256, 0, as_stream(stream)>>>(n_query, channels, query_dims, texture,
                                                                               uv, out);
    return launch_status("gstex_texture_sample");
}

extern "C" int gstex_texture_sample_bwd(int64_t n_query, int32_t channels, const int32_t* query_dims,
                                        int64_t n_texels, const float* uv, const float* v_out, float* v_texture,
                                        void* stream) {
    (void)n_texels;
    GSTEX_REQUIRE(n_query >= 0 && channels >= 1, "gstex_texture_sample_bwd: invalid arguments");
    if (n_query == 0) return GSTEX_OK;
    GSTEX_REQUIRE(query_dims && uv && v_out && v_texture, "gstex_texture_sample_bwd: null pointer");
    texture_sample_bwd_kernel<<<div_up(n_query, 256), 256, 0, as_stream(stream)>>>(n_query, channels, query_dims, uv,
                                                                                   v_out, v_texture);
    return launch_status("gstex_texture_sample_bwd");
}
