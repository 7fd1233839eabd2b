// raster_common.h — what the raster units (raster_fwd.hip, raster_bwd.hip, raster_edit.hip) share: the splat record
// as the kernels read it, the per-wave cull, the per-(pixel, splat) evaluation, the texel loaders, the layout of the
// aux buffer the forward writes for the backward (one definition, read by both) and the entry points' argument checks.
// Semantics: SURVEY.md Appendix A and the comments of gstex_common.h; the CPU restatement is oracle/raster.py.
//
// Only the tunables that more than one kernel reads are here; a kernel's own live in its file.
#pragma once

#include "gstex_common.h"
#include "gstex_error.h"
#include "splat_math.h"  // splat_record
#include <cfloat>

namespace gstex {

constexpr int kThreads = kTilePixels;  // 256
#ifndef GSTEX_FWD_BATCH
#define GSTEX_FWD_BATCH 128
#endif
#ifndef GSTEX_FAST_RCP
#define GSTEX_FAST_RCP 1  // v_rcp_f32 for backward divisions that feed no threshold decision
#endif
#ifndef GSTEX_FAST_EVAL
#define GSTEX_FAST_EVAL 1  // hardware v_exp_f32 / v_rcp_f32 in the pair evaluation (0: expf sequence, IEEE division)
#endif
constexpr int kFwdBatch = GSTEX_FWD_BATCH;
constexpr int kRecF4 = GSTEX_REC_FLOATS / 4;  // 8 float4 per record

// ------------------------------------------------------------------------------------------
// shared per-(pixel, splat) evaluation
// ------------------------------------------------------------------------------------------
struct Rec {
    f3 A, B, Tw;
    float Pz;
    float x, y, opac, mark;  // opac = |R_OPAC|; mark = the raw word (sign bit: near edge-on, gstex_common.h kHpCos)
    float rgb[3], nrm[3];
    float tu0, auu, auv, tv0, avu, avv;
    int h, w, off;
    float xa, ya;
    float hm1, wm1;  // (float)(h - 1), (float)(w - 1)
};

// Record fields from its 8 float4 planes (gstex_common.h RecField)
__device__ __forceinline__ Rec rec_from_planes(float4 a, float4 b, float4 c, float4 d, float4 e, float4 f, float4 g,
                                               float4 q) {
    const float v[GSTEX_REC_FLOATS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w,
                                       e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w, g.x, g.y, g.z, g.w, q.x, q.y, q.z, q.w};
    Rec r;
    r.A = f3{v[R_A], v[R_A + 1], v[R_A + 2]};
    r.B = f3{v[R_B], v[R_B + 1], v[R_B + 2]};
    r.Pz = v[R_PZ];
    r.Tw = f3{v[R_TW], v[R_TW + 1], v[R_TW + 2]};
    r.x = v[R_XY]; r.y = v[R_XY + 1];
    r.opac = fabsf(v[R_OPAC]);
    r.mark = v[R_OPAC];
    r.rgb[0] = v[R_RGB]; r.rgb[1] = v[R_RGB + 1]; r.rgb[2] = v[R_RGB + 2];
    r.tu0 = v[R_TU0]; r.auu = v[R_AUU]; r.auv = v[R_AUV]; r.tv0 = v[R_TV0]; r.avu = v[R_AVU]; r.avv = v[R_AVV];
    r.h = __float_as_int(v[R_H]); r.w = __float_as_int(v[R_W]); r.off = __float_as_int(v[R_OFF]);
    r.xa = v[R_XA]; r.ya = v[R_YA];
    r.nrm[0] = v[R_NRM]; r.nrm[1] = v[R_NRM + 1]; r.nrm[2] = v[R_NRM + 2];
    r.hm1 = v[R_HM1]; r.wm1 = v[R_WM1];
    return r;
}

// Pixel of thread tid inside a 16x16 tile and the wave's block of pixel centres.
struct WaveBlock { int px, py; float wx0, wx1, wy0, wy1; };  // w*: the cull box (pixel centres +- 0.05)
__device__ __forceinline__ WaveBlock wave_block(int tx, int ty, int tid) {
    WaveBlock b;
    const int w = tid >> 6, l = tid & 63;
    b.px = tx * kTile + (w & 1) * 8 + (l & 7);  // wave w covers the 8x8 quadrant (w & 1, w >> 1)
    b.py = ty * kTile + (w >> 1) * 8 + (l >> 3);
    // the cull box is wave-uniform: held in SGPRs (as VGPRs its four bounds were the allocator's first spill
    // candidates, reloaded from scratch by every record's cull test)
    auto uni = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
    const float x0 = (float)(tx * kTile + (w & 1) * 8) + 0.5f, y0 = (float)(ty * kTile + (w >> 1) * 8) + 0.5f;
    b.wx0 = uni(x0 - 0.05f);
    b.wy0 = uni(y0 - 0.05f);
    b.wx1 = uni((x0 + 7.0f) + 0.05f);
    b.wy1 = uni((y0 + 7.0f) + 0.05f);
    return b;
}

// Record j of a batch staged in LDS as [plane][splat] float4
template <int NB>
__device__ __forceinline__ Rec read_rec(const float4* s, int j) {
    return rec_from_planes(s[0 * NB + j], s[1 * NB + j], s[2 * NB + j], s[3 * NB + j], s[4 * NB + j], s[5 * NB + j],
                           s[6 * NB + j], s[7 * NB + j]);
}

// Visit-mask layout: tile t owns 64-bit words [ceil(start_t / 64) + t, + ceil(len_t / 64)) (disjoint across tiles);
// word i holds, for each of the 4 waves (interleaved: word * 4 + wave), one bit per tile-list position
// 64 i .. 64 i + 63: the forward's per-wave cull (the splat's contribution region meets the wave's block).
__host__ __device__ __forceinline__ size_t visit_mask_base(int start, int tile) {
    return (size_t)((start + 63) / 64) + (size_t)tile;
}

// Backward units: the backward splits each (tile, 8x8 quadrant) list at every kSegLen positions into segments, one
// wave each, so no wave walks more than kSegLen positions (a deep unit as one wave was the kernel's critical path).
// Segment k of tile t has slot seg_base(start_t, t) + k (disjoint across tiles, like the visit-mask words); unit =
// 4 slot + quadrant.  The forward records, per unit, the number of splats it evaluated (the backward's cost
// estimate and launch order), the tile of every slot, and per-pixel checkpoints: for each segment boundary it
// crosses with a lane still running, the state after the segment (T and the colour / texture / depth / normal /
// distortion accumulators), and for a wave whose last contributor lies past the first segment, its final
// accumulators in the slot of that last segment.  The backward of segment k starts from checkpoint k instead of
// the final state: T = T_k, and R = (back half of sum_j w_j g_j + T_final bg-term) / T_k from the accumulators.
#ifndef GSTEX_SEG_LEN
#define GSTEX_SEG_LEN 256
#endif
constexpr int kSegLen = GSTEX_SEG_LEN;
static_assert(kSegLen % 128 == 0, "segments end at forward batch boundaries");
__host__ __device__ __forceinline__ int seg_base(int start, int tile) { return (start + kSegLen - 1) / kSegLen + tile; }
__host__ __device__ __forceinline__ int ck_fields(int C) { return 4 + C + 6; }  // T, img[3], tex[C], D, nrm[3], M1, M2

struct AuxPtrs {
    unsigned long long* masks;
    int32_t* cost;       // [n_units] evaluation count | XCD group (2x2-tile macro-block) << 24
    int32_t* order;      // [n_units] (written by the backward)
    int32_t* order_ws;   // gstex_unit_order scratch
    int32_t* slot_tile;  // [n_slots]
    float* ckpt;         // [n_units][F][64]
    int F;
};
struct AuxLayout { size_t masks, cost, order, order_ws, slot_tile, ckpt, bytes; int64_t n_slots, n_units; int F; };
struct ZeroBufs { float* p[2]; int64_t n[2]; };  // buffers a raster grid zeroes (zero_buf of gstex_raster_fwd / _bwd)
// The accumulation buffers a raster kernel's whole grid zeroes as a side job (gstex_raster_fwd's zero_buf / zero_buf2:
// the texel gradient and the splat-gradient sums of the backward that follows; gstex_raster_bwd's zero_buf: the next
// step's texel gradient):
// plain streaming stores the VALU-bound raster kernels hide, instead of fill passes (or an Adam update's zero stores)
__device__ __forceinline__ void zero_bufs(const ZeroBufs& zb) {
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        float* zp = zb.p[b];
        const int64_t zn = zb.n[b];
        if (!zp) continue;
        if ((reinterpret_cast<uintptr_t>(zp) & 15) == 0) {
            typedef float z4v __attribute__((ext_vector_type(4)));
            z4v* z4 = reinterpret_cast<z4v*>(zp);
            const z4v zero = {0.f, 0.f, 0.f, 0.f};
            for (int64_t i = t0; i < zn / 4; i += nthr) __builtin_nontemporal_store(zero, z4 + i);
            if (t0 < zn % 4) zp[zn / 4 * 4 + t0] = 0.0f;
        } else {
            for (int64_t i = t0; i < zn; i += nthr) zp[i] = 0.0f;
        }
    }
}
__host__ inline AuxLayout aux_layout(int64_t n_isect, int n_tiles, int C) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    AuxLayout a;
    a.n_slots = (n_isect + kSegLen - 1) / kSegLen + n_tiles + 1;
    a.n_units = a.n_slots * 4;
    a.F = ck_fields(C);
    size_t o = 0;
    a.masks = o; o = al(o + (((size_t)n_isect + 63) / 64 + (size_t)n_tiles + 1) * 4 * sizeof(uint64_t));
    a.cost = o; o = al(o + (size_t)a.n_units * 4);
    a.order = o; o = al(o + (size_t)a.n_units * 4);
    a.order_ws = o; o = al(o + gstex_unit_order_scratch_words() * 4);
    a.slot_tile = o; o = al(o + (size_t)a.n_slots * 4);
    a.ckpt = o; o = al(o + (size_t)a.n_units * a.F * 64 * sizeof(float));
    a.bytes = o;
    return a;
}
__host__ inline AuxPtrs aux_ptrs(void* aux, const AuxLayout& a) {
    char* b = (char*)aux;
    AuxPtrs p;
    p.masks = aux ? (unsigned long long*)(b + a.masks) : nullptr;
    p.cost = aux ? (int32_t*)(b + a.cost) : nullptr;
    p.order = aux ? (int32_t*)(b + a.order) : nullptr;
    p.order_ws = aux ? (int32_t*)(b + a.order_ws) : nullptr;
    p.slot_tile = aux ? (int32_t*)(b + a.slot_tile) : nullptr;
    p.ckpt = aux ? (float*)(b + a.ckpt) : nullptr;
    p.F = a.F;
    return p;
}

// The same record read from global memory at a wave-uniform address: scalar loads straight into SGPRs
// (no LDS read, no v_readfirstlane per value).
__device__ __forceinline__ Rec read_rec_global(const float4* __restrict__ rec) {
    return rec_from_planes(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7]);
}

// min over t in [lo, hi] of f(t) = |Q.xy + t A.xy|^2 - rm (Q.z + t A.z)^2 is <= 0?  (true when the slice
// is not convex in t: the conic is then not an ellipse there and nothing is culled)
__device__ __forceinline__ bool conic_edge(float ax, float ay, float az, float qx, float qy, float qz, float rm,
                                           float lo, float hi) {
    const float a = (ax * ax + ay * ay) - rm * (az * az);
    if (!(a > 0.0f)) return true;
    const float b = (qx * ax + qy * ay) - rm * (qz * az);
    const float t = fminf(fmaxf(-b / a, lo), hi);
    const float px = qx + t * ax, py = qy + t * ay, pz = qz + t * az;
    return (px * px + py * py) - rm * (pz * pz) <= 0.0f;
}

// Can splat j reach alpha >= 1/255 anywhere in the wave's block of pixel centres [wx0, wx1] x [wy0, wy1]?
// The homogeneous point is affine in the pixel offset d = pixel - anchor, p = d.x A + d.y B + (0, 0, Pz) (record
// planes 0-1), so the pair passes iff rho3 = |p.xy|^2 / p.z^2 <= rm = 2 ln(255 o) (or, with the AA filter, the
// disc 2 |pixel - centre|^2 <= rm): an ellipse (splats whose disc crosses the camera plane were culled
// upstream), tested exactly against the rectangle -- anchor inside, or an edge meeting it -- with a 1 %
// threshold margin and a 0.05 px larger rectangle, so the fp32 evaluation can never accept a pair the test
// rejected.
// (the cull fields are record dwords [0, 12): planes 0-2, RecField)
__device__ __forceinline__ bool may_hit_planes(float4 p0, float4 p1, float4 p2, float wx0, float wx1, float wy0,
                                               float wy1, bool aa) {
    const float v[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
    const float opac = fabsf(v[R_OPAC]);
    if (!(opac * 255.0f > 1.0f)) return false;
    const float rm = 2.0f * logf(255.0f * opac) * 1.01f + 1e-2f;
    const float x0 = wx0, x1 = wx1, y0 = wy0, y1 = wy1;  // (wave_block's cull box: already widened by 0.05)
    const float cx = v[R_XY], cy = v[R_XY + 1];
    if (aa) {
        const float ex = cx - fminf(fmaxf(cx, x0), x1), ey = cy - fminf(fmaxf(cy, y0), y1);
        if (2.0f * (ex * ex + ey * ey) <= rm) return true;
    }
    const float xa = v[R_XA], ya = v[R_YA];
    if (xa >= x0 && xa <= x1 && ya >= y0 && ya <= y1) return true;
    const float Ax = v[R_A], Ay = v[R_A + 1], Az = v[R_A + 2], Bx = v[R_B], By = v[R_B + 1], Bz = v[R_B + 2];
    const float Pz = v[R_PZ];
    const float dx0 = x0 - xa, dx1 = x1 - xa, dy0 = y0 - ya, dy1 = y1 - ya;
    return conic_edge(Ax, Ay, Az, dy0 * Bx, dy0 * By, Pz + dy0 * Bz, rm, dx0, dx1) ||
           conic_edge(Ax, Ay, Az, dy1 * Bx, dy1 * By, Pz + dy1 * Bz, rm, dx0, dx1) ||
           conic_edge(Bx, By, Bz, dx0 * Ax, dx0 * Ay, Pz + dx0 * Az, rm, dy0, dy1) ||
           conic_edge(Bx, By, Bz, dx1 * Ax, dx1 * Ay, Pz + dx1 * Az, rm, dy0, dy1);
}
template <int NB>
__device__ __forceinline__ bool wave_may_hit(const float4* s, int j, float wx0, float wx1, float wy0, float wy1,
                                             bool aa) {
    return may_hit_planes(s[0 * NB + j], s[1 * NB + j], s[2 * NB + j], wx0, wx1, wy0, wy1, aa);
}

struct Hit {
    float dx, dy, ipz, u, v, rho3, rho2, z, G, a_raw, alpha;
    f3 p;
    bool use3;
};

// reciprocal for values that feed no threshold decision (gradients and the distortion term only)
__device__ __forceinline__ float grad_rcp(float x) {
#if GSTEX_FAST_RCP
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// expf for x <= 0: the device library's expf sequence (two-part x*log2(e), rint, v_exp_f32, ldexp) without its
// overflow/underflow selects, so the same bits wherever expf is finite and non-zero.  The argument is
// clamped at -104 (expf's own flush-to-zero point; a NaN argument also lands there), so a degenerate
// pair gets G ~ 0 and fails the alpha test instead of propagating NaN.
__device__ __forceinline__ float exp_nonpos(float x) {
    x = fmaxf(x, -104.0f);
    const float ph = x * 1.44269502e+00f;                        // 0x3fb8aa3b
    float pl = __builtin_fmaf(x, 1.44269502e+00f, -ph);
    pl = __builtin_fmaf(x, 1.92596286e-08f, pl);                  // 0x32a5705f
    const float e = __builtin_rintf(ph);
    const float a = (ph - e) + pl;
    return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return __builtin_amdgcn_readfirstlane(v);
}
// The pair's offset from the anchor and homogeneous point p = k x l in affine form (gstex_common.h affine_homog):
// explicit fused multiply-adds (oracle/raster.py restates them: exact product, one rounding)
__device__ __forceinline__ void hit_p(const Rec& r, float px, float py, Hit& h) {
    h.dx = px - r.xa;
    h.dy = py - r.ya;
    h.p = f3{__builtin_fmaf(h.dx, r.A.x, h.dy * r.B.x), __builtin_fmaf(h.dx, r.A.y, h.dy * r.B.y),
             __builtin_fmaf(h.dy, r.B.z, __builtin_fmaf(h.dx, r.A.z, r.Pz))};
}
// The same for a near-edge-on splat (gstex_common.h kHpCos) from its fp64 setup row (A, B, Pz, anchor), each value
// rounded once: p is a small difference of larger terms there, and every value derived from it (u, v, the depth, the
// weights and all gradients through them) inherits the fp32 record's rounding amplified.  Used by every kernel that
// evaluates pairs of records carrying the mark (forward and backward alike, so both take the same decisions).
// The row is read with vector buffer loads (its 18 dwords would not fit beside the record in the kernels' SGPRs).
__device__ __forceinline__ double hp_load(__amdgpu_buffer_rsrc_t rs, int k) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, k * 8, 0, 0));
}
__device__ __forceinline__ void hit_p_hp(const double* __restrict__ row, float px, float py, Hit& h) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(row), 0, H_TW * 8,
                                                                        0x00020000);
    const double dx = (double)px - hp_load(rs, H_XA), dy = (double)py - hp_load(rs, H_YA);
    h.dx = (float)dx;
    h.dy = (float)dy;
    // one component at a time (the empty asm statements keep the row loads from being hoisted together): the
    // fp64 temporaries stay few, so the forward's visit loop keeps its register budget without spills
    h.p.x = (float)__builtin_fma(dx, hp_load(rs, H_A), dy * hp_load(rs, H_B));
    asm volatile("" : "+v"(h.p.x));
    h.p.y = (float)__builtin_fma(dx, hp_load(rs, H_A + 1), dy * hp_load(rs, H_B + 1));
    asm volatile("" : "+v"(h.p.y));
    h.p.z = (float)__builtin_fma(dy, hp_load(rs, H_B + 2), __builtin_fma(dx, hp_load(rs, H_A + 2), hp_load(rs, H_PZ)));
}
// The forward's copy: the row address is wave-uniform there, so plain loads become scalar loads and the row's
// doubles sit in SGPRs (fused multiply-adds take them as the scalar operand) -- the forward's visit loop is at its
// VGPR budget, and fp64 row values in VGPRs made the allocator spill the cull's loop-carried bounds
__device__ __forceinline__ void hit_p_hp_uniform(const double* __restrict__ row, float px, float py, Hit& h) {
    const double dx = (double)px - row[H_XA], dy = (double)py - row[H_YA];
    h.dx = (float)dx;
    h.dy = (float)dy;
    h.p = f3{(float)__builtin_fma(dx, row[H_A], dy * row[H_B]), (float)__builtin_fma(dx, row[H_A + 1], dy * row[H_B + 1]),
             (float)__builtin_fma(dy, row[H_B + 2], __builtin_fma(dx, row[H_A + 2], row[H_PZ]))};
}

// Returns false when the pair is skipped (degenerate, behind the near plane or alpha < 1/255).  h.dx, h.dy, h.p from
// hit_p / hit_p_hp.
__device__ __forceinline__ bool eval_rest(const Rec& r, float px, float py, bool aa, Hit& h) {
    // branch-free: a skipped pair's values are computed anyway (possibly inf/NaN) and never used, so
    // the callers see one predicate instead of three divergent exits (fewer exec-mask joins)
    const bool ok = h.p.z != 0.0f;
#if GSTEX_FAST_EVAL
    h.ipz = __builtin_amdgcn_rcpf(h.p.z);
#else
    h.ipz = 1.0f / h.p.z;
#endif
    h.u = h.p.x * h.ipz;
    h.v = h.p.y * h.ipz;
    h.rho3 = __builtin_fmaf(h.u, h.u, h.v * h.v);
    float dx = r.x - px, dy = r.y - py;
    h.rho2 = kFilterInvSq * __builtin_fmaf(dx, dx, dy * dy);
    h.use3 = !aa || (h.rho3 <= h.rho2);
    float rho = h.use3 ? h.rho3 : h.rho2;
    h.z = h.use3 ? __builtin_fmaf(h.u, r.Tw.x, __builtin_fmaf(h.v, r.Tw.y, r.Tw.z)) : r.Tw.z;
#if GSTEX_FAST_EVAL
    h.G = __builtin_amdgcn_exp2f(-0.72134752f * rho);  // exp(-rho/2) = 2^(-rho/(2 ln 2))
#else
    h.G = exp_nonpos(-0.5f * rho);
#endif
    h.a_raw = r.opac * h.G;
    h.alpha = fminf(kAlphaMax, h.a_raw);
    return ok && h.z >= kNear && h.alpha >= kAlphaMin;  // oracle/raster.py: nz & (zz >= near) & (alpha >= amin)
}
__device__ __forceinline__ bool eval_hit(const Rec& r, float px, float py, bool aa, Hit& h) {
    hit_p(r, px, py, h);
    return eval_rest(r, px, py, aa, h);
}

// One texel's channels: with C == 3 a single 12-B global_load_dwordx3 (the three channels share a cache
// line; three dword loads would look the same lines up three times in the vL1D).
struct __attribute__((aligned(4))) Texel3 { float v[3]; };
template <int CM>
__device__ __forceinline__ void load_texel(const float* __restrict__ p, int Cn, float (&out)[CM]) {
    if constexpr (CM == 3) {
        const Texel3 t = *reinterpret_cast<const Texel3*>(p);
        out[0] = t.v[0];
        out[1] = t.v[1];
        out[2] = t.v[2];
    } else {
#pragma unroll
        for (int c = 0; c < CM; ++c) out[c] = (c < Cn) ? p[c] : 0.0f;
    }
}

// A splat's texel block as a buffer resource: the wave-uniform block base and size live in SGPRs and
// each lane supplies a 32-bit byte offset, so a gather costs one buffer_load and no 64-bit address
// arithmetic; the hardware range check (size = the block's h*w*C floats) returns 0 outside the block.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t texel_rsrc(const float* texture, int off, int n_texels, int Cn) {
    off = __builtin_amdgcn_readfirstlane(off);
    n_texels = __builtin_amdgcn_readfirstlane(n_texels);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(texture) + (size_t)off * Cn, 0, n_texels * Cn * 4,
                                             0x00020000);
}
template <int CM>
__device__ __forceinline__ void load_texel_rs(__amdgpu_buffer_rsrc_t rs, int idx, int Cn, float (&out)[CM]) {
    if constexpr (CM == 3) {
        const auto t = __builtin_amdgcn_raw_buffer_load_b96(rs, idx * 12, 0, 0);
        out[0] = __int_as_float(t[0]);
        out[1] = __int_as_float(t[1]);
        out[2] = __int_as_float(t[2]);
    } else {
#pragma unroll
        for (int c = 0; c < CM; ++c)
            out[c] = (c < Cn) ? __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (idx * Cn + c) * 4, 0, 0)) : 0.0f;
    }
}

// The 4 bilinear texels of a splat block: byte offsets from one 24-bit multiply-add (v_mul_u32_u24 is
// full rate; the block index i*w + j < 2^24) plus wave-uniform row/column steps.
// Forward variant (C = 3): the far corners at i0 + 1 / j0 + 1 without the clamp to the block's edge.  When the
// coordinate is clamped to the last row / column its weight is exactly 0 (ax = 0 / ay = 0) and the lerp returns
// the near value bit for bit, so the far texel only has to be finite: one row down past the block reads 0 (buffer
// range check), one column right reads the next row's first texel.
__device__ __forceinline__ void load_texel_quad_unclamped(__amdgpu_buffer_rsrc_t rs, const Bilerp& b, int w,
                                                          float (&t00)[3], float (&t01)[3], float (&t10)[3],
                                                          float (&t11)[3]) {
    const int rowb = w * 12;  // row stride in bytes (wave-uniform: scalar when w is)
    const int o00 = (int)(__umul24(b.i0, (unsigned)rowb) + __umul24(b.j0, 12u));
    const int o10 = o00 + rowb;
    const auto a = __builtin_amdgcn_raw_buffer_load_b96(rs, o00, 0, 0);
    const auto c = __builtin_amdgcn_raw_buffer_load_b96(rs, o00 + 12, 0, 0);
    const auto d = __builtin_amdgcn_raw_buffer_load_b96(rs, o10, 0, 0);
    const auto e = __builtin_amdgcn_raw_buffer_load_b96(rs, o10 + 12, 0, 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t00[k] = __int_as_float(a[k]);
        t01[k] = __int_as_float(c[k]);
        t10[k] = __int_as_float(d[k]);
        t11[k] = __int_as_float(e[k]);
    }
}
template <int CM>
__device__ __forceinline__ void load_texel_quad(__amdgpu_buffer_rsrc_t rs, const Bilerp& b, int w, int Cn,
                                                float (&t00)[CM], float (&t01)[CM], float (&t10)[CM],
                                                float (&t11)[CM]) {
    if constexpr (CM == 3) {
        const int o00 = (int)__umul24(__umul24(b.i0, w) + b.j0, 12u);
        const int o01 = b.j1 > b.j0 ? o00 + 12 : o00;
        const int o10 = b.i1 > b.i0 ? o00 + w * 12 : o00;
        const int o11 = b.j1 > b.j0 ? o10 + 12 : o10;
        const auto a = __builtin_amdgcn_raw_buffer_load_b96(rs, o00, 0, 0);
        const auto c = __builtin_amdgcn_raw_buffer_load_b96(rs, o01, 0, 0);
        const auto d = __builtin_amdgcn_raw_buffer_load_b96(rs, o10, 0, 0);
        const auto e = __builtin_amdgcn_raw_buffer_load_b96(rs, o11, 0, 0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t00[k] = __int_as_float(a[k]);
            t01[k] = __int_as_float(c[k]);
            t10[k] = __int_as_float(d[k]);
            t11[k] = __int_as_float(e[k]);
        }
    } else if constexpr (CM == 6) {
        // the eval render's 6 channels: two 12-B loads per corner (24 B contiguous per texel) instead of six dwords
        const int o00 = (int)__umul24(__umul24(b.i0, w) + b.j0, 24u);
        const int o01 = b.j1 > b.j0 ? o00 + 24 : o00;
        const int o10 = b.i1 > b.i0 ? o00 + w * 24 : o00;
        const int o11 = b.j1 > b.j0 ? o10 + 24 : o10;
        const int off[4] = {o00, o01, o10, o11};
        float (*dst[4])[CM] = {&t00, &t01, &t10, &t11};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const auto lo = __builtin_amdgcn_raw_buffer_load_b96(rs, off[q], 0, 0);
            const auto hi = __builtin_amdgcn_raw_buffer_load_b96(rs, off[q] + 12, 0, 0);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                (*dst[q])[k] = __int_as_float(lo[k]);
                (*dst[q])[3 + k] = __int_as_float(hi[k]);
            }
        }
    } else {
        load_texel_rs<CM>(rs, b.i0 * w + b.j0, Cn, t00);
        load_texel_rs<CM>(rs, b.i0 * w + b.j1, Cn, t01);
        load_texel_rs<CM>(rs, b.i1 * w + b.j0, Cn, t10);
        load_texel_rs<CM>(rs, b.i1 * w + b.j1, Cn, t11);
    }
}

// the sample point in texel units (xr, yr) = (tu h, tv w) from the record's prescaled texture affine (setup_kernel)
__device__ __forceinline__ void tex_coords(const Rec& r, float u, float v, float& xr, float& yr) {
    xr = __builtin_fmaf(u, r.auu, __builtin_fmaf(v, r.auv, r.tu0));  // fused (oracle/raster.py restates it)
    yr = __builtin_fmaf(u, r.avu, __builtin_fmaf(v, r.avv, r.tv0));
}

// ------------------------------------------------------------------------------------------
// entry checks (host): the rules the tile-walking entry points (gstex_raster_fwd, gstex_raster_bwd, gstex_texture_edit,
// gstex_paint_scatter) share, each stated once.  Each entry point calls them in the order it has always checked in,
// since the first rule broken decides the status and the message; `who` opens the message.
// ------------------------------------------------------------------------------------------
#define GSTEX_CHECK(call)                       \
    do {                                        \
        if (const int rc_ = (call)) return rc_; \
    } while (0)

struct SettingsRule { int accepted; const char* list; };  // the accepted bits, and as the message names them
constexpr SettingsRule kRenderSettings{GSTEX_SETTING_AA_BLUR | GSTEX_SETTING_DIST_REG | GSTEX_SETTING_EVAL_NORMAL,
                                       "1<<9, 1<<10, 1<<15"};
constexpr SettingsRule kEditSettings{kRenderSettings.accepted | GSTEX_SETTING_EDIT,  // the viewer's edit flag rides along
                                     "1<<9, 1<<10, 1<<13, 1<<15"};

inline int check_settings(const char* who, int settings, const SettingsRule& rule) {
    if (!(settings & ~rule.accepted)) return GSTEX_OK;
    set_error("%s: unsupported settings bits 0x%x (supported: %s)", who, settings & ~rule.accepted, rule.list);
    return GSTEX_ERR_UNSUPPORTED;
}

inline int check_camera(const char* who, const gstex_camera* cam) {
    GSTEX_REQUIRE(cam && cam->H > 0 && cam->W > 0, "%s: invalid camera", who);
    GSTEX_REQUIRE(cam->block == kTile, "%s: block_width must be %d (got %d)", who, kTile, cam->block);
    return GSTEX_OK;
}

inline int check_channels(const char* who, int channels) {
    GSTEX_REQUIRE(channels >= 1 && channels <= 8, "%s: channels must be in [1, 8] (got %d)", who, channels);
    return GSTEX_OK;
}

// the kernels index a texel's floats with an int (channels = 1: the texels themselves)
inline int check_n_texels(const char* who, int64_t n_texels, int channels) {
    GSTEX_REQUIRE(n_texels >= 0 && n_texels * channels < (int64_t)INT32_MAX, "%s: n_texels out of range (%lld)", who,
                  (long long)n_texels);
    return GSTEX_OK;
}

inline int check_n_isect(const char* who, int64_t n_isect) {
    GSTEX_REQUIRE(n_isect >= 0 && n_isect < (int64_t)INT32_MAX, "%s: n_isect out of range", who);
    return GSTEX_OK;
}

}  // namespace gstex
