// raster_bwd.hip — the raster backward (gstex_raster_bwd, gstex_raster_bwd_variant): the gradient of the forward's
// composite (raster_fwd.hip) with respect to each splat's record, accumulated per splat, and to the texels.  The
// record's chain to the splat parameters is raster_setup_bwd.hip's.
//
// Replaces the backward of gstex_cuda.texture.texture_gaussians (through autograd at engine/trainer.py:460).
//
// MI355X layout: one wave64 workgroup per unit = (tile, 8x8 quadrant, segment), launched costliest first, no barriers
// and no shared state between waves; a unit starts from the forward's checkpoint after its segment and walks back to
// front; per visit the 24 splat partials are reduced across the wave with a reduce-scatter butterfly (permlane32/16
// swaps + DPP) and added into the splat's accumulator row with one coalesced float-atomic instruction (deterministic
// mode: stored as the (pair, quadrant) row at the pair's emission slot and summed in fixed order by setup_bwd); texel
// gradients go through a DPP segmented scan, int32 fixed-point LDS staging of the splat's block and a flush of its
// non-zero entries with global fp32 atomics.
#include "raster_common.h"
#include "gstex_internal.h"
#define GSTEX_DIAG_BWD
#include "raster_diag.h"  // diagnostic builds only (GSTEX_STATS counters, GSTEX_PAIR_DUMP); empty by default

using namespace gstex;

namespace {

#ifndef GSTEX_SEG_W
// texel-gradient segment width in lanes: half a pixel row of the 8x8 quadrant (2 scan steps, twice the run tails of
// a whole row: measured 4% faster backward than 8, 2 is slower again)
#define GSTEX_SEG_W 4
#endif
// Backward occupancy: waves per SIMD the register allocation targets, per instantiation.  The generic photometric
// build (C = 3, no geometry gradients) fits 7 (72 VGPRs; 1 VGPR + 5 SGPR spills, none in the visit loop; at 8 it
// takes 7 + 23 and measured 3 % slower); the others 5.  The training call (TRAIN: one upstream gradient for img and
// tex, no deterministic rows) drops a register set, the slot load and the row branch, which leaves 1 VGPR + 12 SGPR
// spills at 8 waves (64 VGPRs, 78 SGPRs): the word loop reloads them, the visit loop only in the unstaged-block
// branch (4 v_readlane, blocks above kTexStage / 3 texels); measured 1347 us against the generic build's 1380 ..
// 1387 (TRAIN at 7 waves: spill-free, 1368 .. 1372; profiles/bwd_train_summary.md).
// Measured: warming the next visit's record line with a scalar load during the current visit gains nothing
// (records hit in cache).
#ifndef GSTEX_BWD_WAVES_TRAIN
#define GSTEX_BWD_WAVES_TRAIN 7
#endif
#ifndef GSTEX_BWD_WAVES
#define GSTEX_BWD_WAVES 5
#endif
#ifndef GSTEX_BWD_WAVES_TRAINCALL
#define GSTEX_BWD_WAVES_TRAINCALL 8
#endif
template <int C, bool GEO, bool TRAIN = false>
struct BwdShape {
    static constexpr bool kTrain = (C == 3 && !GEO);
    static constexpr int kWaves = TRAIN ? GSTEX_BWD_WAVES_TRAINCALL : kTrain ? GSTEX_BWD_WAVES_TRAIN : GSTEX_BWD_WAVES;
};
// Backward per-wave texel staging: one splat's texel block (h * w * C int32 fixed-point entries) at a time, 4 KiB
// per wave (341 texels at C = 3; cfg3's largest block is 169); a larger block adds its run tails straight to global
// memory.  Measured: 6 KiB staging 3 % slower than 4, 3 and 2 KiB (equal); int64 staging +0.15 ms.)
#ifndef GSTEX_TEX_STAGE
#define GSTEX_TEX_STAGE 1024
#endif
constexpr int kTexStage = GSTEX_TEX_STAGE;
#ifndef GSTEX_WORD_WAIT
#define GSTEX_WORD_WAIT 1  // backward: the visit loop's id wait hoisted to the word start (see raster_bwd_kernel)
#endif

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// Reduce-scatter butterfly over the 64 lanes, entirely on VALU cross-lane ops (no LDS traffic):
// xor-32 and xor-16 halvings with v_permlane32_swap / v_permlane16_swap, xor-8 with DPP row_ror:8,
// then an 8-lane all-reduce (quad_perm xor1, xor2, row_half_mirror).  On return, lane l with
// (l & 7) == 0 holds the wave sums of values [NV/2 b5 + NV/4 b4 + NV/8 b3 + 0 .. NV/8 - 1] (b5,b4,b3 = bits of l).
template <int NV>
__device__ __forceinline__ void wave_reduce(float (&v)[NV]) {
    static_assert(NV == 24 || NV == 32, "reduce-scatter over 8 lane groups of 3 or 4 values");
    constexpr int H = NV / 2, Q = NV / 4, E = NV / 8;
    const int lane = threadIdx.x & 63;
    // permlane32_swap(a, b) leaves a = [a_lo, b_lo], b = [a_hi, b_hi]: a + b holds a's half-sum in
    // lanes 0-31 and b's in lanes 32-63 (likewise per row pair for permlane16_swap)
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + H]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + Q]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        // the last four stages as single v_add_f32_dpp instructions (the compiler emits a DPP move plus an add):
        // row_ror:8 (lane ^ 8 inside a 16-lane row), quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror (the other
        // quad of the 8-lane group).  dpp(x) + y rounds as y + dpp(x).  The leading s_nop covers the VALU-write ->
        // DPP-read hazard for the inputs (the asm is opaque to the hazard recognizer); inside, each value is DPP-read
        // again only after the other E - 1 >= 2 values' writes; the trailing s_nop covers a following DPP read.
        const bool hi = lane & 8;
        float keep[4], send[4];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            send[i] = hi ? v[i] : v[i + E];
            keep[i] = hi ? v[i + E] : v[i];
        }
#define GSTEX_DPP_ADD(CTRL, D, S) "v_add_f32_dpp %" #D ", %" #S ", %" #D " " CTRL " row_mask:0xf bank_mask:0xf\n"
#define GSTEX_DPP_SELF(CTRL, D) "v_add_f32_dpp %" #D ", %" #D ", %" #D " " CTRL " row_mask:0xf bank_mask:0xf\n"
        if constexpr (E == 3) {
            asm volatile("s_nop 1\n"
                         GSTEX_DPP_ADD("row_ror:8", 0, 3) GSTEX_DPP_ADD("row_ror:8", 1, 4) GSTEX_DPP_ADD("row_ror:8", 2, 5)
                         GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 0) GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 1)
                         GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 2)
                         GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 0) GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 1)
                         GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 2)
                         GSTEX_DPP_SELF("row_half_mirror", 0) GSTEX_DPP_SELF("row_half_mirror", 1)
                         GSTEX_DPP_SELF("row_half_mirror", 2)
                         "s_nop 1"
                         : "+v"(keep[0]), "+v"(keep[1]), "+v"(keep[2])
                         : "v"(send[0]), "v"(send[1]), "v"(send[2]));
        } else {
            asm volatile("s_nop 1\n"
                         GSTEX_DPP_ADD("row_ror:8", 0, 4) GSTEX_DPP_ADD("row_ror:8", 1, 5) GSTEX_DPP_ADD("row_ror:8", 2, 6)
                         GSTEX_DPP_ADD("row_ror:8", 3, 7)
                         GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 0) GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 1)
                         GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 2) GSTEX_DPP_SELF("quad_perm:[1,0,3,2]", 3)
                         GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 0) GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 1)
                         GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 2) GSTEX_DPP_SELF("quad_perm:[2,3,0,1]", 3)
                         GSTEX_DPP_SELF("row_half_mirror", 0) GSTEX_DPP_SELF("row_half_mirror", 1)
                         GSTEX_DPP_SELF("row_half_mirror", 2) GSTEX_DPP_SELF("row_half_mirror", 3)
                         "s_nop 1"
                         : "+v"(keep[0]), "+v"(keep[1]), "+v"(keep[2]), "+v"(keep[3])
                         : "v"(send[0]), "v"(send[1]), "v"(send[2]), "v"(send[3]));
        }
#undef GSTEX_DPP_ADD
#undef GSTEX_DPP_SELF
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = keep[i];
    }
}

// ------------------------------------------------------------------------------------------
// texel-gradient pre-reduction: along each 16-lane row (16 consecutive pixels of one image row)
// the bilinear cell of a splat's texture forms contiguous runs, so a segmented inclusive scan
// by cell key with DPP row shifts leaves each run's sum in its last lane; only run tails issue
// the 4*C atomics (instead of every contributing lane, which serialised on the LDS atomic unit).
// ------------------------------------------------------------------------------------------
// row_shr:OFF with out-of-row lanes reading 0 (bound_ctrl)
template <int CTRL>
__device__ __forceinline__ int dpp_bc_i(int v) {
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
}
template <int OFF>
__device__ __forceinline__ float dpp_shr_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + OFF, 0xF, 0xF, false));
}

// v += row_shr:OFF(v) * mf, mf = 1 where the lane OFF to the left is in the same segment, else 0: one
// v_fmac_f32 with a DPP source per value (the compiler does not fold a DPP move into the tied-accumulator
// fmac, so it is written out).  fma(t, 1, v) rounds as t + v and fma(t, 0, v) = v, so the result equals the
// add-and-select form bit for bit.  The leading s_nop covers the VALU-write -> DPP-read hazard for the
// values' last writers (the asm is opaque to the compiler's hazard recognizer); within the block each value is
// read by DPP only after the other NV - 1 writes, and the trailing s_nop covers the compiler's next DPP read.
template <int OFF>
__device__ __forceinline__ void fmac_dpp_shr(float& v, float mf) {
    if constexpr (OFF == 1)
        asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(v) : "v"(mf));
    else if constexpr (OFF == 2)
        asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(v) : "v"(mf));
    else if constexpr (OFF == 4)
        asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(v) : "v"(mf));
    else
        asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(v) : "v"(mf));
}
// Segments = maximal runs of equal key inside a 16-lane row (a lane whose key differs from its left
// neighbour starts a segment, so a non-contributing lane splits a run instead of being bridged).
// Returns true for the last lane of a segment with key >= 0; it then holds the segment's sums.
// 1.0f in the lanes whose bit of the wave mask m is set, else 0 (one v_cndmask with the mask as lane select)
__device__ __forceinline__ float mask_one(unsigned long long m) {
    float r;
    asm("v_cndmask_b32_e64 %0, 0, 1.0, %1" : "=v"(r) : "s"(m));
    return r;
}
// The segment heads as one wave mask H (ballot of key changes, plus every group's first
// lane); lane l joins lane l - OFF iff no head lies in (l - OFF, l], i.e. bit l of ~(H | H << 1 | ... | H << (OFF-1)),
// computed on the scalar unit; the run tails are the lanes before a head or at a group's end.
template <int NV>
__device__ __forceinline__ bool seg_reduce_rows(int key, float (&v)[NV]) {
    constexpr int SW = GSTEX_SEG_W;
    static_assert(SW == 2 || SW == 4 || SW == 8 || SW == 16, "segment width");
    constexpr unsigned long long kFirst = SW == 2 ? 0x5555555555555555ull : SW == 4 ? 0x1111111111111111ull
                                        : SW == 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
    constexpr unsigned long long kLast = kFirst << (SW - 1);
    const int left = dpp_bc_i<0x111>(key);  // row_shr:1 (lanes at a group start are heads regardless)
    const unsigned long long H = __ballot(left != key) | kFirst;
    const unsigned long long live = __ballot(key >= 0);
    unsigned long long cover = H;  // heads in (l - off, l] for the current off
#pragma unroll
    for (int off = 1; off < SW; off <<= 1) {
        const float mf = mask_one(~cover);
        asm volatile("s_nop 1" ::: "memory");
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (off == 1) fmac_dpp_shr<1>(v[i], mf);
            else if (off == 2) fmac_dpp_shr<2>(v[i], mf);
            else if (off == 4) fmac_dpp_shr<4>(v[i], mf);
            else fmac_dpp_shr<8>(v[i], mf);
        }
        asm volatile("s_nop 1" ::: "memory");
        cover = cover | (cover << off);
    }
    const unsigned long long tails = ((H >> 1) | kLast) & live;
    return mask_one(tails) != 0.0f;
}

// Backward: one wave64 workgroup per (tile, 8x8 quadrant) -- the 4 quadrant waves of a tile share nothing, so
// no wave ever waits for another (no barriers; a finished wave frees its slot at once).  The wave walks the
// tile list back to front over the forward's cull bits for its quadrant, up to its last contributor.  Per
// visited splat it reduces its 24 gradient partials across its 64 pixels and adds them into the splat's accumulator
// row with one float-atomic instruction; in the deterministic mode (row_flags given) it stores them instead as the
// (pair, quadrant) row partials[slot][quadrant] (slot = the pair's emission slot), flagging the row in
// row_flags[slot] (byte = quadrant; rows never written stay unflagged and are never read), and
// gstex_raster_setup_bwd sums each splat's flagged rows in (slot, quadrant) order -> bitwise reproducible.
// Texel gradients: segmented scan along each 4-pixel half row, run tails
// added to the splat's texel block staged in the wave's LDS as int32 fixed point (exact, order-independent),
// and the block flushed to v_texture (global float atomics, non-zero entries only) right after the visit.
//
// GEO = false: no depth / distortion / normal upstream gradient (all NULL, the training default:
// gstex.py:198-201 sets both weights to 0), so every term they scale is dropped at compile time.  The
// remaining arithmetic is unchanged (x + 0 * y = x), so both variants give the same values.
//
// TRAIN = true (C = 3, GEO = false; gstex_raster_bwd_variant): the photometric training step's call, whose facts
// are known before the launch -- v_tex is v_img (the loss's one gradient image for both outputs), v_img and v_alpha
// are given, and the accumulation is the float-atomic one.  dL/dtex is then dL/dimg's registers, and the emission
// slot and the row stores are gone; every sum is formed in the generic build's order.

// Texel-gradient fixed point, per visit: the reduce also sums M = sum over the wave's pixels of |w tex_scale| x
// max_c |dL/dtex[c]|, a bound on what the visit adds to any staged entry (bilinear weights <= 1).  Contributions
// are formed at scale 2^S, S = 30 - e (M < 2^e); each run tail of the 8-lane row scan (< 2^30) is rounded to
// int32 (one v_cvt_rpi_i32_f32) and the tails are summed exactly in int32 (|sum| <= 2^30 + rounding).
// Resolution: 2^-30 of the visit's total.
__device__ __forceinline__ int fixed_round(float y) {  // y already scaled by 2^S; round half up, one VALU op
    int q;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(q) : "v"(y));
    return q;
}
constexpr int kTexFixBits = 30;

// (fp32 staging with ds_add_f32 instead measured 2x slower: 3.2 vs 1.57 ms, round 2; 3.0 vs 1.4 ms, round 4)
__device__ __forceinline__ void stage_add(int* a, float y) { atomicAdd(a, fixed_round(y)); }
#ifndef GSTEX_FLUSH_U
#define GSTEX_FLUSH_U 4
#endif
constexpr int kFlushU = GSTEX_FLUSH_U;  // staging entries per lane per flush pass
static_assert(kTexStage % (64 * kFlushU) == 0, "flush passes tile the staging area");


template <int C, bool GEO, bool TRAIN = false>
__global__ __launch_bounds__(64, (BwdShape<C, GEO, TRAIN>::kWaves)) void raster_bwd_kernel(
    CamArgs cam_args, int tiles_x, int settings, const float* __restrict__ bg, int Cdyn,
    const float4* __restrict__ records, const double* __restrict__ hp_records, const int2* __restrict__ tile_ranges,
    const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ sorted_slots, const float* __restrict__ texture,
    int n_texels, float tex_scale, float tex_bias, const float4* __restrict__ state, const float* __restrict__ v_img,
    const float* __restrict__ v_depth, const float* __restrict__ v_reg, const float* __restrict__ v_alpha,
    const float* __restrict__ v_tex, const float* __restrict__ v_normal, float* __restrict__ partials,
    unsigned char* __restrict__ row_flags, float* __restrict__ v_texture, const AuxPtrs aux, const ZeroBufs zb) {
    static_assert(!TRAIN || (C == 3 && !GEO), "the training call is photometric, 3 channels");
    zero_bufs(zb);
    const Camera cam = load_camera(cam_args);
    constexpr int CM = (C > 0) ? C : 8;
    const int Cn = (C > 0) ? C : Cdyn;
    __shared__ int s_texq[kTexStage];

    // unit = 4 slot + quadrant (see AuxPtrs), launched costliest first; a unit the forward never evaluated in is empty
    const int unit = aux.order[blockIdx.x] - 1;  // entries are unit + 1
    if (unit < 0) return;  // a launch position no unit was placed at (empty units take none)
    const int quad = unit & 3, slot = unit >> 2;
    const int tile = aux.slot_tile[slot];
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int lane = threadIdx.x;
    const WaveBlock wb = wave_block(tx, ty, quad * 64 + lane);
    const int pxi = wb.px, pyi = wb.py;
    const bool inside = pxi < cam.W && pyi < cam.H;
    const float px = (float)pxi + 0.5f, py = (float)pyi + 0.5f;  // pixel centres (gstex_common.h)
    const bool aa = (settings & GSTEX_SETTING_AA_BLUR) != 0;
    const bool dreg = (settings & GSTEX_SETTING_DIST_REG) != 0;
    const int2 rng = tile_ranges[tile];
    const float bg0 = bg ? bg[0] : 0.f, bg1 = bg ? bg[1] : 0.f, bg2 = bg ? bg[2] : 0.f;

    float T = 1.0f, M1f = 0.f, M2f = 0.f;
    int last = -1;
    float Gimg[3] = {0.f, 0.f, 0.f}, Gn[3] = {0.f, 0.f, 0.f}, Gtex[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) Gtex[c] = 0.f;
    float Gd = 0.f, Greg = 0.f, Ga = 0.f;
    if (inside) {
        const size_t pix = (size_t)pyi * cam.W + pxi;
        const float4 st = state[pix];
        T = st.x; M1f = st.y; M2f = st.z; last = __float_as_int(st.w);
        // a NULL upstream gradient (an output the loss does not use) counts as zero
        if (TRAIN || v_img) { Gimg[0] = v_img[3 * pix]; Gimg[1] = v_img[3 * pix + 1]; Gimg[2] = v_img[3 * pix + 2]; }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            if constexpr (TRAIN) Gtex[c] = Gimg[c];  // v_tex is v_img: one set of registers
            else if (c < Cn && v_tex) Gtex[c] = v_tex[(size_t)Cn * pix + c];
        }
        Ga = (TRAIN || v_alpha) ? v_alpha[pix] : 0.f;
        if (GEO) {
            Gd = v_depth ? v_depth[pix] : 0.f;
            Greg = (dreg && v_reg) ? v_reg[pix] : 0.f;
            if (v_normal) { Gn[0] = v_normal[3 * pix]; Gn[1] = v_normal[3 * pix + 1]; Gn[2] = v_normal[3 * pix + 2]; }
        }
    }
    // the wave's last contributor: pairs behind it receive no gradient from this quadrant (no row, no flag); this
    // unit walks tile-list positions [lo, hi] of its segment
    const int wave_last = wave_max_i(last);
    GSTEX_WG_STAMP(rng.y - rng.x, wave_last);
    const int sbase = seg_base(rng.x, tile);
    const int seg = slot - sbase, lo = seg * kSegLen;
    if (wave_last < lo) return;
    const int hi = min(lo + kSegLen - 1, wave_last), kf = wave_last / kSegLen;
    GSTEX_STAT(0, 1);
    const float Af = 1.0f - T;
    float R = (Gimg[0] * bg0 + Gimg[1] * bg1) + Gimg[2] * bg2;
    float Gtex_bias = 0.f;  // tex_bias * sum_c dL/dtex[c]: the bias part of sum_c dL/dtex[c] * texel value
#pragma unroll
    for (int c = 0; c < CM; ++c) Gtex_bias += Gtex[c];
    Gtex_bias *= tex_bias;
    if (seg < kf) {
        // start from the forward's checkpoint after this segment: T_k, and R T_k = sum over the splats behind the
        // segment of w_j g_j + T_final (bg term) = (final - checkpoint accumulators) . upstream gradients
        const float* ck = aux.ckpt + ((size_t)slot * 4 + quad) * aux.F * 64 + lane;
        const float* fin = aux.ckpt + ((size_t)(sbase + kf) * 4 + quad) * aux.F * 64 + lane;
        const float Tk = ck[0];
        float back = (Gimg[0] * (fin[64] - ck[64]) + Gimg[1] * (fin[128] - ck[128])) + Gimg[2] * (fin[192] - ck[192]);
#pragma unroll
        for (int c = 0; c < CM; ++c)
            if (c < Cn) back += Gtex[c] * (fin[(4 + c) * 64] - ck[(4 + c) * 64]);
        back += Ga * (Tk - T);  // the weights behind sum to T_k - T_final
        if (GEO) {
            const float* fg = fin + (4 + Cn) * 64;
            const float* cg = ck + (4 + Cn) * 64;
            back += Gd * (fg[0] - cg[0]);
            back += (Gn[0] * (fg[64] - cg[64]) + Gn[1] * (fg[128] - cg[128])) + Gn[2] * (fg[192] - cg[192]);
            if (dreg) back += Greg * ((Af * (fg[320] - cg[320]) - 2.0f * M1f * (fg[256] - cg[256])) + M2f * (Tk - T));
        }
        if (inside) {
            R = (back + T * R) / Tk;
            T = Tk;
        }
    }
    float gabs = 0.f;  // max_c |dL/dtex[c]|: bounds this pixel's texel-gradient contributions (x w |tex_scale|)
#pragma unroll
    for (int c = 0; c < CM; ++c) gabs = fmaxf(gabs, fabsf(Gtex[c]));
    for (int i = lane; i < kTexStage; i += 64) s_texq[i] = 0;
    const size_t vm_base = visit_mask_base(rng.x, tile);

    for (int wd = hi >> 6; wd >= (lo >> 6); --wd) {
        const int pos0 = wd << 6;
        // the word's splats this wave visits: the forward's cull bits for this quadrant, clipped to the segment's
        // end (the wave's last contributor in the last segment)
        unsigned long long todo = aux.masks[(vm_base + wd) * 4 + quad];
        const int lim = hi - pos0 + 1;
        if (lim < 64) todo &= (1ull << lim) - 1ull;
        if (!todo) continue;
        // lane k <-> position pos0 + k: splat id and emission slot, loaded once per word (coalesced)
        int my_gid = 0, my_slot = 0;
        if ((todo >> lane) & 1ull) {
            my_gid = sorted_ids[rng.x + pos0 + lane];
            if constexpr (!TRAIN) my_slot = sorted_slots[rng.x + pos0 + lane];  // (the row path's: TRAIN has none)
        }
#if GSTEX_WORD_WAIT
        // wait for the word's ids here, once: otherwise the waitcnt pass, which merges the loop's entry (ids
        // pending) with its back edge (the previous visit's atomics pending), waits at the top of EVERY visit for
        // all but one of the previous visit's atomics before the record can be addressed (vmcnt counts the
        // no-return atomics in order with the loads)
        if constexpr (TRAIN) asm volatile("; word ids %0" ::"v"(my_gid));
        else asm volatile("; word ids %0 %1" ::"v"(my_gid), "v"(my_slot));
#endif
        while (todo) {
            const int j = 63 - __builtin_clzll(todo);
            todo &= ~(1ull << j);
            const int rel = pos0 + j;
            const int gid = __builtin_amdgcn_readlane(my_gid, j);
            const float4* rp = records + (size_t)gid * kRecF4;
            const Rec r = read_rec_global(rp);
            // one predicate for the whole heavy path (a single exec-mask region)
            Hit h;
            hit_p(r, px, py, h);
            // a near-edge-on splat (the record opacity's sign bit): p from its fp64 row, as in the forward
            if (hp_records && __float_as_int(rp[2].w) < 0) hit_p_hp(hp_records + (size_t)gid * H_FIELDS, px, py, h);
            const bool contrib = eval_rest(r, px, py, aa, h) && rel <= last;
            GSTEX_STAT(1, 1);
            GSTEX_STAT(3, __popcll(__ballot(contrib)));
            GSTEX_STAT(13, __popcll(__ballot(rel <= last)));           // lanes not yet past their last contributor
            GSTEX_STAT(14, __popcll(__ballot(contrib)) <= 16 ? 1 : 0);  // sparse visits
            GSTEX_STAT(15, __popcll(__ballot(contrib)) >= 48 ? 1 : 0);  // dense visits
            constexpr int NP = GEO ? kPartRowGeo : kPartRow;
            // a spare slot of the row (zero when stored): the texel fixed-point bound
            constexpr int kMBound = GEO ? 27 : P_NRM;
            float P[NP];
#pragma unroll
            for (int i = 0; i < NP; i += 2) {
                // zero rows in 64-bit moves (one v_mov_b64 per register pair)
                unsigned long long zz;
                asm volatile("v_mov_b64 %0, 0" : "=v"(zz));
                P[i] = __uint_as_float((unsigned)zz);
                P[i + 1] = __uint_as_float((unsigned)(zz >> 32));
            }
            // texel-gradient inputs, expanded into the 4*C bilinear contributions after P is reduced:
            // tkey = top-left texel of the block | (i1 - i0) << 29 | (j1 - j0) << 30, -1 if none
            int tkey = -1;
            float tw = 0.f, tax = 0.f, tay = 0.f;
            const bool blk_ok = r.off + r.h * r.w <= n_texels;  // wave-uniform; false only for corrupt dims
            if (contrib) {
                // gradient arithmetic only from here on (the pair decisions above are the forward's): contracted
#pragma clang fp contract(fast)
                const float one_m = 1.0f - h.alpha;
                T = T * grad_rcp(one_m);
                const float w = h.alpha * T;
                // issue the texel gathers first, then everything that does not need them
                const bool has_tex = r.h * r.w > 0 && blk_ok;
                Bilerp b;
                const __amdgpu_buffer_rsrc_t rs = texel_rsrc(texture, r.off, r.h * r.w, Cn);
                float t00[CM], t01[CM], t10[CM], t11[CM];
#pragma unroll
                for (int c = 0; c < CM; ++c) t00[c] = t01[c] = t10[c] = t11[c] = 0.f;
                if (has_tex) {
                    float xr, yr;
                    tex_coords(r, h.u, h.v, xr, yr);
                    // (converting h, w here measured faster than reading r.hf, r.wf)
                    b = bilerp_xy(xr, yr, r.h, r.w, (float)r.h - 1.0f, (float)r.w - 1.0f);
                    // (far corners unclamped: at a clamped edge their weight is 0 in the value and the edge's
                    // in_u / in_v = false drops the coordinate gradient, so the results are bit-identical)
                    if constexpr (CM == 3) {
                        load_texel_quad_unclamped(rs, b, r.w, t00, t01, t10, t11);
                    } else {
                        load_texel_quad<CM>(rs, b, r.w, Cn, t00, t01, t10, t11);
                    }
                }
                float g = (Gimg[0] * r.rgb[0] + Gimg[1] * r.rgb[1]) + Gimg[2] * r.rgb[2];
                P[P_RGB + 0] = w * Gimg[0];
                P[P_RGB + 1] = w * Gimg[1];
                P[P_RGB + 2] = w * Gimg[2];
                // depth: direct + distortion (m depends on z)
                float dz = 0.f, E = 0.f;
                if (GEO) {
                    P[P_NRM + 0] = w * Gn[0];
                    P[P_NRM + 1] = w * Gn[1];
                    P[P_NRM + 2] = w * Gn[2];
                    const float iz = grad_rcp(h.z);
                    const float m = kFarRatio * (1.0f - kNear * iz);
                    E = dreg ? ((m * m * Af - 2.0f * m * M1f) + M2f) : 0.0f;
                    dz = w * Gd;
                    if (dreg) dz += Greg * (2.0f * w * (m * Af - M1f)) * ((kFarRatio * kNear) * (iz * iz));
                }
                if (has_tex) {
                    tkey = (int)(__umul24(b.i0, r.w) + b.j0) | ((b.i1 - b.i0) << 29) | ((b.j1 - b.j0) << 30);
                    tw = w * tex_scale;  // d value / d stored texel
                    P[kMBound] = fabsf(tw) * gabs;  // summed by the reduce: the visit's fixed-point bound
                    tax = b.ax;
                    tay = b.ay;
                }
                // texture value (tex_scale * stored + tex_bias) and its uv-gradient.  Both are linear in the
                // texels, so the channels are folded first: D_k = sum_c Gtex[c] * t_k[c] per bilinear corner,
                // then one bilinear mix and one pair of differences serve all channels
                float dtu = 0.f, dtv = 0.f, dxr = 0.f, dyr = 0.f;
                if (has_tex) {
                    const float hf = (float)r.h, wf = (float)r.w;
                    float D00 = 0.f, D01 = 0.f, D10 = 0.f, D11 = 0.f;
#pragma unroll
                    for (int c = 0; c < CM; ++c) {
                        if (c < Cn) {
                            D00 = D00 + Gtex[c] * t00[c];
                            D01 = D01 + Gtex[c] * t01[c];
                            D10 = D10 + Gtex[c] * t10[c];
                            D11 = D11 + Gtex[c] * t11[c];
                        }
                    }
                    g += bilerp_mix(D00, D01, D10, D11, b.ax, b.ay) * tex_scale + Gtex_bias;
                    const float su = (1.0f - b.ay) * (D10 - D00) + b.ay * (D11 - D01);
                    const float sv = (1.0f - b.ax) * (D01 - D00) + b.ax * (D11 - D10);
                    // d value / d xr, d yr (texel units); the record's texture affine is prescaled by h, w
                    dxr = b.in_u ? w * su : 0.0f;
                    dyr = b.in_v ? w * sv : 0.0f;
                    dtu = dxr * hf;
                    dtv = dyr * wf;
                }
                if (GEO) {
                    g += Gd * h.z;
                    g += (Gn[0] * r.nrm[0] + Gn[1] * r.nrm[1]) + Gn[2] * r.nrm[2];
                }
                g += Ga;
                if (GEO) g += Greg * E;
                const float dL_dalpha = T * (g - R);
                R = h.alpha * g + one_m * R;

                float drho = 0.f;
                if (h.a_raw < kAlphaMax) {
                    P[P_OPAC] = dL_dalpha * h.G;
                    drho = dL_dalpha * h.a_raw * -0.5f;
                }
                GSTEX_PAIR(__int_as_float(gid), px, py, __int_as_float((h.use3 ? 1 : 0) | (h.a_raw < kAlphaMax ? 0 : 2)), T,
                           w, dL_dalpha, drho, h.u, h.v, h.ipz, h.z, h.alpha, h.G, h.dx, h.dy);
                // texture coordinates
                dtu *= tex_scale;  // the raw-value differences above, in value units
                dtv *= tex_scale;
                dxr *= tex_scale;
                dyr *= tex_scale;
                // gradients of the unscaled affine (uv0, auu, ...: what setup_bwd chains), and of u, v through the
                // prescaled one
                P[P_TU0] = dtu; P[P_AUU] = dtu * h.u; P[P_AUV] = dtu * h.v;
                P[P_TV0] = dtv; P[P_AVU] = dtv * h.u; P[P_AVV] = dtv * h.v;
                float du = dxr * r.auu + dyr * r.avu;
                float dv = dxr * r.auv + dyr * r.avv;
                // ray-splat (use3) vs screen-space low-pass branch, per lane, as selects
                const float du3 = GEO ? drho * 2.0f * h.u + dz * r.Tw.x : drho * 2.0f * h.u;
                const float dv3 = GEO ? drho * 2.0f * h.v + dz * r.Tw.y : drho * 2.0f * h.v;
                du = h.use3 ? du + du3 : du;
                dv = h.use3 ? dv + dv3 : dv;
                P[P_XY + 0] = h.use3 ? 0.f : drho * (2.0f * kFilterInvSq) * (r.x - px);
                P[P_XY + 1] = h.use3 ? 0.f : drho * (2.0f * kFilterInvSq) * (r.y - py);
                const float ipz = h.ipz;
                const f3 dp = f3{du * ipz, dv * ipz, -(du * h.u + dv * h.v) * ipz};
                // p = dx A + dy B + P0 (affine form): dL/dA = dp dx, dL/dB = dp dy, dL/dP0 = dp
                P[P_A + 0] = dp.x * h.dx; P[P_A + 1] = dp.y * h.dx; P[P_A + 2] = dp.z * h.dx;
                P[P_B + 0] = dp.x * h.dy; P[P_B + 1] = dp.y * h.dy; P[P_B + 2] = dp.z * h.dy;
                P[P_P0 + 0] = dp.x; P[P_P0 + 1] = dp.y; P[P_P0 + 2] = dp.z;
                if constexpr (GEO) {  // the depth's direct dependence on Tw (z = u Tw.x + v Tw.y + Tw.z)
                    P[P_TW + 0] = h.use3 ? dz * h.u : 0.f;
                    P[P_TW + 1] = h.use3 ? dz * h.v : 0.f;
                    P[P_TW + 2] = dz;
                }
            }
            float vis_M = 0.f;  // sum over the wave's pixels of |w tex_scale| max_c |dL/dtex[c]| for this splat
            if (__any(contrib)) {
                GSTEX_STAT(2, 1);
                wave_reduce<NP>(P);
                // take the bound out of the spare slot (kMBound) before the row is stored
                constexpr int kML = GEO ? 48 : 56, kMI = GEO ? 3 : 0;  // its lane and index after the reduce-scatter
                vis_M = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(P[kMI]), kML));
                if (lane == kML) P[kMI] = 0.0f;
                // lanes 8k hold NP / 8 consecutive values each.  Deterministic mode (row_flags given): the
                // (pair, quadrant) row, whose flag (1: 24-value row, 2: 32-value row) marks it written, summed by
                // setup_bwd in a fixed order.  Otherwise: added with float atomics into the splat's NP-value
                // accumulator row (zeroed by the caller): no row traffic, no summing pass, order-dependent rounding
                constexpr int E = NP / 8;
                const int base = (NP / 2) * ((lane >> 5) & 1) + (NP / 4) * ((lane >> 4) & 1) + E * ((lane >> 3) & 1);
                if (!TRAIN && row_flags) {
                    const int slot = __builtin_amdgcn_readlane(my_slot, j);
                    if ((lane & 7) == 0) {
                        float* dst = partials + ((size_t)slot * 4 + quad) * NP + base;  // rows NP floats apart
                        if constexpr (E == 4) {
                            *reinterpret_cast<float4*>(dst) = make_float4(P[0], P[1], P[2], P[3]);
                        } else {
                            dst[0] = P[0];
                            dst[1] = P[1];
                            dst[2] = P[2];
                        }
                    }
                    if (lane == 0) row_flags[(size_t)slot * 4 + quad] = GEO ? 2 : 1;
                } else {
                    float* dst = partials + (size_t)gid * NP + base;
                    // lane 8k + e takes value e of lane 8k (DPP row shifts): one atomic instruction covers the NP
                    // contiguous floats (2 cache-line requests; E atomics from each lane 8k measured +0.2 ms)
                    const int e = lane & 7;
                    float v = P[0];
                    const float s1 = dpp_shr_f<1>(P[1]), s2 = dpp_shr_f<2>(P[2]);
                    v = e == 1 ? s1 : v;
                    v = e == 2 ? s2 : v;
                    if constexpr (E == 4) {
                        const float s3 = dpp_shr_f<3>(P[3]);
                        v = e == 3 ? s3 : v;
                    }
                    if (e < E) atomicAdd(dst + e, v);
                }
            }
            if (__any(tkey >= 0)) {
                // fixed point for this visit: every staged entry receives at most vis_M in value units (bilinear
                // weights <= 1), so at scale 2^S, S = 30 - e (vis_M < 2^e), the tails (each < 2^30) and their int32
                // sums stay in range; resolution 2^-30 of the visit's total
                // S = 30 - e with vis_M = m 2^e, m in [0.5, 1) (frexp), from the float's exponent field on the scalar
                // unit (vis_M is wave-uniform); 2^S and 2^-S are built as float bit patterns, so the scalings below
                // are exact multiplies (what ldexp computed); S is clamped to [-126, 126] (denormal / zero bounds)
                const uint32_t mbits = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(vis_M));
                const int biased = (int)((mbits >> 23) & 0xFFu);
                const int e_m = biased > 0 ? biased - 126 : 0;
                const int tex_S = min(max(kTexFixBits - e_m, -126), 126);
                const float pow_S = __uint_as_float((uint32_t)(tex_S + 127) << 23);     // 2^S
                const float pow_mS = __uint_as_float((uint32_t)(127 - tex_S) << 23);    // 2^-S
                const float twq = tw * pow_S;
                float tg[4 * CM];
                {
#pragma clang fp contract(fast)
                    const float fi0 = 1.0f - tax, fi1 = tax, fj0 = 1.0f - tay, fj1 = tay;
                    const float w00 = fi0 * fj0, w01 = fi0 * fj1;
                    const float w10 = fi1 * fj0, w11 = fi1 * fj1;
#pragma unroll
                    for (int c = 0; c < CM; ++c) {
                        const float gt = (c < Cn) ? twq * Gtex[c] : 0.0f;
                        tg[c] = gt * w00;
                        tg[CM + c] = gt * w01;
                        tg[2 * CM + c] = gt * w10;
                        tg[3 * CM + c] = gt * w11;
                    }
                }
                const bool tail = seg_reduce_rows<4 * CM>(tkey, tg);
                const int bsize = r.h * r.w * Cn;  // wave-uniform
                const bool staged = bsize <= kTexStage;
                GSTEX_STAT(5, __popcll(__ballot(tail)));
                GSTEX_STAT(7, 1);
                if (tail) {
                    const int t0 = tkey & ((1 << 29) - 1), tdi = (tkey >> 29) & 1, tdj = (tkey >> 30) & 1;
                    const int c00 = t0 * Cn, c01 = (t0 + tdj) * Cn;
                    const int c10 = (t0 + tdi * r.w) * Cn, c11 = (t0 + tdi * r.w + tdj) * Cn;
                    if (staged) {
#pragma unroll
                        for (int c = 0; c < CM; ++c) {
                            if (c < Cn) {
                                stage_add(&s_texq[c00 + c], tg[c]);
                                stage_add(&s_texq[c01 + c], tg[CM + c]);
                                stage_add(&s_texq[c10 + c], tg[2 * CM + c]);
                                stage_add(&s_texq[c11 + c], tg[3 * CM + c]);
                            }
                        }
                    } else {
                        // block larger than the staging area: straight to global, back in value units
                        float* base = v_texture + (size_t)r.off * Cn;
                        auto val = [&](float y) { return y * pow_mS; };
#pragma unroll
                        for (int c = 0; c < CM; ++c) {
                            if (c < Cn) {
                                atomicAdd(base + c00 + c, val(tg[c]));
                                atomicAdd(base + c01 + c, val(tg[CM + c]));
                                atomicAdd(base + c10 + c, val(tg[2 * CM + c]));
                                atomicAdd(base + c11 + c, val(tg[3 * CM + c]));
                            }
                        }
                    }
                }
                if (staged) {
                    // flush the block (non-zero entries only) and leave the staging area zeroed; the wave's LDS
                    // operations complete in order, so these reads see every tail added above
                    float* dst = v_texture + (size_t)r.off * Cn;
                    // kFlushU entries per lane per pass, their LDS reads issued together (one wait per pass); entries
                    // past the block are zero (the staging area is kept zeroed) and kTexStage is a multiple of the pass
                    for (int e0 = lane; e0 < bsize; e0 += 64 * kFlushU) {
                        int v[kFlushU];
                        GSTEX_STAT(4, 1);
#pragma unroll
                        for (int k = 0; k < kFlushU; ++k) v[k] = s_texq[e0 + 64 * k];
#pragma unroll
                        for (int k = 0; k < kFlushU; ++k) {
                            GSTEX_STAT(6, __popcll(__ballot(v[k] != 0)));
                            if (v[k] == 0) continue;
                            s_texq[e0 + 64 * k] = 0;
                            atomicAdd(dst + e0 + 64 * k, (float)v[k] * pow_mS);
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

// depth / distortion / normal gradients present?  (the distortion one only counts when enabled)
static bool bwd_has_geo(const gstex_raster_bwd_args* a) {
    return a->v_depth || a->v_normal || (a->v_reg && (a->scene.settings & GSTEX_SETTING_DIST_REG));
}

extern "C" int gstex_raster_bwd_variant(const gstex_raster_bwd_args* a) {
    if (!a) return -1;
    const bool train = a->scene.channels == 3 && !bwd_has_geo(a) && !a->row_flags && a->v_img && a->v_alpha &&
                       a->v_tex && a->v_tex == a->v_img;
    return train ? GSTEX_BWD_TRAIN : GSTEX_BWD_GENERIC;
}

extern "C" int gstex_raster_bwd(const gstex_raster_bwd_args* a, void* stream) {
    GSTEX_REQUIRE(a, "gstex_raster_bwd: null args");
    GSTEX_REQUIRE(a->zero_floats >= 0 && (a->zero_floats == 0 || a->zero_buf) &&
                      (!a->zero_buf || a->zero_buf != a->v_texture),
                  "gstex_raster_bwd: invalid zero_buf / zero_floats (it must not be the gradient accumulated)");
    const gstex_raster_scene& s = a->scene;
    const gstex_camera* cam = &s.cam;
    const int channels = s.channels;
    const int settings = s.settings;
    GSTEX_CHECK(check_camera("gstex_raster_bwd", cam));
    GSTEX_CHECK(check_channels("gstex_raster_bwd", channels));
    GSTEX_CHECK(check_settings("texture_gaussians", settings, kRenderSettings));
    GSTEX_REQUIRE(s.tile_ranges && s.state && s.aux,
                  "gstex_raster_bwd: null pointer (tile_ranges, state and the forward's aux)");
    GSTEX_CHECK(check_n_isect("gstex_raster_bwd", s.n_isect));
    GSTEX_REQUIRE(s.n_isect == 0 || (a->partials && s.sorted_ids && a->sorted_slots),
                  "gstex_raster_bwd: null pair buffer");
    GSTEX_CHECK(check_n_texels("gstex_raster_bwd", s.n_texels, channels));
    GSTEX_REQUIRE(s.n_texels == 0 || (s.texture && a->v_texture), "gstex_raster_bwd: null texture");
    GSTEX_REQUIRE(!(settings & GSTEX_SETTING_EVAL_NORMAL) || !a->v_normal,
                  "gstex_raster_bwd: settings bit 15 (unit-normal eval render) has no normal gradient; pass v_normal = NULL");
    const int tiles_x = (cam->W + kTile - 1) / kTile, tiles_y = (cam->H + kTile - 1) / kTile;
    CamArgs dc = to_device_camera(*cam);
    hipStream_t st = as_stream(stream);
    const AuxLayout al = aux_layout(s.n_isect, tiles_x * tiles_y, channels);
    const AuxPtrs ap = aux_ptrs(s.aux, al);
    if (s.n_isect > 0 && a->row_flags && hipMemsetAsync(a->row_flags, 0, (size_t)s.n_isect * 4, st) != hipSuccess)
        return launch_status("gstex_raster_bwd (row_flags)");
    // costliest units first, from the histogram the forward built (order entries are unit + 1)
    GSTEX_CHECK(unit_order_from_hist((int32_t)al.n_units, ap.cost, ap.order, ap.order_ws, st));
    const bool geo = bwd_has_geo(a);
    const ZeroBufs zbuf{{a->zero_floats > 0 ? a->zero_buf : nullptr, nullptr}, {a->zero_floats, 0}};
#define GSTEX_BWD(CC, ...)                                                                                     \
    raster_bwd_kernel<CC, __VA_ARGS__><<<(unsigned)al.n_units, 64, 0, st>>>(                                   \
        dc, tiles_x, settings, s.background, channels, (const float4*)s.records, s.hp_records,                \
        (const int2*)s.tile_ranges, s.sorted_ids, a->sorted_slots, s.texture, (int)s.n_texels, s.tex_scale,   \
        s.tex_bias, (const float4*)s.state, a->v_img, a->v_depth, a->v_reg, a->v_alpha, a->v_tex, a->v_normal, \
        a->partials, (unsigned char*)a->row_flags, a->v_texture, ap, zbuf)
    if (gstex_raster_bwd_variant(a) == GSTEX_BWD_TRAIN) GSTEX_BWD(3, false, /*TRAIN=*/true);
    else if (channels == 3 && !geo) GSTEX_BWD(3, false);
    else if (channels == 3) GSTEX_BWD(3, true);
    else if (channels == 6 && !geo) GSTEX_BWD(6, false);
    else if (channels == 6) GSTEX_BWD(6, true);
    else if (!geo) GSTEX_BWD(0, false);
    else GSTEX_BWD(0, true);
#undef GSTEX_BWD
    return launch_status("gstex_raster_bwd");
}
