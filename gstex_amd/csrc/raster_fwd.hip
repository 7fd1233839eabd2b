// raster_fwd.hip — the raster forward: the per-splat record build (gstex_raster_setup) and the front-to-back
// alpha-composite of per-primitive-textured 2D Gaussian splats (gstex_raster_fwd), with the aux buffer it leaves for the
// backward (gstex_raster_aux_bytes, gstex::raster_aux_zero_span; layout in raster_common.h).
//
// Replaces the forward of gstex_cuda.texture.texture_gaussians (nerfstudio/models/gstex.py:1133-1162).
//
// MI355X layout: one 256-thread workgroup (4 wave64, one 8x8 quadrant each) per 16x16 tile, launched in descending
// pair-count order (gstex_tile_order); splat records are 128-B lines staged per batch in LDS as [plane][splat] float4;
// each wave ballots the batch against its quadrant (exact ellipse-vs-rectangle test), walks the set bits, early-outs
// per lane and per workgroup; it records for the backward (aux): its cull bits, per-unit evaluation counts and
// per-pixel checkpoints at 256-position segment boundaries.
#include "raster_common.h"
#include "gstex_internal.h"
#define GSTEX_DIAG_FWD
#include "raster_diag.h"  // diagnostic builds only (GSTEX_STATS counters 8-12); empty by default

using namespace gstex;

namespace {

#ifndef GSTEX_UNIT_COARSE
#define GSTEX_UNIT_COARSE 3  // backward unit-order cost buckets of 2^k visits (inside a bucket: about slot order,
                             // better L2 reuse of texel blocks). Measured: 3 same time, bwd fetch -18 %; 5, 6 slower
#endif
#ifndef GSTEX_FWD_OCC
#define GSTEX_FWD_OCC 6  // forward waves per SIMD the register allocation targets (measured: 8 at 64 VGPRs is slower; 5 with
                         // a record prefetch or a second pending texel set, both measured slower in round 5)
#endif
#ifndef GSTEX_XCD_MB
#define GSTEX_XCD_MB 2  // backward units of one 2x2-tile macro-block dispatched to one XCD (unit_order groups)
#endif
#ifndef GSTEX_FWD_DEFER
#define GSTEX_FWD_DEFER 1
#endif
constexpr bool kFwdDefer = GSTEX_FWD_DEFER;  // forward: texel gathers folded in one visit later (C = 3)

// ------------------------------------------------------------------------------------------
// setup: per-splat record
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void setup_kernel(int n, const float* __restrict__ means,
                                                    const float* __restrict__ scales, float glob,
                                                    const float* __restrict__ quats,
                                                    const float* __restrict__ rgbs,
                                                    const float* __restrict__ opacities,
                                                    const float* __restrict__ centers,
                                                    const float* __restrict__ uv0,
                                                    const float* __restrict__ umap,
                                                    const float* __restrict__ vmap,
                                                    const int32_t* __restrict__ tdims,
                                                    const int32_t* __restrict__ nth, CamArgs cam_args,
                                                    float* __restrict__ rec_out, double* __restrict__ hp_out) {
    const Camera cam = load_camera(cam_args);
    int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    if (nth[g] <= 0) return;
    // the record, in fp64 (splat_math.h: the function the training prologue's fused kernel also calls)
    splat_record(cam, means[3 * g], means[3 * g + 1], means[3 * g + 2], scales[3 * g], scales[3 * g + 1], glob,
                 quats + 4 * g, rgbs + 3 * g, opacities[g], centers[2 * g], centers[2 * g + 1], uv0 + 2 * g,
                 umap + 3 * g, vmap + 3 * g, tdims + 3 * g, rec_out + (size_t)g * GSTEX_REC_FLOATS,
                 hp_out ? hp_out + (size_t)g * H_FIELDS : nullptr);
}

__host__ __device__ __forceinline__ int fwd_grid(int tiles_x, int tiles_y) { return tiles_x * tiles_y; }

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// acc + w (tex_scale * bilinear(v) + tex_bias) in lerp form with fused multiply-adds (8 VALU per channel instead of
// 13): no threshold decision depends on a texel value, so it is compared with the oracle within tolerance only
__device__ __forceinline__ float tex_accum(float acc, float v00, float v01, float v10, float v11, float ax, float ay,
                                           float s, float b, float w) {
    const float top = __builtin_fmaf(ay, v01 - v00, v00);
    const float bot = __builtin_fmaf(ay, v11 - v10, v10);
    const float mix = __builtin_fmaf(ax, bot - top, top);
    return __builtin_fmaf(__builtin_fmaf(mix, s, b), w, acc);
}
// GEOF = false: depth / distortion / normal not produced (their outputs are NULL: a caller whose loss does
// not use them, e.g. the photometric training step); every other output is computed unchanged.
// One 256-thread workgroup per tile; its four quadrant waves share 128-record batches staged in LDS (a barrier per
// batch).  (One wave64 workgroup per (tile, quadrant) with scalar record loads measured 12 % slower in round 3: the
// shared staging reads each record once per tile instead of once per quadrant.)
template <int C, bool GEOF>
__global__ __launch_bounds__(kThreads, GSTEX_FWD_OCC) void raster_fwd_kernel(
    CamArgs cam_args, int tiles_x, int settings, const float* __restrict__ bg, int Cdyn,
    const float4* __restrict__ records, const double* __restrict__ hp_records, const int2* __restrict__ tile_ranges,
    const int32_t* __restrict__ tile_order,
    const int32_t* __restrict__ sorted_ids, const float* __restrict__ texture, int n_texels, float tex_scale,
    float tex_bias, float* __restrict__ out_img,
    float* __restrict__ out_depth, float* __restrict__ out_reg, float* __restrict__ out_alpha,
    float* __restrict__ out_tex, float* __restrict__ out_normal, float4* __restrict__ state, AuxPtrs aux,
    int n_tiles, const ZeroBufs zb) {
    const Camera cam = load_camera(cam_args);
    unsigned long long* __restrict__ visit_masks = aux.masks;
    zero_bufs(zb);
    constexpr int CM = (C > 0) ? C : 8;  // register capacity for the runtime-C path
    const int Cn = (C > 0) ? C : Cdyn;
    constexpr int kStep = kFwdBatch, kWords = kStep / 64;
    __shared__ float4 s_rec[kRecF4 * kFwdBatch];
    __shared__ int s_gid[kFwdBatch];  // the batch's splat ids (the near-edge-on splats' fp64 rows are read by id)
    // the next batch's ids, copied global -> LDS (no VGPR) during the current batch's visits, so the batch staging's
    // record loads do not wait on a dependent id load first (raster loop at cfg3: forward 0.510 vs 0.5155 ms)
    __shared__ int s_gid_next[kFwdBatch];
    const int ti = (int)blockIdx.x;
    const int tile = tile_order ? tile_order[ti] : ti;  // largest-first when given
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = (int)threadIdx.x;
    const WaveBlock wb = wave_block(tx, ty, tid);
    const int pxi = wb.px, pyi = wb.py;
    const bool inside = pxi < cam.W && pyi < cam.H;
    const float px = (float)pxi + 0.5f, py = (float)pyi + 0.5f;  // pixel centres (gstex_common.h)
    const bool aa = (settings & GSTEX_SETTING_AA_BLUR) != 0;
    const bool dreg = (settings & GSTEX_SETTING_DIST_REG) != 0;
    const int2 rng = tile_ranges[tile];
    const float bg0 = bg ? bg[0] : 0.f, bg1 = bg ? bg[1] : 0.f, bg2 = bg ? bg[2] : 0.f;
    const float wx0 = wb.wx0, wx1 = wb.wx1, wy0 = wb.wy0, wy1 = wb.wy1;

    float T = 1.0f;
    float img[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
    float tex[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) tex[c] = 0.f;
    float D = 0.f, M1 = 0.f, M2 = 0.f, reg = 0.f;
    int last = -1;
    // per-lane "still running" as a float, not a bool: a bool carried around the visit loop becomes an SGPR lane
    // mask that the compiler re-merges with exec at every join (three SALU per join; measured: the forward with the
    // divergent per-lane loop exits and bool lane state 0.595 ms, with this loop 0.550 ms)
    float alive = inside ? 1.0f : 0.0f;
#define GSTEX_FWD_DONE (alive == 0.0f)
    // Deferred texel accumulation (kFwdDefer): a visit's four texel gathers are issued into the pending registers
    // and folded into tex[] at the lane's next contributing visit (or at a checkpoint / the end), so their latency
    // overlaps the next visit's record read and pair evaluation.  Same values, same order of accumulation.
    constexpr bool kDefer = kFwdDefer && C == 3;
    float pend = 0.0f;  // (a float: see `alive`)
    float p00[CM], p01[CM], p10[CM], p11[CM], pax = 0.f, pay = 0.f, pw = 0.f;
    // kDefer: tex[c] accumulates sum_k w_k bilerp_k(texels) with the weight folded into the four corner weights (4
    // fused multiply-adds per channel), texw = sum_k w_k over the textured visits, and the affine (tex_scale, tex_bias)
    // is applied once, by tex_value(): sum_k w_k (s m_k + b) = s sum_k w_k m_k + b sum_k w_k (9 + 4 C VALU per visit
    // instead of 8 C; no decision depends on a texel value)
    float texw = 0.0f;
    auto fold_set = [&](float (&a00)[CM], float (&a01)[CM], float (&a10)[CM], float (&a11)[CM], float ax, float ay,
                        float aw, float& apend) {
        if (kDefer && apend != 0.0f) {
            const float c1 = aw * ax, c0 = aw * (1.0f - ax), qy = 1.0f - ay;
            const float w00 = c0 * qy, w01 = c0 * ay, w10 = c1 * qy, w11 = c1 * ay;
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c < Cn)
                    tex[c] = __builtin_fmaf(a11[c], w11, __builtin_fmaf(a10[c], w10, __builtin_fmaf(a01[c], w01,
                             __builtin_fmaf(a00[c], w00, tex[c]))));
            }
            texw = texw + aw;
            apend = 0.0f;
        }
    };
    auto fold_pending = [&]() { fold_set(p00, p01, p10, p11, pax, pay, pw, pend); };
    auto tex_value = [&](int c) {  // the texture output of channel c so far
        return kDefer ? __builtin_fmaf(tex[c], tex_scale, tex_bias * texw) : tex[c];
    };
    const int lane = tid & 63, wave = tid >> 6;
    const size_t vm_base = visit_mask_base(rng.x, tile);
    const int sbase = seg_base(rng.x, tile);
    int seg_visits = 0, cur_seg = 0;  // this wave's splat evaluations in the current segment (backward cost)
    // XCD group of the tile's backward units: its GSTEX_XCD_MB x GSTEX_XCD_MB-tile macro-block
    const int xgroup = (((tx / GSTEX_XCD_MB) + (ty / GSTEX_XCD_MB) * ((tiles_x + GSTEX_XCD_MB - 1) / GSTEX_XCD_MB)) & 7)
                       << 24;
    if (aux.slot_tile)
        for (int k = tid; k * kSegLen < rng.y - rng.x; k += kThreads) aux.slot_tile[sbase + k] = tile;
    // one checkpoint record: field f of the wave's lane at ckpt[((slot * 4 + wave) * F + f) * 64 + lane]
    auto write_ck = [&](int slot) {
        float* ck = aux.ckpt + ((size_t)slot * 4 + wave) * aux.F * 64 + lane;
        ck[0] = T;
        ck[64] = img[0];
        ck[128] = img[1];
        ck[192] = img[2];
#pragma unroll
        for (int c = 0; c < CM; ++c)
            if (c < Cn) ck[(4 + c) * 64] = tex_value(c);
        if (GEOF) {
            float* g = ck + (4 + Cn) * 64;
            g[0] = D;
            g[64] = nrm[0];
            g[128] = nrm[1];
            g[192] = nrm[2];
            g[256] = M1;
            g[320] = M2;
        }
    };

    if (tid < kFwdBatch && rng.x + tid < rng.y) s_gid_next[tid] = sorted_ids[rng.x + tid];  // the first batch's
    for (int b0 = rng.x; b0 < rng.y; b0 += kStep) {
        if (aux.cost && b0 > rng.x && (b0 - rng.x) % kSegLen == 0) {
            // segment cur_seg complete: its cost, and the state after it while a lane of the wave still runs
            const int cnt = wave_max_i(seg_visits);  // lanes leave the visit loop as they finish: the wave's count
            if (lane == 0 && cnt) {
                const int key = ((cnt >> GSTEX_UNIT_COARSE) + 1) | xgroup;
                aux.cost[(sbase + cur_seg) * 4 + wave] = key;
                atomicAdd(&aux.order_ws[unit_bin(key)], 1);  // the backward's unit-order histogram
            }
            fold_pending();
            if (__any(!GSTEX_FWD_DONE)) write_ck(sbase + cur_seg);
            seg_visits = 0;
            ++cur_seg;
        }
        const int nb = min(kStep, rng.y - b0);
        if (__syncthreads_count(GSTEX_FWD_DONE ? 1 : 0) == kThreads) break;
        for (int q = tid; q < kFwdBatch * kRecF4; q += kThreads) {
            const int j = q / kRecF4, k = q % kRecF4;
            if (b0 + j < rng.y) {
                const int gid = s_gid_next[j];
                s_rec[k * kFwdBatch + j] = records[(size_t)gid * kRecF4 + k];
                if (k == 0) s_gid[j] = gid;
            }
        }
        __syncthreads();
        if (tid < kFwdBatch && b0 + kStep < rng.y) {  // waves 0-1: lane l of wave w fetches id kStep + 64 w + l ahead
            const int nx = min(b0 + kStep + tid, rng.y - 1);  // (past the list: a valid address, value unused)
            __builtin_amdgcn_global_load_lds(const_cast<int32_t*>(sorted_ids + nx), s_gid_next + (tid & ~63), 4, 0, 0);
        }
        // the batch splats whose contribution region meets this wave's 8x8 block, tested all at once
        unsigned long long todo[kWords];
#pragma unroll
        for (int hb = 0; hb < kWords; ++hb) {
            const int jj = hb * 64 + lane;
            const bool hit = jj < nb && wave_may_hit<kFwdBatch>(s_rec, jj < nb ? jj : 0, wx0, wx1, wy0, wy1, aa);
            todo[hb] = __ballot(hit);
            GSTEX_STAT(8, (unsigned long long)max(0, min(64, nb - hb * 64)));  // cull candidates (wave, splat)
            GSTEX_STAT(9, __popcll(todo[hb]));                                 // passing the wave's cull
            // hand the cull to the backward, which visits these splats up to the wave's last contributor
            if (visit_masks && lane == 0 && hb * 64 < nb)
                visit_masks[(vm_base + ((b0 - rng.x) >> 6) + hb) * 4 + wave] = todo[hb];
        }
        // wave-uniform visit loop: finished lanes stay in it with their updates predicated off (no divergent exits:
        // the loop control is a scalar bit scan, not exec-mask bookkeeping); it ends when the batch's bits run out
        // or every lane of the wave has finished
        bool all_done = __all(GSTEX_FWD_DONE);
        for (int hb = 0; hb < kWords && !all_done; ++hb) {
          unsigned long long m = todo[hb];
          while (m) {
            const int j = hb * 64 + __builtin_ctzll(m);
            m &= m - 1;
            const Rec r = read_rec<kFwdBatch>(s_rec, j);
            ++seg_visits;
            Hit h;
            hit_p(r, px, py, h);
            // a near-edge-on splat (the record opacity's sign bit, wave-uniform): p from its fp64 row
            if (hp_records && __builtin_amdgcn_readfirstlane(__float_as_int(r.mark)) < 0)
                hit_p_hp_uniform(hp_records + (size_t)__builtin_amdgcn_readfirstlane(s_gid[j]) * H_FIELDS, px, py, h);
            const bool ok = eval_rest(r, px, py, aa, h) && alive != 0.0f;
            const float test_T = T * (1.0f - h.alpha);
            const bool stop = ok && test_T < kTMin;
            GSTEX_STAT(10, 1);                                    // visits (the wave evaluates a splat)
            GSTEX_STAT(11, __ballot(ok) ? 1 : 0);                 // ... with a contributing lane
            GSTEX_STAT(12, __popcll(__ballot(ok && !stop)));      // contributing lanes
            alive = stop ? 0.0f : alive;
            if (ok && !stop) {
                const float w = h.alpha * T;
                const int bh = __builtin_amdgcn_readfirstlane(r.h), bw = __builtin_amdgcn_readfirstlane(r.w);
                const int boff = __builtin_amdgcn_readfirstlane(r.off);
                const bool has_tex = bh * bw > 0 && boff + bh * bw <= n_texels;
                if (kDefer) {
                    // (computed whether or not the splat has texels: used only when it has)
                    float tu, tv;
                    tex_coords(r, h.u, h.v, tu, tv);
                    const Bilerp b = bilerp_xy(tu, tv, bh, bw, r.hm1, r.wm1);
                    fold_pending();
                    if (has_tex) {
                        const __amdgpu_buffer_rsrc_t rs = texel_rsrc(texture, boff, bh * bw, Cn);
                        if constexpr (CM == 3) load_texel_quad_unclamped(rs, b, bw, p00, p01, p10, p11);
                        else load_texel_quad<CM>(rs, b, bw, Cn, p00, p01, p10, p11);
                        pax = b.ax;
                        pay = b.ay;
                        pw = w;
                        pend = 1.0f;
                    }
                } else if (has_tex) {
                    float tu, tv;
                    tex_coords(r, h.u, h.v, tu, tv);
                    const Bilerp b = bilerp_xy(tu, tv, r.h, r.w, r.hm1, r.wm1);
                    const __amdgpu_buffer_rsrc_t rs = texel_rsrc(texture, boff, bh * bw, Cn);
                    float t00[CM], t01[CM], t10[CM], t11[CM];
                    load_texel_quad<CM>(rs, b, bw, Cn, t00, t01, t10, t11);
#pragma unroll
                    for (int c = 0; c < CM; ++c)
                        if (c < Cn) tex[c] = tex_accum(tex[c], t00[c], t01[c], t10[c], t11[c], b.ax, b.ay, tex_scale, tex_bias, w);
                }
                img[0] = __builtin_fmaf(r.rgb[0], w, img[0]);
                img[1] = __builtin_fmaf(r.rgb[1], w, img[1]);
                img[2] = __builtin_fmaf(r.rgb[2], w, img[2]);
                if (GEOF) {
                    D = D + h.z * w;
                    nrm[0] = nrm[0] + r.nrm[0] * w;
                    nrm[1] = nrm[1] + r.nrm[1] * w;
                    nrm[2] = nrm[2] + r.nrm[2] * w;
                }
                if (GEOF && dreg) {
                    const float A = 1.0f - T;
                    const float mm = kFarRatio * (1.0f - kNear * grad_rcp(h.z));
                    reg = reg + ((mm * mm * A + M2) - 2.0f * mm * M1) * w;
                    M1 = M1 + mm * w;
                    M2 = M2 + mm * mm * w;
                }
                T = test_T;
                last = b0 - rng.x + j;
            }
            if (__builtin_amdgcn_ballot_w64(alive != 0.0f) == 0) {
                all_done = true;
                break;
            }
          }
        }
    }
    fold_pending();
    if (aux.cost) {
        const int cnt = wave_max_i(seg_visits);
        if (lane == 0 && cnt) {
            const int key = ((cnt >> GSTEX_UNIT_COARSE) + 1) | xgroup;
            aux.cost[(sbase + cur_seg) * 4 + wave] = key;
            atomicAdd(&aux.order_ws[unit_bin(key)], 1);
        }
        // final accumulators for the backward's earlier segments, in the slot of the wave's last segment
        const int wl = wave_max_i(last);
        if (wl >= kSegLen) write_ck(sbase + wl / kSegLen);
    }
    if (!inside) return;
    const size_t pix = (size_t)pyi * cam.W + pxi;
    out_img[3 * pix + 0] = img[0] + T * bg0;
    out_img[3 * pix + 1] = img[1] + T * bg1;
    out_img[3 * pix + 2] = img[2] + T * bg2;
    if (GEOF) {
        out_depth[pix] = D;
        out_reg[pix] = reg;
    }
    out_alpha[pix] = 1.0f - T;
#pragma unroll
    for (int c = 0; c < CM; ++c)
        if (c < Cn) out_tex[(size_t)Cn * pix + c] = tex_value(c);
    if (GEOF) {
        if (settings & GSTEX_SETTING_EVAL_NORMAL) {
            // bit 15 (gstex.py:1198-1203, the eval "clean normal" render): the accumulated normal is returned
            // as a unit vector (0 where nothing was accumulated); every other output is unchanged
            const float n2 = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2];
            const float inv = n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
            nrm[0] = nrm[0] * inv;
            nrm[1] = nrm[1] * inv;
            nrm[2] = nrm[2] * inv;
        }
        out_normal[3 * pix + 0] = nrm[0];
        out_normal[3 * pix + 1] = nrm[1];
        out_normal[3 * pix + 2] = nrm[2];
    }
    state[pix] = make_float4(T, M1, M2, __int_as_float(last));
}

}  // namespace

namespace gstex {
ZeroSpan raster_aux_zero_span(void* aux, int64_t n_isect, int32_t n_tiles, int32_t channels) {
    const AuxLayout al = aux_layout(n_isect, n_tiles, channels);
    return ZeroSpan{aux ? (char*)aux + al.cost : nullptr, al.order_ws - al.cost + (size_t)2 * kUnitBins * 4};
}
}  // namespace gstex

extern "C" int gstex_raster_setup(int32_t n, const float* means, const float* scales, float glob_scale,
                                  const float* quats, const float* rgbs, const float* opacities,
                                  const float* centers, const float* uv0, const float* umap, const float* vmap,
                                  const int32_t* texture_dims, const int32_t* num_tiles_hit,
                                  const gstex_camera* cam, float* records, double* hp_records, void* stream) {
    GSTEX_REQUIRE(n >= 0 && cam, "gstex_raster_setup: invalid arguments");
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(means && scales && quats && rgbs && opacities && centers && uv0 && umap && vmap &&
                      texture_dims && num_tiles_hit && records,
                  "gstex_raster_setup: null pointer");
    setup_kernel<<<div_up(n, 256), 256, 0, as_stream(stream)>>>(n, means, scales, glob_scale, quats, rgbs, opacities,
                                                                 centers, uv0, umap, vmap, texture_dims,
                                                                 num_tiles_hit, to_device_camera(*cam), records,
                                                                 hp_records);
    return launch_status("gstex_raster_setup");
}

extern "C" int gstex_raster_fwd(const gstex_raster_fwd_args* a, void* stream) {
    GSTEX_REQUIRE(a, "gstex_raster_fwd: null args");
    GSTEX_REQUIRE(a->zero_floats >= 0 && (a->zero_floats == 0 || a->zero_buf) && a->zero_floats2 >= 0 &&
                  (a->zero_floats2 == 0 || a->zero_buf2), "gstex_raster_fwd: invalid zero_buf / zero_floats");
    const gstex_raster_scene& s = a->scene;
    const gstex_camera* cam = &s.cam;
    const int channels = s.channels;
    GSTEX_CHECK(check_camera("gstex_raster_fwd", cam));
    GSTEX_CHECK(check_channels("gstex_raster_fwd", channels));
    GSTEX_CHECK(check_n_texels("gstex_raster_fwd", s.n_texels, channels));
    GSTEX_REQUIRE(s.n_texels == 0 || s.texture, "gstex_raster_fwd: null texture");
    GSTEX_CHECK(check_settings("texture_gaussians", s.settings, kRenderSettings));
    GSTEX_REQUIRE(s.tile_ranges && a->out_img && a->out_alpha && a->out_tex && s.state,
                  "gstex_raster_fwd: null pointer");
    const bool geo = a->out_depth || a->out_reg || a->out_normal;
    GSTEX_REQUIRE(!geo || (a->out_depth && a->out_reg && a->out_normal),
                  "gstex_raster_fwd: out_depth, out_reg and out_normal must be all given or all NULL");
    GSTEX_CHECK(check_n_isect("gstex_raster_fwd", s.n_isect));
    const int tiles_x = (cam->W + kTile - 1) / kTile, tiles_y = (cam->H + kTile - 1) / kTile;
    CamArgs dc = to_device_camera(*cam);
    hipStream_t st = as_stream(stream);
    const int nblk = tiles_x * tiles_y;
    const AuxLayout al = aux_layout(s.n_isect, nblk, channels);
    const AuxPtrs ap = aux_ptrs(s.aux, al);
    // one fill: unit costs (units the forward never reaches keep 0; the backward skips them), the launch order
    // (0 = no unit at that position) and the unit-order histogram the forward builds (contiguous in the layout)
    if (s.aux && !a->aux_zeroed &&
        hipMemsetAsync(ap.cost, 0, al.order_ws - al.cost + (size_t)2 * kUnitBins * 4, st) != hipSuccess)
        return launch_status("gstex_raster_fwd (aux)");
    ZeroBufs zbuf;
    zbuf.p[0] = a->zero_floats > 0 ? a->zero_buf : nullptr;
    zbuf.n[0] = a->zero_floats;
    zbuf.p[1] = a->zero_floats2 > 0 ? a->zero_buf2 : nullptr;
    zbuf.n[1] = a->zero_floats2;
    int fgrid = fwd_grid(tiles_x, tiles_y);
#define GSTEX_FWD(CC, GG)                                                                                      \
    raster_fwd_kernel<CC, GG><<<fgrid, kThreads, 0, st>>>(                                                    \
        dc, tiles_x, s.settings, s.background, channels, (const float4*)s.records, s.hp_records,              \
        (const int2*)s.tile_ranges, a->tile_order, s.sorted_ids, s.texture, (int)s.n_texels, s.tex_scale,     \
        s.tex_bias, a->out_img, a->out_depth, a->out_reg, a->out_alpha, a->out_tex, a->out_normal,            \
        (float4*)s.state, ap, nblk, zbuf)
    if (channels == 3 && geo) GSTEX_FWD(3, true);
    else if (channels == 3) GSTEX_FWD(3, false);
    else if (channels == 6 && geo) GSTEX_FWD(6, true);
    else if (channels == 6) GSTEX_FWD(6, false);
    else if (geo) GSTEX_FWD(0, true);
    else GSTEX_FWD(0, false);
#undef GSTEX_FWD
    return launch_status("gstex_raster_fwd");
}

extern "C" size_t gstex_raster_aux_bytes(int64_t n_isect, int32_t n_tiles, int32_t channels) {
    if (n_isect < 0 || n_tiles < 0 || channels < 1 || channels > 8) return 0;
    return aux_layout(n_isect, n_tiles, channels).bytes;
}
