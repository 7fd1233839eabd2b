// raster_chain.h — the record chain of the raster's setup backward: one splat's summed partials (a kPartRowGeo row)
// chained through the fp64 record to its parameters' gradients, FOLD_AABB adding get_aabb_2d's centre backward.  One
// definition for its two users: setup_bwd_chain_kernel (raster_setup_bwd.hip) and the fused step's
// train_epilogue_kernel (trainstep_epilogue.hip).
#pragma once

#include "gstex_common.h"
#include "splat_math.h"

namespace gstex {

template <bool FOLD_AABB>
__device__ __forceinline__ void setup_bwd_chain(int g, const float (&S)[kPartRowGeo], int cnt, const Camera& cam,
    const float* __restrict__ means, const float* __restrict__ scales, float glob,
    const float* __restrict__ quats, const float* __restrict__ umap, const float* __restrict__ vmap,
    float* __restrict__ v_means, float* __restrict__ v_scales, float* __restrict__ v_quats,
    float* __restrict__ v_rgbs, float* __restrict__ v_opac, float* __restrict__ v_centers, float* __restrict__ v_uv0) {
    v_rgbs[3 * g + 0] = S[P_RGB + 0];
    v_rgbs[3 * g + 1] = S[P_RGB + 1];
    v_rgbs[3 * g + 2] = S[P_RGB + 2];
    v_opac[g] = S[P_OPAC];
    v_centers[2 * g + 0] = S[P_XY + 0];
    v_centers[2 * g + 1] = S[P_XY + 1];
    v_uv0[2 * g + 0] = S[P_TU0];
    v_uv0[2 * g + 1] = S[P_TV0];
    if (cnt <= 0) {
        v_means[3 * g] = v_means[3 * g + 1] = v_means[3 * g + 2] = 0.f;
        v_scales[3 * g] = v_scales[3 * g + 1] = v_scales[3 * g + 2] = 0.f;
        v_quats[4 * g] = v_quats[4 * g + 1] = v_quats[4 * g + 2] = v_quats[4 * g + 3] = 0.f;
        return;
    }
    // fp64 chain (one thread per splat): the record it differentiates was evaluated in fp64 (setup_kernel)
    const FrameT<double> fr = quat_frame_t<double>(quats + 4 * g);
    const double su = (double)scales[3 * g] * (double)glob, sv = (double)scales[3 * g + 1] * (double)glob;
    const d3 mu = d3{(double)means[3 * g], (double)means[3 * g + 1], (double)means[3 * g + 2]};
    const AnchoredT<double> an = splat_anchored(cam, mu, su, sv, fr);
    d3 dTu, dTv, dTw;
    auto sd = [&](int i) { return d3{(double)S[i], (double)S[i + 1], (double)S[i + 2]}; };
    affine_homog_vjp(an.Tu, an.Tv, an.Tw, sd(P_A), sd(P_B), sd(P_P0), dTu, dTv, dTw);
    dTw = add3(dTw, sd(P_TW));
    const HomogGradT<double> hg = splat_anchored_vjp(cam, su, sv, fr, an.xn, an.yn, dTu, dTv, dTw);
    const d3 um = d3{(double)umap[3 * g], (double)umap[3 * g + 1], (double)umap[3 * g + 2]};
    const d3 vm = d3{(double)vmap[3 * g], (double)vmap[3 * g + 1], (double)vmap[3 * g + 2]};
    const double dauu = S[P_AUU], dauv = S[P_AUV], davu = S[P_AVU], davv = S[P_AVV];
    const double dsu = hg.dsu + dauu * dot3(fr.tu, um) + davu * dot3(fr.tu, vm);
    const double dsv = hg.dsv + dauv * dot3(fr.tv, um) + davv * dot3(fr.tv, vm);
    const d3 dtu = add3(hg.dtu, add3(scale3(um, dauu * su), scale3(vm, davu * su)));
    const d3 dtv = add3(hg.dtv, add3(scale3(um, dauv * sv), scale3(vm, davv * sv)));
    const d3 dir = d3{(double)cam.campos[0] - mu.x, (double)cam.campos[1] - mu.y, (double)cam.campos[2] - mu.z};
    const double sgn = dot3(fr.tw, dir) < 0.0 ? -1.0 : 1.0;
    const d3 dtw = d3{sgn * S[P_NRM], sgn * S[P_NRM + 1], sgn * S[P_NRM + 2]};
    double dqd[4];
    frame_vjp(fr, dtu, dtv, dtw, dqd);
    // rounded to fp32 once; the folded AABB-centre chain below stays fp32 (bit-identical to get_aabb_2d's backward)
    f3 vmu = to_f3(hg.dmu);
    float vsu = (float)(dsu * (double)glob), vsv = (float)(dsv * (double)glob);
    float dq[4] = {(float)dqd[0], (float)dqd[1], (float)dqd[2], (float)dqd[3]};
    if (FOLD_AABB) {
        // aabb_bwd_kernel for this splat (zero when there is no centre gradient or the splat is culled)
        f3 amu = f3{0.f, 0.f, 0.f};
        float asu = 0.f, asv = 0.f, aq[4] = {0.f, 0.f, 0.f, 0.f};
        const float gcx = S[P_XY + 0], gcy = S[P_XY + 1];
        float acx, acy, aex, aey;
        const Frame frf = quat_frame(quats + 4 * g);
        const float suf = scales[3 * g] * glob, svf = scales[3 * g + 1] * glob;
        const Homog ah = splat_homography(cam, mk3(means[3 * g], means[3 * g + 1], means[3 * g + 2]), suf, svf, frf);
        if (!(gcx == 0.0f && gcy == 0.0f) && aabb_from_homog(ah, acx, acy, aex, aey)) {
            f3 dTu, dTv, dTw;
            aabb_centre_vjp(ah, acx, acy, gcx, gcy, dTu, dTv, dTw);
            const HomogGrad ag = splat_homography_vjp(cam, suf, svf, frf, dTu, dTv, dTw);
            frame_vjp(frf, ag.dtu, ag.dtv, f3{0.0f, 0.0f, 0.0f}, aq);
            amu = ag.dmu;
            asu = ag.dsu * glob;
            asv = ag.dsv * glob;
        }
        vmu = add3(vmu, amu);
        vsu = vsu + asu;
        vsv = vsv + asv;
#pragma unroll
        for (int k = 0; k < 4; ++k) dq[k] = dq[k] + aq[k];
    }
    v_means[3 * g + 0] = vmu.x;
    v_means[3 * g + 1] = vmu.y;
    v_means[3 * g + 2] = vmu.z;
    v_scales[3 * g + 0] = vsu;
    v_scales[3 * g + 1] = vsv;
    v_scales[3 * g + 2] = 0.f;
    v_quats[4 * g + 0] = dq[0];
    v_quats[4 * g + 1] = dq[1];
    v_quats[4 * g + 2] = dq[2];
    v_quats[4 * g + 3] = dq[3];
}

}  // namespace gstex
