// select.hip — keep a subset of the splats of a textured model: the jagged texel store compacted by a per-splat mask
// (not in the reference, whose clustering tool writes a new file instead; DESIGN.md "Selecting splats").
//
//   gstex_select_plan    one thread per splat: rows[i] = keep ? 1 : 0, texels[i] = keep ? h * w : 0, and a flag word
//                        that any malformed dims row (kept or not) sets
//   gstex_select_dims    one thread per splat: a kept splat's new dims row (h, w, new offset) and its source offset
//   gstex_select_texels  the jagged gather of up to GSTEX_SELECT_MAX_TENSORS (src, dst) pairs, destination-indexed
//
// Between plan and dims the caller runs gstex_scan_offsets over rows and over texels and reads (n_new, T_new, flag)
// back in one copy (the operation's only synchronisation).  Per-splat tensors go through gstex_density_apply with
// rows as planned here and every kind KEEP.  Nothing below rounds: every value is copied.
#include "gstex_common.h"
#include "gstex_error.h"

using namespace gstex;

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 1024;  // destination texels per workgroup of the texel gather (4 KB of LDS)
constexpr int kMaxTensors = GSTEX_SELECT_MAX_TENSORS;
constexpr int kBatch = 4;  // words per lane and tensor in flight in the texel gather's copy loop

__global__ __launch_bounds__(kThreads) void select_plan_kernel(int n, long long n_texels,
                                                               const uint8_t* __restrict__ keep,
                                                               const int32_t* __restrict__ dims,
                                                               int32_t* __restrict__ rows, int32_t* __restrict__ texels,
                                                               int32_t* flag) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int h = dims[3 * (size_t)i], w = dims[3 * (size_t)i + 1], off = dims[3 * (size_t)i + 2];
    const long long hw = (long long)h * (long long)w;  // |h|, |w| < 2^31: no overflow in 64 bits
    const bool bad = h < 0 || w < 0 || off < 0 || hw > 0x7fffffffll || (long long)off + hw > n_texels;
    const bool k = keep[i] != 0;
    rows[i] = k ? 1 : 0;
    texels[i] = (k && !bad) ? (int)hw : 0;
    if (bad) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kThreads) void select_dims_kernel(int n, int n_new, const uint8_t* __restrict__ keep,
                                                               const int32_t* __restrict__ dims,
                                                               const int32_t* __restrict__ row_off,
                                                               const int32_t* __restrict__ tex_off,
                                                               int32_t* __restrict__ new_dims,
                                                               int32_t* __restrict__ src_off) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || keep[i] == 0) return;
    const int j = row_off[i];
    if (j < 0 || j >= n_new) return;  // never past the n_new rows the caller allocated
    new_dims[3 * (size_t)j] = dims[3 * (size_t)i];
    new_dims[3 * (size_t)j + 1] = dims[3 * (size_t)i + 1];
    new_dims[3 * (size_t)j + 2] = tex_off[i];
    src_off[j] = dims[3 * (size_t)i + 2];
}

struct TexelArgs {
    gstex_select_pair t[kMaxTensors];
    int n_tensors, n_new, channels;
    long long T_new, n_texels;
    const int32_t *new_dims, *src_off;
};

// The first k in [lo, hi) with new offset > t (hi when there is none); offsets are non-decreasing.  32 halvings cover
// any int range, so the bound is static.
__device__ __forceinline__ int first_above(const int32_t* __restrict__ new_dims, int lo, int hi, long long t) {
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)new_dims[3 * (size_t)mid + 2] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup owns kRun consecutive destination texels [t0, t1).  The chart of texel t is the LAST j with
// new_off_j <= t: zero-texel charts share their successor's offset, so the rule passes over them.  Two wave-uniform
// searches bound the run's charts [j0, j1]; each lane then resolves its texels inside that range (no lane walks a
// chart) and leaves the SOURCE texel in LDS; after the barrier the run is copied element by element, consecutive lanes
// writing consecutive words of every destination and reading consecutive words within each source block.  A texel
// whose chart does not cover it or whose source lies outside the store (arrays that are not a plan's) is skipped.
template <int kC>
__global__ __launch_bounds__(kThreads) void select_texels_kernel(const TexelArgs a) {
    __shared__ int32_t src_texel[kRun];
    const int C = kC > 0 ? kC : a.channels;
    const long long t0 = (long long)blockIdx.x * kRun;
    const long long t1 = t0 + kRun < a.T_new ? t0 + kRun : a.T_new;
    const int run = (int)(t1 - t0);  // >= 1: the grid has ceil(T_new / kRun) workgroups
    const int j0 = first_above(a.new_dims, 0, a.n_new, t0) - 1;
    const int j1 = first_above(a.new_dims, j0 < 0 ? 0 : j0, a.n_new, t1 - 1) - 1;
    for (int l = threadIdx.x; l < kRun; l += kThreads) {
        int s = -1;
        if (l < run && j0 >= 0) {
            const long long t = t0 + l;
            int j = first_above(a.new_dims, j0, j1 + 1, t) - 1;
            j = j < j0 ? j0 : j;  // (new_off_j0 <= t0 <= t: only offsets that are not sorted get here)
            const long long local = t - (long long)a.new_dims[3 * (size_t)j + 2];
            const long long size = (long long)a.new_dims[3 * (size_t)j] * (long long)a.new_dims[3 * (size_t)j + 1];
            const long long from = (long long)a.src_off[j] + local;
            if (local >= 0 && local < size && from >= 0 && from < a.n_texels) s = (int)from;  // n_texels < 2^31
        }
        src_texel[l] = s;
    }
    __syncthreads();
    const int words = run * C;
    const long long base = t0 * C;
    // kBatch words per lane are loaded before the first is stored (src and dst may alias as far as the compiler knows,
    // so it would not move a load above a store by itself): more bytes in flight per wave.  A skipped word loads
    // word 0, which exists (n_texels > 0), and stores nothing.
    for (int e0 = threadIdx.x; e0 < words; e0 += kThreads * kBatch) {
        float v[kBatch][kMaxTensors];
        bool ok[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int e = e0 + b * kThreads;
            ok[b] = false;
            if (e < words) {
                const int l = e / C, c = e - l * C;
                const int s = src_texel[l];
                ok[b] = s >= 0;
                const long long from = ok[b] ? (long long)s * C + c : 0;
#pragma unroll
                for (int k = 0; k < kMaxTensors; ++k)
                    if (k < a.n_tensors) v[b][k] = a.t[k].src[from];
            }
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            if (!ok[b]) continue;
#pragma unroll
            for (int k = 0; k < kMaxTensors; ++k)
                if (k < a.n_tensors) a.t[k].dst[base + e0 + b * kThreads] = v[b][k];
        }
    }
}

}  // namespace

extern "C" int gstex_select_plan(const gstex_select_plan_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_select_plan: null args");
    const gstex_select_plan_args& p = *args;
    GSTEX_REQUIRE(p.n >= 0, "gstex_select_plan: n < 0 (got %d)", p.n);
    GSTEX_REQUIRE(p.n_texels >= 0 && p.n_texels < (1ll << 31),
                  "gstex_select_plan: n_texels must be in [0, 2^31) (got %lld)", (long long)p.n_texels);
    GSTEX_REQUIRE(p.flag, "gstex_select_plan: null pointer (flag)");
    GSTEX_REQUIRE(aligned(p.flag, 4), "gstex_select_plan: misaligned pointer (flag; 4-byte words)");
    if (p.n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.keep && p.texture_dims && p.rows && p.texels,
                  "gstex_select_plan: null pointer (keep / texture_dims / rows / texels)");
    GSTEX_REQUIRE(aligned(p.texture_dims, 4) && aligned(p.rows, 4) && aligned(p.texels, 4),
                  "gstex_select_plan: misaligned pointer (texture_dims / rows / texels; 4-byte words)");
    select_plan_kernel<<<div_up(p.n, kThreads), kThreads, 0, as_stream(stream)>>>(
        p.n, (long long)p.n_texels, p.keep, p.texture_dims, p.rows, p.texels, p.flag);
    return launch_status("gstex_select_plan");
}

extern "C" int gstex_select_dims(const gstex_select_dims_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_select_dims: null args");
    const gstex_select_dims_args& p = *args;
    GSTEX_REQUIRE(p.n >= 0, "gstex_select_dims: n < 0 (got %d)", p.n);
    GSTEX_REQUIRE(p.n_new >= 0 && p.n_new <= p.n, "gstex_select_dims: n_new must be in [0, n] (n=%d, n_new=%d)", p.n,
                  p.n_new);
    if (p.n == 0 || p.n_new == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.keep && p.texture_dims && p.row_off && p.tex_off && p.new_dims && p.src_off,
                  "gstex_select_dims: null pointer (keep / texture_dims / row_off / tex_off / new_dims / src_off)");
    GSTEX_REQUIRE(aligned(p.texture_dims, 4) && aligned(p.row_off, 4) && aligned(p.tex_off, 4) &&
                      aligned(p.new_dims, 4) && aligned(p.src_off, 4),
                  "gstex_select_dims: misaligned pointer (4-byte words)");
    GSTEX_REQUIRE(p.new_dims != p.texture_dims, "gstex_select_dims: new_dims and texture_dims must differ");
    select_dims_kernel<<<div_up(p.n, kThreads), kThreads, 0, as_stream(stream)>>>(
        p.n, p.n_new, p.keep, p.texture_dims, p.row_off, p.tex_off, p.new_dims, p.src_off);
    return launch_status("gstex_select_dims");
}

extern "C" int gstex_select_texels(const gstex_select_texels_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_select_texels: null args");
    const gstex_select_texels_args& p = *args;
    GSTEX_REQUIRE(p.n_new >= 0, "gstex_select_texels: n_new < 0 (got %d)", p.n_new);
    GSTEX_REQUIRE(p.channels >= 1 && p.channels <= 8, "gstex_select_texels: channels must be in [1, 8] (got %d)",
                  p.channels);
    GSTEX_REQUIRE(p.n_tensors >= 0 && p.n_tensors <= kMaxTensors,
                  "gstex_select_texels: n_tensors must be in [0, %d] (got %d)", kMaxTensors, p.n_tensors);
    GSTEX_REQUIRE(p.n_texels >= 0 && p.n_texels < (1ll << 31) && p.n_texels_new >= 0 && p.n_texels_new < (1ll << 31),
                  "gstex_select_texels: n_texels and n_texels_new must be in [0, 2^31) (got %lld, %lld)",
                  (long long)p.n_texels, (long long)p.n_texels_new);
    if (p.n_tensors == 0 || p.n_texels_new == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.n_new > 0 && p.n_texels > 0,
                  "gstex_select_texels: n_texels_new > 0 needs n_new > 0 and n_texels > 0 (got %d, %lld)", p.n_new,
                  (long long)p.n_texels);
    GSTEX_REQUIRE(p.new_dims && p.src_off, "gstex_select_texels: null pointer (new_dims / src_off)");
    GSTEX_REQUIRE(aligned(p.new_dims, 4) && aligned(p.src_off, 4),
                  "gstex_select_texels: misaligned pointer (new_dims / src_off; 4-byte words)");
    TexelArgs a{};
    for (int i = 0; i < p.n_tensors; ++i) {
        const gstex_select_pair& t = p.tensors[i];
        GSTEX_REQUIRE(t.src && t.dst, "gstex_select_texels: tensor %d: null pointer (src / dst)", i);
        GSTEX_REQUIRE(aligned(t.src, 4) && aligned(t.dst, 4), "gstex_select_texels: tensor %d: misaligned pointer", i);
        GSTEX_REQUIRE(t.src != t.dst, "gstex_select_texels: tensor %d: src and dst must differ", i);
        a.t[i] = t;
    }
    a.n_tensors = p.n_tensors;
    a.n_new = p.n_new;
    a.channels = p.channels;
    a.T_new = p.n_texels_new;
    a.n_texels = p.n_texels;
    a.new_dims = p.new_dims;
    a.src_off = p.src_off;
    const unsigned blocks = (unsigned)((p.n_texels_new + kRun - 1) / kRun);
    if (p.channels == 3)
        select_texels_kernel<3><<<blocks, kThreads, 0, as_stream(stream)>>>(a);
    else
        select_texels_kernel<0><<<blocks, kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_select_texels");
}
