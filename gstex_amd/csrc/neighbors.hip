// neighbors.hip — mesh scoring: a uniform-grid nearest-neighbour index over a 3D point set and a deterministic area
// sampler of a triangle mesh (not in the reference; DESIGN.md "Mesh scoring and nearest neighbours").
//
//   gstex_nn_grid_count     one thread per point: its cell's count, by integer atomics
//   gstex_nn_grid_place     one thread per point: one 16-byte record (x, y, z, index) into its cell's segment
//   gstex_nn_query          one thread per query: nn_grid.h's ring walk around the query's cell, a sorted top-k in
//                           registers (k compile-time), exact
//   gstex_mesh_sample_mark  one thread per face: n^2 and the totals
//   gstex_mesh_sample_emit  one thread per sample: its face by bisection of the offsets, then (i, j, upright / inverted)
//
// Between count and place, and between mark and emit, the caller runs gstex_scan_offsets.  Every value is one
// individually rounded fp32 operation in a fixed order (-ffp-contract=off; sqrtf and / are the correctly rounded ones),
// so gstex_amd.neighbors' eager twins reproduce every ordered output bit for bit.
#include "nn_grid.h"

using namespace gstex;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = GSTEX_NN_MAX_K;

// (int)((p - o) / h) clamped to [0, n - 1]; p >= o for the points the grid was sized for
__device__ __forceinline__ int point_cell_axis(float p, float o, float h, int n) {
    const float t = (p - o) / h;
    const float tc = fminf(fmaxf(t, 0.0f), (float)(n - 1));  // (NaN -> 0)
    return (int)tc;
}

__device__ __forceinline__ int point_cell(const GridK& g, float x, float y, float z) {
    const int cx = point_cell_axis(x, g.ox, g.h, g.nx);
    const int cy = point_cell_axis(y, g.oy, g.h, g.ny);
    const int cz = point_cell_axis(z, g.oz, g.h, g.nz);
    return (cz * g.ny + cy) * g.nx + cx;
}

__global__ __launch_bounds__(kThreads) void nn_count_kernel(const GridK g, int n, const float* __restrict__ points,
                                                            int32_t* __restrict__ cell_count) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t b = (size_t)3 * i;
    atomicAdd(&cell_count[point_cell(g, points[b], points[b + 1], points[b + 2])], 1);
}

__global__ __launch_bounds__(kThreads) void nn_place_kernel(const GridK g, int n, const float* __restrict__ points,
                                                            const int32_t* __restrict__ cell_start,
                                                            int32_t* __restrict__ cursor, float4* __restrict__ records) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t b = (size_t)3 * i;
    const float x = points[b], y = points[b + 1], z = points[b + 2];
    const int c = point_cell(g, x, y, z);
    const int slot = cell_start[c] + atomicAdd(&cursor[c], 1);
    if (slot < 0 || slot >= n) return;  // offsets that are not this point set's scan must not make the write leave
    records[slot] = make_float4(x, y, z, __int_as_float(i));
}

struct QueryK {
    GridK g;
    int n_points, n_queries, exclude_self;
    float r2max;
    const int32_t* cell_start;
    const float4* records;
    const float4* queries;
    float* d2;
    int32_t* index;
};

// The records [p, pe) against the query: the sorted top-k (d2 ascending, ties to the lower index) in registers.
template <int K>
__device__ __forceinline__ void scan_records(const QueryK& a, const float4& q, int self, int p, int pe, float (&bd)[K],
                                             int (&bi)[K]) {
    p = max(p, 0); pe = min(pe, a.n_points);  // never outside the records
    for (; p < pe; ++p) {
        const float4 rec = a.records[p];
        const int idx = __float_as_int(rec.w);
        const float dx = q.x - rec.x, dy = q.y - rec.y, dz = q.z - rec.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (idx == self || !(d <= a.r2max)) continue;
        if (!(d < bd[K - 1] || (d == bd[K - 1] && idx < bi[K - 1]))) continue;
        float cd = d;
        int ci = idx;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const bool before = cd < bd[s] || (cd == bd[s] && ci < bi[s]);
            const float td = bd[s];
            const int ti = bi[s];
            bd[s] = before ? cd : td;
            bi[s] = before ? ci : ti;
            cd = before ? td : cd;
            ci = before ? ti : ci;
        }
    }
}

// The ring walk of one query, the top-k carried through it.  A function of its own, the arrays its parameters, not a
// call in the kernel with the kernel's arrays captured: the lambdas' closures are then gone before this is inlined
// into the kernel, where the compiler turns bd and bi into vector registers only while nothing else holds their
// address (as captures would); without that the k = 3 launch is 5 % slower (EXPERIMENTS.md "Nearest neighbours").
template <int K>
__device__ __forceinline__ void walk_query(const QueryK& a, const float4& q, int self, float (&bd)[K], int (&bi)[K]) {
    walk_rings(a.g, a.cell_start, q.x, q.y, q.z, [&](int p, int pe) { scan_records<K>(a, q, self, p, pe, bd, bi); },
               [&] { return fminf(bd[K - 1], a.r2max); });
}

template <int K>
__global__ __launch_bounds__(kThreads) void nn_query_kernel(const QueryK a) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= a.n_queries) return;
    const float4 q = a.queries[t];
    const int row = __float_as_int(q.w);
    if (row < 0 || row >= a.n_queries) return;  // a record that is not one of this query set's rows
    const int self = a.exclude_self ? row : -1;
    float bd[K];
    int bi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = -1; }
    walk_query<K>(a, q, self, bd, bi);
    const size_t o = (size_t)row * K;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        a.d2[o + s] = bd[s];
        a.index[o + s] = bi[s];
    }
}

// ------------------------------------------------------------------------------------------ mesh sampler
struct SampleK {
    int n_vertices, n_faces;
    const float* vertices;
    const int32_t* faces;
    float spacing;
    int32_t *count, *stats;
    const int32_t* offsets;
    long long n_samples;
    float *samples, *weights;
    int32_t* face_of;
};

__device__ __forceinline__ bool load_face(const SampleK& a, int f, float pa[3], float pb[3], float pc[3]) {
    const int ia = a.faces[3 * (size_t)f], ib = a.faces[3 * (size_t)f + 1], ic = a.faces[3 * (size_t)f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= a.n_vertices || ib >= a.n_vertices || ic >= a.n_vertices) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pa[c] = a.vertices[3 * (size_t)ia + c];
        pb[c] = a.vertices[3 * (size_t)ib + c];
        pc[c] = a.vertices[3 * (size_t)ic + c];
    }
    return true;
}

__device__ __forceinline__ float len2(const float e[3]) { return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]; }

__global__ __launch_bounds__(kThreads) void sample_mark_kernel(const SampleK a) {
    __shared__ unsigned long long s_sum;
    __shared__ int s_max, s_bad;
    if (threadIdx.x == 0) { s_sum = 0; s_max = 0; s_bad = 0; }
    __syncthreads();
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f < a.n_faces) {
        float pa[3], pb[3], pc[3];
        int count = 0;
        if (!load_face(a, f, pa, pb, pc)) {
            atomicAdd(&s_bad, 1);
        } else {
            float e1[3], e2[3], e3[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { e1[c] = pb[c] - pa[c]; e2[c] = pc[c] - pa[c]; e3[c] = pc[c] - pb[c]; }
            const float L = sqrtf(fmaxf(fmaxf(len2(e1), len2(e2)), len2(e3)));
            const float q = ceilf(L / a.spacing);
            const int n = q < 1073741824.0f ? max((int)q, 1) : 1073741824;  // (inf and NaN -> 2^30: refused)
            atomicMax(&s_max, n);
            if (n <= GSTEX_SAMPLE_MAX_N) {
                count = n * n;
                atomicAdd(&s_sum, (unsigned long long)count);
            }
        }
        a.count[f] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sum) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats), s_sum);
        if (s_max) atomicMax(&a.stats[2], s_max);
        if (s_bad) atomicAdd(&a.stats[3], s_bad);
    }
}

__global__ __launch_bounds__(kThreads) void sample_emit_kernel(const SampleK a) {
    const long long s = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (s >= a.n_samples) return;
    // the face: the last f with offsets[f] <= s
    int lo = 0, hi = a.n_faces;  // offsets[lo] <= s < offsets[hi] once the total covers s
    if (!(a.offsets[hi] > s)) return;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.offsets[mid] <= s) lo = mid; else hi = mid;
    }
    const int f = lo;
    const int first = a.offsets[f], nn = a.offsets[f + 1] - first;
    const int t = (int)(s - first);
    if (t < 0 || nn < 1 || nn > GSTEX_SAMPLE_MAX_N * GSTEX_SAMPLE_MAX_N) return;
    int n = (int)sqrtf((float)nn);  // nn = n^2 <= 2^16: exact
    if (n * n != nn) return;
    float pa[3], pb[3], pc[3];
    if (!load_face(a, f, pa, pb, pc)) return;
    // row i holds 2 (n - i) - 1 samples and starts at i (2 n - i): i = n - ceil(sqrt(n^2 - t))
    const int rem = nn - t;
    int m = (int)sqrtf((float)rem);
    while (m * m < rem) ++m;
    while ((m - 1) * (m - 1) >= rem) --m;
    const int i = n - m;
    const int tt = t - i * (2 * n - i);
    const int j = tt >> 1;
    const float third = (tt & 1) ? (2.0f / 3.0f) : (1.0f / 3.0f);
    const float fn = (float)n;
    const float u = ((float)i + third) / fn, v = ((float)j + third) / fn;
    float e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { e1[c] = pb[c] - pa[c]; e2[c] = pc[c] - pa[c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.samples[3 * s + c] = (pa[c] + u * e1[c]) + v * e2[c];
    float cr[3];
    cr[0] = e1[1] * e2[2] - e1[2] * e2[1];
    cr[1] = e1[2] * e2[0] - e1[0] * e2[2];
    cr[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const float area = 0.5f * sqrtf(len2(cr));
    a.weights[s] = area / (fn * fn);
    a.face_of[s] = f;
}

template <int K>
void launch_query(const QueryK& a, hipStream_t st) {
    nn_query_kernel<K><<<div_up(a.n_queries, kThreads), kThreads, 0, st>>>(a);
}

int fill_sample(const char* who, const gstex_mesh_sample_args* args, SampleK& a) {
    GSTEX_REQUIRE(args, "%s: null args", who);
    const gstex_mesh_sample_args& p = *args;
    GSTEX_REQUIRE(p.n_vertices >= 0 && p.n_faces >= 0 && p.n_vertices < (1ll << 31) && 3 * p.n_faces < (1ll << 31),
                  "%s: invalid sizes (n_vertices=%lld, n_faces=%lld)", who, (long long)p.n_vertices,
                  (long long)p.n_faces);
    GSTEX_REQUIRE(finite_f(p.spacing) && p.spacing > 0.0f, "%s: spacing must be finite and > 0 (got %g)", who,
                  (double)p.spacing);
    GSTEX_REQUIRE(p.n_faces == 0 || (p.vertices && p.faces), "%s: null pointer (vertices / faces)", who);
    GSTEX_REQUIRE(aligned(p.vertices, 4) && aligned(p.faces, 4), "%s: misaligned pointer (4-byte words)", who);
    a.n_vertices = (int)p.n_vertices; a.n_faces = (int)p.n_faces;
    a.vertices = p.vertices; a.faces = p.faces; a.spacing = p.spacing;
    a.count = p.count; a.stats = p.stats; a.offsets = p.offsets; a.n_samples = p.n_samples;
    a.samples = p.samples; a.weights = p.weights; a.face_of = p.face_of;
    return GSTEX_OK;
}

}  // namespace

extern "C" int gstex_nn_grid_count(const gstex_nn_grid* grid, int64_t n, const float* points, int32_t* cell_count,
                                   void* stream) {
    GridK g{};
    const int rc = check_grid("gstex_nn_grid_count", grid, g);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(n >= 0 && n < (1ll << 31), "gstex_nn_grid_count: n must be in [0, 2^31) (got %lld)", (long long)n);
    GSTEX_REQUIRE(cell_count && (n == 0 || points), "gstex_nn_grid_count: null pointer (points / cell_count)");
    GSTEX_REQUIRE(aligned(points, 4) && aligned(cell_count, 4), "gstex_nn_grid_count: misaligned pointer (4-byte words)");
    const hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(cell_count, 0, sizeof(int32_t) * (size_t)cells_of(g), st) != hipSuccess)
        return launch_status("gstex_nn_grid_count (zeroing the counts)");
    if (n == 0) return GSTEX_OK;
    nn_count_kernel<<<div_up(n, kThreads), kThreads, 0, st>>>(g, (int)n, points, cell_count);
    return launch_status("gstex_nn_grid_count");
}

extern "C" int gstex_nn_grid_place(const gstex_nn_grid* grid, int64_t n, const float* points,
                                   const int32_t* cell_start, int32_t* cursor, float* records, void* stream) {
    GridK g{};
    const int rc = check_grid("gstex_nn_grid_place", grid, g);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(n >= 0 && n < (1ll << 31), "gstex_nn_grid_place: n must be in [0, 2^31) (got %lld)", (long long)n);
    GSTEX_REQUIRE(cell_start && cursor && (n == 0 || (points && records)),
                  "gstex_nn_grid_place: null pointer (points / cell_start / cursor / records)");
    GSTEX_REQUIRE(aligned(points, 4) && aligned(cell_start, 4) && aligned(cursor, 4) && aligned(records, 16),
                  "gstex_nn_grid_place: misaligned pointer (4-byte words, 16-byte records)");
    const hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)cells_of(g), st) != hipSuccess)
        return launch_status("gstex_nn_grid_place (zeroing the cursors)");
    if (n == 0) return GSTEX_OK;
    nn_place_kernel<<<div_up(n, kThreads), kThreads, 0, st>>>(g, (int)n, points, cell_start, cursor,
                                                              reinterpret_cast<float4*>(records));
    return launch_status("gstex_nn_grid_place");
}

extern "C" int gstex_nn_query(const gstex_nn_query_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_nn_query: null args");
    const gstex_nn_query_args& p = *args;
    QueryK a{};
    const int rc = check_grid("gstex_nn_query", &p.grid, a.g);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(p.k >= 1 && p.k <= kMaxK, "gstex_nn_query: k must be in [1, %d] (got %d)", kMaxK, p.k);
    GSTEX_REQUIRE(p.n_points >= 0 && p.n_points < (1ll << 31) && p.n_queries >= 0 && p.n_queries < (1ll << 31),
                  "gstex_nn_query: point counts must be in [0, 2^31) (n_points=%lld, n_queries=%lld)",
                  (long long)p.n_points, (long long)p.n_queries);
    GSTEX_REQUIRE(p.max_radius >= 0.0f, "gstex_nn_query: max_radius must be >= 0, +inf for none (got %g)",
                  (double)p.max_radius);
    if (p.n_queries == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.cell_start && p.queries && p.d2 && p.index && (p.n_points == 0 || p.records),
                  "gstex_nn_query: null pointer (cell_start / records / queries / d2 / index)");
    GSTEX_REQUIRE(aligned(p.cell_start, 4) && aligned(p.d2, 4) && aligned(p.index, 4) && aligned(p.records, 16) &&
                      aligned(p.queries, 16),
                  "gstex_nn_query: misaligned pointer (4-byte words, 16-byte records)");
    a.n_points = (int)p.n_points; a.n_queries = (int)p.n_queries; a.exclude_self = p.exclude_self != 0;
    a.r2max = p.max_radius * p.max_radius;
    a.cell_start = p.cell_start;
    a.records = reinterpret_cast<const float4*>(p.records);
    a.queries = reinterpret_cast<const float4*>(p.queries);
    a.d2 = p.d2; a.index = p.index;
    const hipStream_t st = as_stream(stream);
    switch (p.k) {
        case 1: launch_query<1>(a, st); break;
        case 2: launch_query<2>(a, st); break;
        case 3: launch_query<3>(a, st); break;
        case 4: launch_query<4>(a, st); break;
        case 5: launch_query<5>(a, st); break;
        case 6: launch_query<6>(a, st); break;
        case 7: launch_query<7>(a, st); break;
        default: launch_query<8>(a, st); break;
    }
    return launch_status("gstex_nn_query");
}

extern "C" int gstex_mesh_sample_mark(const gstex_mesh_sample_args* args, void* stream) {
    SampleK a{};
    const int rc = fill_sample("gstex_mesh_sample_mark", args, a);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(a.stats && (a.n_faces == 0 || a.count), "gstex_mesh_sample_mark: null pointer (count / stats)");
    GSTEX_REQUIRE(aligned(a.count, 4) && aligned(a.stats, 8),
                  "gstex_mesh_sample_mark: misaligned pointer (4-byte words, 8-byte stats)");
    const hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(a.stats, 0, 4 * sizeof(int32_t), st) != hipSuccess)
        return launch_status("gstex_mesh_sample_mark (zeroing the stats)");
    if (a.n_faces == 0) return GSTEX_OK;
    sample_mark_kernel<<<div_up(a.n_faces, kThreads), kThreads, 0, st>>>(a);
    return launch_status("gstex_mesh_sample_mark");
}

extern "C" int gstex_mesh_sample_emit(const gstex_mesh_sample_args* args, void* stream) {
    SampleK a{};
    const int rc = fill_sample("gstex_mesh_sample_emit", args, a);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(a.n_samples >= 0 && a.n_samples < (1ll << 31),
                  "gstex_mesh_sample_emit: n_samples must be in [0, 2^31) (got %lld)", a.n_samples);
    if (a.n_samples == 0 || a.n_faces == 0) return GSTEX_OK;
    GSTEX_REQUIRE(a.offsets && a.samples && a.weights && a.face_of,
                  "gstex_mesh_sample_emit: null pointer (offsets / samples / weights / face_of)");
    GSTEX_REQUIRE(aligned(a.offsets, 4) && aligned(a.samples, 4) && aligned(a.weights, 4) && aligned(a.face_of, 4),
                  "gstex_mesh_sample_emit: misaligned pointer (4-byte words)");
    sample_emit_kernel<<<div_up(a.n_samples, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_mesh_sample_emit");
}
