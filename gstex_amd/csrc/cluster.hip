// cluster.hip — DBSCAN over the splats under the squared 2-Wasserstein distance of their (flat) Gaussians (the
// reference's dbscan_clustering/dbscan_ballquery.py; DESIGN.md "Clustering the splats").
//
//   gstex_cluster_shapes   one thread per grid record: the 32-byte shape record (a.xyz, T, b.xyz, 0) in record order
//   gstex_cluster_degree   one thread per record: the fixed-radius ring walk, degree[index], parent[index] = index
//   gstex_cluster_link     the same walk: a core unites with every core neighbour of lower index (lock-free union-find)
//   gstex_cluster_roots    one thread per splat: parent[i] = find(i), flag[i] = core and root
//   gstex_cluster_assign   cores: offsets[parent] + 1; other splats with neighbours: the walk once more, the lowest id
//                          among the core neighbours; the rest -1
//   gstex_cluster_pair_w2  one thread per caller-given pair: d2, tr and w2
//
// The grid is neighbors.hip's (gstex_nn_grid_count / _place on the means); between roots and assign the caller scans
// the flags with gstex_scan_offsets.  Every value is one individually rounded fp32 operation in a fixed order
// (-ffp-contract=off, correctly rounded sqrtf), so gstex_amd.cluster's eager twins reproduce d2, tr, w2 bit for bit and
// the labels exactly.  The ring walk is nn_grid.h's walk_rings, the one gstex_nn_query runs: that kernel carries a
// sorted top-k through the rings and stops on its k-th best, these visit every record within the fixed radius eps.
#include "nn_grid.h"

using namespace gstex;

namespace {

constexpr int kThreads = 256;

struct ClusterK {
    GridK g;
    int n, min_pts;
    float eps;
    const int32_t* cell_start;
    const float4* records;
    const float4* shapes;  // two per record
    int32_t *degree, *parent;
    const int32_t* offsets;
    int32_t* labels;
};

// ---------------------------------------------------------------------------------------------- the distance
struct Shape { float ax, ay, az, T, bx, by, bz; };

// Unit quaternion (w, x, y, z) and the two in-plane scales -> the scaled tangent axes a = s0 R[:, 0], b = s1 R[:, 1]
// and T = s0^2 + s1^2 (DESIGN.md states every operation)
__device__ __forceinline__ Shape make_shape(float s0, float s1, float w, float x, float y, float z) {
    const float r00 = 1.0f - 2.0f * (y * y + z * z);
    const float r10 = 2.0f * (x * y + w * z);
    const float r20 = 2.0f * (x * z - w * y);
    const float r01 = 2.0f * (x * y - w * z);
    const float r11 = 1.0f - 2.0f * (x * x + z * z);
    const float r21 = 2.0f * (y * z + w * x);
    Shape s;
    s.ax = s0 * r00; s.ay = s0 * r10; s.az = s0 * r20;
    s.bx = s1 * r01; s.by = s1 * r11; s.bz = s1 * r21;
    s.T = s0 * s0 + s1 * s1;
    return s;
}

__device__ __forceinline__ Shape load_shape(const float4* shapes, int slot) {
    const float4 u = shapes[2 * (size_t)slot], v = shapes[2 * (size_t)slot + 1];
    return Shape{u.x, u.y, u.z, u.w, v.x, v.y, v.z};
}

// tr = max((T_i + T_j) - 2 sqrt(|B|_F^2 + 2 |det B|), 0) with B = [[a_i.a_j, a_i.b_j], [b_i.a_j, b_i.b_j]]; the order of
// the sums makes the value the same for (i, j) and (j, i), bit for bit
__device__ __forceinline__ float trace_term(const Shape& p, const Shape& q) {
    const float m00 = (p.ax * q.ax + p.ay * q.ay) + p.az * q.az;
    const float m01 = (p.ax * q.bx + p.ay * q.by) + p.az * q.bz;
    const float m10 = (p.bx * q.ax + p.by * q.ay) + p.bz * q.az;
    const float m11 = (p.bx * q.bx + p.by * q.by) + p.bz * q.bz;
    const float fro = (m00 * m00 + m11 * m11) + (m01 * m01 + m10 * m10);
    const float det = m00 * m11 - m01 * m10;
    const float root = sqrtf(fro + 2.0f * fabsf(det));
    return fmaxf((p.T + q.T) - 2.0f * root, 0.0f);
}

__device__ __forceinline__ float dist2(float qx, float qy, float qz, float px, float py, float pz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---------------------------------------------------------------------------------------------- the walk
// Every record within the fixed radius of the record q: on_neighbor(index) for each other splat with w2 <= eps.
// walk_rings stops on eps itself: what it has not visited is farther than that in d2, and w2 >= d2.
template <class F>
__device__ __forceinline__ void for_each_neighbor(const ClusterK& a, const float4& q, int self, const Shape& mine,
                                                  F&& on_neighbor) {
    auto scan = [&](int p, int pe) {
        p = max(p, 0); pe = min(pe, a.n);  // never outside the records
        for (; p < pe; ++p) {
            const float4 rec = a.records[p];
            const int idx = __float_as_int(rec.w);
            const float d2 = dist2(q.x, q.y, q.z, rec.x, rec.y, rec.z);
            if (idx == self || idx < 0 || idx >= a.n || !(d2 <= a.eps)) continue;
            const float w2 = d2 + trace_term(mine, load_shape(a.shapes, p));
            if (w2 <= a.eps) on_neighbor(idx);
        }
    };
    walk_rings(a.g, a.cell_start, q.x, q.y, q.z, scan, [&] { return a.eps; });
}

// the record of thread t, refused unless its index is one of this set's
__device__ __forceinline__ bool load_self(const ClusterK& a, int t, float4& q, int& self) {
    if (t >= a.n) return false;
    q = a.records[t];
    self = __float_as_int(q.w);
    return self >= 0 && self < a.n;
}

// ---------------------------------------------------------------------------------------------- union-find
// parent[x] <= x always, every store lowers an entry (atomicMin, or the CAS of a root x to a lower root) and every
// value ever stored in parent[x] is an ancestor of x: no cycle can form, and each step of find moves to a strictly
// lower index, so it ends within n steps whatever the other lanes do.  No lane waits for another.
__device__ __forceinline__ int load_parent(const int32_t* parent, int x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_root(int32_t* parent, int x) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p >= x || p < 0) return x;  // a root (p == x); anything else is no entry of this array's and ends the walk
        const int gp = load_parent(parent, p);
        if (gp < p && gp >= 0) atomicMin(&parent[x], gp);  // path halving
        x = (gp < p && gp >= 0) ? gp : p;
    }
}

__device__ __forceinline__ void unite(int32_t* parent, int u, int v) {
    for (;;) {
        u = find_root(parent, u);
        v = find_root(parent, v);
        if (u == v) return;
        const int hi = max(u, v), lo = min(u, v);
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old >= hi || old < 0) return;  // hooked (old == hi)
        // hi was hooked under `old` < hi by another lane meanwhile: go on from what the compare-and-swap itself
        // returned, so progress does not rest on a later load seeing that hook.  max(u, v) is now below hi, and find
        // only lowers it: the retries end within n rounds
        u = old;
        v = lo;
    }
}

// ---------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(kThreads) void shapes_kernel(int n, const float4* __restrict__ records,
                                                          const float* __restrict__ scales, int scale_cols,
                                                          const float* __restrict__ quats, float4* __restrict__ shapes) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    const int i = __float_as_int(records[t].w);
    Shape s{};
    if (i >= 0 && i < n) {
        const float* sc = scales + (size_t)scale_cols * i;
        const float* q = quats + (size_t)4 * i;
        s = make_shape(sc[0], sc[1], q[0], q[1], q[2], q[3]);
    }
    shapes[2 * (size_t)t] = make_float4(s.ax, s.ay, s.az, s.T);
    shapes[2 * (size_t)t + 1] = make_float4(s.bx, s.by, s.bz, 0.0f);
}

__global__ __launch_bounds__(kThreads) void degree_kernel(const ClusterK a) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    float4 q;
    int self;
    if (!load_self(a, t, q, self)) return;
    int count = 0;
    for_each_neighbor(a, q, self, load_shape(a.shapes, t), [&](int) { ++count; });
    a.degree[self] = count;
    a.parent[self] = self;
}

__global__ __launch_bounds__(kThreads) void link_kernel(const ClusterK a) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    float4 q;
    int self;
    if (!load_self(a, t, q, self)) return;
    if (a.degree[self] < a.min_pts) return;
    for_each_neighbor(a, q, self, load_shape(a.shapes, t), [&](int j) {
        if (j < self && a.degree[j] >= a.min_pts) unite(a.parent, self, j);
    });
}

__global__ __launch_bounds__(kThreads) void roots_kernel(int n, int min_pts, const int32_t* __restrict__ degree,
                                                         int32_t* parent, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int r = find_root(parent, i);  // no hook runs in this launch: the roots are fixed
    if (r < i) atomicMin(&parent[i], r);
    flag[i] = (degree[i] >= min_pts && r == i) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void assign_kernel(const ClusterK a) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    float4 q;
    int self;
    if (!load_self(a, t, q, self)) return;
    const int deg = a.degree[self];
    int label = -1;
    auto id_of = [&](int i) {  // the flattened parent of a core is its component's lowest core index
        const int r = a.parent[i];
        return (r >= 0 && r < a.n) ? a.offsets[r] + 1 : -1;
    };
    if (deg >= a.min_pts) {
        label = id_of(self);
    } else if (deg > 0) {
        int best = INT32_MAX;
        for_each_neighbor(a, q, self, load_shape(a.shapes, t), [&](int j) {
            if (a.degree[j] >= a.min_pts) {
                const int id = id_of(j);
                if (id >= 1) best = min(best, id);
            }
        });
        if (best != INT32_MAX) label = best;
    }
    a.labels[self] = label;
}

__global__ __launch_bounds__(kThreads) void pair_w2_kernel(int n, const float* __restrict__ means,
                                                           const float* __restrict__ scales, int scale_cols,
                                                           const float* __restrict__ quats, int n_pairs,
                                                           const int32_t* __restrict__ pairs, float* __restrict__ d2,
                                                           float* __restrict__ tr, float* __restrict__ w2) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_pairs) return;
    const int i = pairs[2 * (size_t)t], j = pairs[2 * (size_t)t + 1];
    float d = NAN, c = NAN;  // a pair outside [0, n) has no distance
    if (i >= 0 && i < n && j >= 0 && j < n) {
        const float *mi = means + (size_t)3 * i, *mj = means + (size_t)3 * j;
        const float *si = scales + (size_t)scale_cols * i, *sj = scales + (size_t)scale_cols * j;
        const float *qi = quats + (size_t)4 * i, *qj = quats + (size_t)4 * j;
        d = dist2(mi[0], mi[1], mi[2], mj[0], mj[1], mj[2]);
        c = trace_term(make_shape(si[0], si[1], qi[0], qi[1], qi[2], qi[3]),
                       make_shape(sj[0], sj[1], qj[0], qj[1], qj[2], qj[3]));
    }
    d2[t] = d;
    tr[t] = c;
    w2[t] = d + c;
}

// ---------------------------------------------------------------------------------------------- argument checks
int check_splats(const char* who, int64_t n, const float* scales, int32_t scale_cols, const float* quats) {
    GSTEX_REQUIRE(n >= 0 && n < (1ll << 31), "%s: n must be in [0, 2^31) (got %lld)", who, (long long)n);
    GSTEX_REQUIRE(scale_cols >= 2, "%s: scale_cols must be >= 2 (got %d)", who, scale_cols);
    GSTEX_REQUIRE(n == 0 || (scales && quats), "%s: null pointer (scales / quats)", who);
    GSTEX_REQUIRE(aligned(scales, 4) && aligned(quats, 4), "%s: misaligned pointer (4-byte words)", who);
    return GSTEX_OK;
}

// the fields every walk reads; -1: n == 0, nothing to launch
int fill_cluster(const char* who, const gstex_cluster_args* args, ClusterK& a) {
    GSTEX_REQUIRE(args, "%s: null args", who);
    const gstex_cluster_args& p = *args;
    const int rc = check_grid(who, &p.grid, a.g);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(p.n >= 0 && p.n < (1ll << 31), "%s: n must be in [0, 2^31) (got %lld)", who, (long long)p.n);
    GSTEX_REQUIRE(finite_f(p.eps) && p.eps >= 0.0f, "%s: eps must be finite and >= 0 (got %g)", who, (double)p.eps);
    GSTEX_REQUIRE(p.min_pts >= 1, "%s: min_pts must be >= 1 (got %d)", who, p.min_pts);
    if (p.n == 0) return -1;
    GSTEX_REQUIRE(p.cell_start && p.records && p.shapes && p.degree && p.parent,
                  "%s: null pointer (cell_start / records / shapes / degree / parent)", who);
    GSTEX_REQUIRE(aligned(p.cell_start, 4) && aligned(p.degree, 4) && aligned(p.parent, 4) && aligned(p.records, 16) &&
                      aligned(p.shapes, 16),
                  "%s: misaligned pointer (4-byte words, 16-byte records and shapes)", who);
    a.n = (int)p.n; a.min_pts = p.min_pts; a.eps = p.eps;
    a.cell_start = p.cell_start;
    a.records = reinterpret_cast<const float4*>(p.records);
    a.shapes = reinterpret_cast<const float4*>(p.shapes);
    a.degree = p.degree; a.parent = p.parent; a.offsets = p.offsets; a.labels = p.labels;
    return GSTEX_OK;
}

}  // namespace

extern "C" int gstex_cluster_shapes(int64_t n, const float* records, const float* scales, int32_t scale_cols,
                                    const float* quats, float* shapes, void* stream) {
    const int rc = check_splats("gstex_cluster_shapes", n, scales, scale_cols, quats);
    if (rc != GSTEX_OK) return rc;
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(records && shapes, "gstex_cluster_shapes: null pointer (records / shapes)");
    GSTEX_REQUIRE(aligned(records, 16) && aligned(shapes, 16),
                  "gstex_cluster_shapes: misaligned pointer (16-byte records and shapes)");
    shapes_kernel<<<div_up(n, kThreads), kThreads, 0, as_stream(stream)>>>(
        (int)n, reinterpret_cast<const float4*>(records), scales, scale_cols, quats, reinterpret_cast<float4*>(shapes));
    return launch_status("gstex_cluster_shapes");
}

extern "C" int gstex_cluster_degree(const gstex_cluster_args* args, void* stream) {
    ClusterK a{};
    const int rc = fill_cluster("gstex_cluster_degree", args, a);
    if (rc != GSTEX_OK) return rc < 0 ? GSTEX_OK : rc;
    degree_kernel<<<div_up(a.n, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_cluster_degree");
}

extern "C" int gstex_cluster_link(const gstex_cluster_args* args, void* stream) {
    ClusterK a{};
    const int rc = fill_cluster("gstex_cluster_link", args, a);
    if (rc != GSTEX_OK) return rc < 0 ? GSTEX_OK : rc;
    link_kernel<<<div_up(a.n, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_cluster_link");
}

extern "C" int gstex_cluster_roots(int64_t n, int32_t min_pts, const int32_t* degree, int32_t* parent,
                                   int32_t* root_flag, void* stream) {
    GSTEX_REQUIRE(n >= 0 && n < (1ll << 31), "gstex_cluster_roots: n must be in [0, 2^31) (got %lld)", (long long)n);
    GSTEX_REQUIRE(min_pts >= 1, "gstex_cluster_roots: min_pts must be >= 1 (got %d)", min_pts);
    if (n == 0) return GSTEX_OK;
    GSTEX_REQUIRE(degree && parent && root_flag, "gstex_cluster_roots: null pointer (degree / parent / root_flag)");
    GSTEX_REQUIRE(aligned(degree, 4) && aligned(parent, 4) && aligned(root_flag, 4),
                  "gstex_cluster_roots: misaligned pointer (4-byte words)");
    roots_kernel<<<div_up(n, kThreads), kThreads, 0, as_stream(stream)>>>((int)n, min_pts, degree, parent, root_flag);
    return launch_status("gstex_cluster_roots");
}

extern "C" int gstex_cluster_assign(const gstex_cluster_args* args, void* stream) {
    ClusterK a{};
    const int rc = fill_cluster("gstex_cluster_assign", args, a);
    if (rc != GSTEX_OK) return rc < 0 ? GSTEX_OK : rc;
    GSTEX_REQUIRE(a.offsets && a.labels, "gstex_cluster_assign: null pointer (offsets / labels)");
    GSTEX_REQUIRE(aligned(a.offsets, 4) && aligned(a.labels, 4), "gstex_cluster_assign: misaligned pointer (4-byte words)");
    assign_kernel<<<div_up(a.n, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_cluster_assign");
}

extern "C" int gstex_cluster_pair_w2(int64_t n, const float* means, const float* scales, int32_t scale_cols,
                                     const float* quats, int64_t n_pairs, const int32_t* pairs, float* d2, float* tr,
                                     float* w2, void* stream) {
    const int rc = check_splats("gstex_cluster_pair_w2", n, scales, scale_cols, quats);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 30), "gstex_cluster_pair_w2: n_pairs must be in [0, 2^30) (got %lld)",
                  (long long)n_pairs);
    if (n_pairs == 0) return GSTEX_OK;
    GSTEX_REQUIRE((n == 0 || means) && pairs && d2 && tr && w2,
                  "gstex_cluster_pair_w2: null pointer (means / pairs / d2 / tr / w2)");
    GSTEX_REQUIRE(aligned(means, 4) && aligned(pairs, 4) && aligned(d2, 4) && aligned(tr, 4) && aligned(w2, 4),
                  "gstex_cluster_pair_w2: misaligned pointer (4-byte words)");
    pair_w2_kernel<<<div_up(n_pairs, kThreads), kThreads, 0, as_stream(stream)>>>(
        (int)n, means, scales, scale_cols, quats, (int)n_pairs, pairs, d2, tr, w2);
    return launch_status("gstex_cluster_pair_w2");
}
