// tsdf.hip — mesh extraction: TSDF fusion of rendered depth maps and marching tetrahedra on the volume (not in the
// reference, whose lineage leaves both to Open3D; DESIGN.md "Mesh extraction").
//
//   gstex_tsdf_integrate     one thread per voxel, up to 8 views per launch: the voxel stays in registers across them
//   gstex_mesh_extract_mark  one thread per cell: which edges carry a vertex (a 7-bit mask per owning voxel) and how
//                            many faces the cell emits; then one thread per voxel: the mask's population count
//   gstex_mesh_extract_emit  one thread per voxel: the vertices it owns and the faces of its cell
//
// Between mark and emit the caller runs gstex_scan_offsets over the two counts and reads the two totals back (the
// extraction's only synchronisation).  Every value is one individually rounded fp32 + - * / in a fixed order
// (-ffp-contract=off), so gstex_amd.mesh's eager twins reproduce all three entry points bit for bit.  The case table
// comes from the caller (gstex_amd.mesh derives it by geometry); the twin reads the same words.
#include "gstex_common.h"
#include "gstex_error.h"

using namespace gstex;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxViews = GSTEX_TSDF_MAX_VIEWS;
static_assert(GSTEX_MESH_TABLE_WORDS == 6 * 16 + 6, "16 case words and one corner word per tetrahedron");

struct Grid {
    int nx, ny, nz, n_vox;
    float ox, oy, oz, h;
};

struct ViewK {
    const float *viewmat, *depth, *alpha, *rgb;
    float fx, fy, cx, cy, fw, fh;  // fw, fh: (float)W, (float)H
    int W;
};

struct IntegrateArgs {
    Grid g;
    float *tsdf, *weight, *color;
    int n_views;
    float sdf_trunc, alpha_min, depth_trunc, near_z;
    ViewK v[kMaxViews];
};

__device__ __forceinline__ void voxel_index(const Grid& g, int v, int& i, int& j, int& k) {
    const int row = v / g.nx;
    i = v - row * g.nx;
    k = row / g.ny;
    j = row - k * g.ny;
}

__global__ __launch_bounds__(kThreads) void tsdf_integrate_kernel(const IntegrateArgs a) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= a.g.n_vox) return;
    int i, j, k;
    voxel_index(a.g, v, i, j, k);
    const float px = a.g.ox + a.g.h * (float)i;
    const float py = a.g.oy + a.g.h * (float)j;
    const float pz = a.g.oz + a.g.h * (float)k;
    const bool has_color = a.color != nullptr;
    const size_t plane = (size_t)a.g.n_vox;
    float tsdf = a.tsdf[v], w = a.weight[v];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (has_color) {
        c0 = a.color[v]; c1 = a.color[plane + v]; c2 = a.color[2 * plane + v];
    }
    bool changed = false;
#pragma unroll 1
    for (int q = 0; q < a.n_views; ++q) {
        const ViewK& vw = a.v[q];
        const float* V = vw.viewmat;  // row-major (3, 4), wave-uniform loads
        const float z = ((V[8] * px + V[9] * py) + V[10] * pz) + V[11];
        if (!(z > a.near_z)) continue;
        const float x = ((V[0] * px + V[1] * py) + V[2] * pz) + V[3];
        const float y = ((V[4] * px + V[5] * py) + V[6] * pz) + V[7];
        const float pu = vw.fx * (x / z) + vw.cx;
        const float pv = vw.fy * (y / z) + vw.cy;
        if (!(pu >= 0.0f && pu < vw.fw && pv >= 0.0f && pv < vw.fh)) continue;
        const int c = (int)pu, r = (int)pv;  // pixel (r, c) covers [c, c + 1) x [r, r + 1)
        const size_t pix = (size_t)r * vw.W + c;
        const float al = vw.alpha[pix];
        if (!(al >= a.alpha_min)) continue;
        const float d = vw.depth[pix] / al;
        if (!(d > 0.0f) || (a.depth_trunc > 0.0f && d > a.depth_trunc)) continue;
        const float s = d - z;
        if (s < -a.sdf_trunc) continue;
        const float t = fminf(1.0f, s / a.sdf_trunc);
        const float w1 = w + 1.0f;
        tsdf = (tsdf * w + t) / w1;
        if (has_color) {
            c0 = (c0 * w + vw.rgb[3 * pix]) / w1;
            c1 = (c1 * w + vw.rgb[3 * pix + 1]) / w1;
            c2 = (c2 * w + vw.rgb[3 * pix + 2]) / w1;
        }
        w = w1;
        changed = true;
    }
    if (!changed) return;
    a.tsdf[v] = tsdf;
    a.weight[v] = w;
    if (has_color) {
        a.color[v] = c0; a.color[plane + v] = c1; a.color[2 * plane + v] = c2;
    }
}

// ------------------------------------------------------------------------------------------ marching tetrahedra
struct ExtractArgs {
    Grid g;
    const float *tsdf, *weight, *color;
    const int32_t* table;
    int32_t *edge_mask, *vertex_count, *face_count;
    const int32_t *vertex_offsets, *face_offsets;
    long long n_vertices, n_faces;
    float *vertices, *colors;
    int32_t* faces;
};

// class of an edge from its difference dx | dy << 1 | dz << 2, in the header's order
__device__ __forceinline__ int edge_class(int diff) {
    constexpr int kClass[8] = {0, 0, 1, 3, 2, 5, 4, 6};
    return kClass[diff & 7];
}
// the difference of a class
__device__ __forceinline__ int class_diff(int cls) {
    constexpr int kDiff[7] = {1, 2, 4, 3, 6, 5, 7};
    return kDiff[cls];
}

__device__ __forceinline__ int corner_voxel(const Grid& g, int v, int bits) {
    return v + (bits & 1) + ((bits >> 1) & 1) * g.nx + ((bits >> 2) & 1) * g.nx * g.ny;
}

// The cell's eight corners as two bytes indexed by dx | dy << 1 | dz << 2: inside (tsdf < 0) and seen (weight > 0).
__device__ __forceinline__ void cell_corners(const ExtractArgs& a, int v, int& inside, int& seen) {
    inside = 0; seen = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int p = corner_voxel(a.g, v, b);
        inside |= (a.tsdf[p] < 0.0f ? 1 : 0) << b;
        seen |= (a.weight[p] > 0.0f ? 1 : 0) << b;
    }
}

// The table word of tetrahedron `tet` of a cell (0 when the tetrahedron does not emit); corners: its corner word.
__device__ __forceinline__ int tet_word(const int32_t* table, int tet, int inside, int seen, int& corners) {
    corners = table[96 + tet];
    int cs = 0, ok = 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = (corners >> (3 * k)) & 7;
        cs |= ((inside >> b) & 1) << k;
        ok &= (seen >> b) & 1;
    }
    return ok ? table[tet * 16 + cs] : 0;
}

__device__ __forceinline__ bool is_cell(const Grid& g, int i, int j, int k) {
    return i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1;
}

__global__ __launch_bounds__(kThreads) void mesh_mark_kernel(const ExtractArgs a) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= a.g.n_vox) return;
    int i, j, k;
    voxel_index(a.g, v, i, j, k);
    int faces = 0;
    if (is_cell(a.g, i, j, k)) {
        int inside, seen;
        cell_corners(a, v, inside, seen);
        if (seen != 0 && inside != 0 && inside != 0xff) {
            for (int tet = 0; tet < 6; ++tet) {
                int corners;
                const int word = tet_word(a.table, tet, inside, seen, corners);
                const int ntri = (word >> 24) & 3;
                faces += ntri;
                for (int s = 0; s < 3 * ntri; ++s) {
                    const int lo = (word >> (4 * s)) & 3, hi = (word >> (4 * s + 2)) & 3;
                    const int blo = (corners >> (3 * lo)) & 7, bhi = (corners >> (3 * hi)) & 7;
                    // the same bit may be set from several cells: the OR makes the result independent of the order
                    atomicOr(&a.edge_mask[corner_voxel(a.g, v, blo)], 1 << edge_class(bhi - blo));
                }
            }
        }
    }
    a.face_count[v] = faces;
}

__global__ __launch_bounds__(kThreads) void mesh_count_kernel(int n_vox, const int32_t* __restrict__ edge_mask,
                                                              int32_t* __restrict__ vertex_count) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n_vox) return;
    vertex_count[v] = __popc((unsigned)edge_mask[v] & 0x7fu);
}

__global__ __launch_bounds__(kThreads) void mesh_emit_kernel(const ExtractArgs a) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= a.g.n_vox) return;
    int i, j, k;
    voxel_index(a.g, v, i, j, k);
    const int mask = a.edge_mask[v] & 0x7f;
    if (mask) {
        const long long row0 = a.vertex_offsets[v];
        const float pa[3] = {a.g.ox + a.g.h * (float)i, a.g.oy + a.g.h * (float)j, a.g.oz + a.g.h * (float)k};
        const float ta = a.tsdf[v];
        const size_t plane = (size_t)a.g.n_vox;
        int rank = 0;
        for (int cls = 0; cls < 7; ++cls) {
            if (!((mask >> cls) & 1)) continue;
            const long long row = row0 + rank;
            ++rank;
            if (row < 0 || row >= a.n_vertices) continue;  // never past the rows the caller allocated
            const int diff = class_diff(cls);
            const int idx[3] = {i + (diff & 1), j + ((diff >> 1) & 1), k + ((diff >> 2) & 1)};
            // an edge the mark pass set belongs to a cell, so both ends are inside the grid; a mask that did not come
            // from it must not make this read leave the volume
            if (idx[0] >= a.g.nx || idx[1] >= a.g.ny || idx[2] >= a.g.nz) continue;
            const int p = corner_voxel(a.g, v, diff);
            const float tb = a.tsdf[p];
            const float t = ta / (ta - tb);
            const float o[3] = {a.g.ox, a.g.oy, a.g.oz};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float pb = o[c] + a.g.h * (float)idx[c];
                a.vertices[3 * row + c] = pa[c] + t * (pb - pa[c]);
            }
            if (a.colors) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float ca = a.color[c * plane + v], cb = a.color[c * plane + p];
                    a.colors[3 * row + c] = ca + t * (cb - ca);
                }
            }
        }
    }
    if (!is_cell(a.g, i, j, k)) return;
    int inside, seen;
    cell_corners(a, v, inside, seen);
    if (seen == 0 || inside == 0 || inside == 0xff) return;
    long long face = a.face_offsets[v];
    for (int tet = 0; tet < 6; ++tet) {
        int corners;
        const int word = tet_word(a.table, tet, inside, seen, corners);
        const int ntri = (word >> 24) & 3;
        for (int tri = 0; tri < ntri; ++tri, ++face) {
            if (face < 0 || face >= a.n_faces) continue;  // never past the rows the caller allocated
            for (int e = 0; e < 3; ++e) {
                const int s = 3 * tri + e;
                const int lo = (word >> (4 * s)) & 3, hi = (word >> (4 * s + 2)) & 3;
                const int blo = (corners >> (3 * lo)) & 7, bhi = (corners >> (3 * hi)) & 7;
                const int owner = corner_voxel(a.g, v, blo);
                const int below = (a.edge_mask[owner] & 0x7f) & ((1 << edge_class(bhi - blo)) - 1);
                a.faces[3 * face + e] = a.vertex_offsets[owner] + __popc((unsigned)below);
            }
        }
    }
}

// The volume checks every entry point shares; fills g.
int check_volume(const char* who, const gstex_tsdf_volume& vol, Grid& g) {
    GSTEX_REQUIRE(vol.nx >= 2 && vol.ny >= 2 && vol.nz >= 2, "%s: every dim must be >= 2 (got nx=%d, ny=%d, nz=%d)",
                  who, vol.nx, vol.ny, vol.nz);
    const long long n_vox = (long long)vol.nx * vol.ny * vol.nz;
    if (7 * n_vox >= (1ll << 31)) {
        set_error("%s: 7 * n_vox must be below 2^31 (got %lld voxels)", who, n_vox);
        return GSTEX_ERR_UNSUPPORTED;
    }
    GSTEX_REQUIRE(finite_f(vol.origin[0]) && finite_f(vol.origin[1]) && finite_f(vol.origin[2]) &&
                      finite_f(vol.voxel_size) && vol.voxel_size > 0.0f,
                  "%s: the origin must be finite and voxel_size finite and > 0", who);
    GSTEX_REQUIRE(vol.tsdf && vol.weight, "%s: null volume (tsdf / weight)", who);
    GSTEX_REQUIRE(aligned(vol.tsdf, 4) && aligned(vol.weight, 4) && aligned(vol.color, 4),
                  "%s: misaligned pointer (4-byte words)", who);
    g.nx = vol.nx; g.ny = vol.ny; g.nz = vol.nz; g.n_vox = (int)n_vox;
    g.ox = vol.origin[0]; g.oy = vol.origin[1]; g.oz = vol.origin[2]; g.h = vol.voxel_size;
    return GSTEX_OK;
}

int fill_extract(const char* who, const gstex_mesh_extract_args& p, ExtractArgs& a) {
    const int rc = check_volume(who, p.vol, a.g);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(p.table && p.edge_mask && p.vertex_count && p.face_count,
                  "%s: null pointer (table / edge_mask / vertex_count / face_count)", who);
    GSTEX_REQUIRE(aligned(p.table, 4) && aligned(p.edge_mask, 4) && aligned(p.vertex_count, 4) &&
                      aligned(p.face_count, 4),
                  "%s: misaligned pointer (4-byte words)", who);
    a.tsdf = p.vol.tsdf; a.weight = p.vol.weight; a.color = p.vol.color;
    a.table = p.table; a.edge_mask = p.edge_mask; a.vertex_count = p.vertex_count; a.face_count = p.face_count;
    a.vertex_offsets = p.vertex_offsets; a.face_offsets = p.face_offsets;
    a.n_vertices = p.n_vertices; a.n_faces = p.n_faces;
    a.vertices = p.vertices; a.colors = p.colors; a.faces = p.faces;
    return GSTEX_OK;
}

}  // namespace

extern "C" int gstex_tsdf_integrate(const gstex_tsdf_integrate_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_tsdf_integrate: null args");
    const gstex_tsdf_integrate_args& p = *args;
    IntegrateArgs a{};
    const int rc = check_volume("gstex_tsdf_integrate", p.vol, a.g);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(p.n_views >= 1 && p.n_views <= kMaxViews, "gstex_tsdf_integrate: n_views must be in [1, %d] (got %d)",
                  kMaxViews, p.n_views);
    GSTEX_REQUIRE(finite_f(p.sdf_trunc) && p.sdf_trunc > 0.0f, "gstex_tsdf_integrate: sdf_trunc must be finite and > 0 "
                  "(got %g)", (double)p.sdf_trunc);
    GSTEX_REQUIRE(finite_f(p.alpha_min) && p.alpha_min > 0.0f, "gstex_tsdf_integrate: alpha_min must be finite and > 0 "
                  "(got %g)", (double)p.alpha_min);
    GSTEX_REQUIRE(finite_f(p.near_z) && p.near_z > 0.0f, "gstex_tsdf_integrate: near_z must be finite and > 0 (got %g)",
                  (double)p.near_z);
    GSTEX_REQUIRE(finite_f(p.depth_trunc) && p.depth_trunc >= 0.0f,
                  "gstex_tsdf_integrate: depth_trunc must be finite and >= 0 (got %g)", (double)p.depth_trunc);
    GSTEX_REQUIRE(p.views, "gstex_tsdf_integrate: null view table");
    for (int q = 0; q < p.n_views; ++q) {
        const gstex_tsdf_view& s = p.views[q];
        GSTEX_REQUIRE(s.cam.H > 0 && s.cam.W > 0 && (long long)s.cam.H * s.cam.W < (1ll << 31),
                      "gstex_tsdf_integrate: view %d: invalid image size (H=%d, W=%d)", q, s.cam.H, s.cam.W);
        GSTEX_REQUIRE(finite_f(s.cam.fx) && finite_f(s.cam.fy) && finite_f(s.cam.cx) && finite_f(s.cam.cy) &&
                          s.cam.fx > 0.0f && s.cam.fy > 0.0f,
                      "gstex_tsdf_integrate: view %d: fx, fy must be finite and > 0, cx, cy finite", q);
        GSTEX_REQUIRE(s.cam.viewmat && s.depth && s.alpha, "gstex_tsdf_integrate: view %d: null pointer", q);
        GSTEX_REQUIRE(!p.vol.color || s.rgb, "gstex_tsdf_integrate: view %d: null rgb, which a colour volume needs", q);
        GSTEX_REQUIRE(aligned(s.cam.viewmat, 4) && aligned(s.depth, 4) && aligned(s.alpha, 4) && aligned(s.rgb, 4),
                      "gstex_tsdf_integrate: view %d: misaligned pointer (4-byte words)", q);
        ViewK& k = a.v[q];
        k.viewmat = s.cam.viewmat; k.depth = s.depth; k.alpha = s.alpha; k.rgb = s.rgb;
        k.fx = s.cam.fx; k.fy = s.cam.fy; k.cx = s.cam.cx; k.cy = s.cam.cy;
        k.fw = (float)s.cam.W; k.fh = (float)s.cam.H; k.W = s.cam.W;
    }
    a.tsdf = p.vol.tsdf; a.weight = p.vol.weight; a.color = p.vol.color;
    a.n_views = p.n_views;
    a.sdf_trunc = p.sdf_trunc; a.alpha_min = p.alpha_min; a.depth_trunc = p.depth_trunc; a.near_z = p.near_z;
    tsdf_integrate_kernel<<<div_up(a.g.n_vox, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_tsdf_integrate");
}

extern "C" int gstex_mesh_extract_mark(const gstex_mesh_extract_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_mesh_extract_mark: null args");
    ExtractArgs a{};
    const int rc = fill_extract("gstex_mesh_extract_mark", *args, a);
    if (rc != GSTEX_OK) return rc;
    const hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(a.edge_mask, 0, sizeof(int32_t) * (size_t)a.g.n_vox, st) != hipSuccess)
        return launch_status("gstex_mesh_extract_mark (zeroing the edge mask)");
    const int blocks = div_up(a.g.n_vox, kThreads);
    mesh_mark_kernel<<<blocks, kThreads, 0, st>>>(a);
    mesh_count_kernel<<<blocks, kThreads, 0, st>>>(a.g.n_vox, a.edge_mask, a.vertex_count);
    return launch_status("gstex_mesh_extract_mark");
}

extern "C" int gstex_mesh_extract_emit(const gstex_mesh_extract_args* args, void* stream) {
    GSTEX_REQUIRE(args, "gstex_mesh_extract_emit: null args");
    const gstex_mesh_extract_args& p = *args;
    ExtractArgs a{};
    const int rc = fill_extract("gstex_mesh_extract_emit", p, a);
    if (rc != GSTEX_OK) return rc;
    GSTEX_REQUIRE(p.n_vertices >= 0 && p.n_faces >= 0 && p.n_vertices < (1ll << 31) && 3 * p.n_faces < (1ll << 33),
                  "gstex_mesh_extract_emit: invalid sizes (n_vertices=%lld, n_faces=%lld)", (long long)p.n_vertices,
                  (long long)p.n_faces);
    if (p.n_vertices == 0 && p.n_faces == 0) return GSTEX_OK;
    GSTEX_REQUIRE(p.vertex_offsets && p.face_offsets, "gstex_mesh_extract_emit: null offsets");
    GSTEX_REQUIRE(p.n_vertices == 0 || p.vertices, "gstex_mesh_extract_emit: null vertices");
    GSTEX_REQUIRE(p.n_faces == 0 || p.faces, "gstex_mesh_extract_emit: null faces");
    GSTEX_REQUIRE(!p.colors || p.vol.color, "gstex_mesh_extract_emit: colors need a colour volume");
    GSTEX_REQUIRE(aligned(p.vertex_offsets, 4) && aligned(p.face_offsets, 4) && aligned(p.vertices, 4) &&
                      aligned(p.colors, 4) && aligned(p.faces, 4),
                  "gstex_mesh_extract_emit: misaligned pointer (4-byte words)");
    mesh_emit_kernel<<<div_up(a.g.n_vox, kThreads), kThreads, 0, as_stream(stream)>>>(a);
    return launch_status("gstex_mesh_extract_emit");
}
