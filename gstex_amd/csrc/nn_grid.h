// nn_grid.h — the uniform grid of gstex_nn_grid as the kernels of neighbors.hip and cluster.hip see it: the kernel
// form of the struct, the host-side argument check and the ring walk, walk_rings, stated once for both units
// (neighbors.hip carries a sorted top-k through it, cluster.hip a fixed radius).
#pragma once

#include "gstex_common.h"
#include "gstex_error.h"

namespace gstex {

constexpr float kCellLimit = 536870912.0f;    // 2^29: a query's unclamped cell is kept within +-2^29 per axis
constexpr float kRingMargin = 0.9990234375f;  // 1 - 2^-10 (the rounding of the cell assignment)

struct GridK {
    float ox, oy, oz, h;
    int nx, ny, nz;
};

// the query's unclamped cell along one axis: floor((q - o) / h), kept within +-2^29 (a query that far outside is
// farther from the grid than its kept cell says, so the ring bound stays a lower bound)
__device__ __forceinline__ int query_cell_axis(float q, float o, float h) {
    const float t = floorf((q - o) / h);
    return (int)fminf(fmaxf(t, -kCellLimit), kCellLimit);  // (NaN -> -2^29)
}

// The Chebyshev rings of cells around the query's cell, nearest first: scan(p, pe) for every contiguous run of records
// of each ring's cells, every cell of the grid at most once, until bound(), the squared radius still of interest, is
// within the ring bound.  p and pe are cell_start's own values: the caller keeps them inside its records.  After
// ring r >= 1 every record not yet visited lies in a ring beyond r, at least ((float)r h)(1 - 2^-10) from the query.
template <class Scan, class Bound>
__device__ __forceinline__ void walk_rings(const GridK& g, const int32_t* __restrict__ cell_start, float qx, float qy,
                                           float qz, Scan&& scan, Bound&& bound) {
    const int cx = query_cell_axis(qx, g.ox, g.h), cy = query_cell_axis(qy, g.oy, g.h),
              cz = query_cell_axis(qz, g.oz, g.h);
    // the rings that meet the grid: from the Chebyshev distance of the cell to the grid's box ...
    const int out_x = max(max(-cx, cx - (g.nx - 1)), 0), out_y = max(max(-cy, cy - (g.ny - 1)), 0),
              out_z = max(max(-cz, cz - (g.nz - 1)), 0);
    const int r_first = max(max(out_x, out_y), out_z);
    // ... to the one that has left it on every side
    const int far_x = max(cx, (g.nx - 1) - cx), far_y = max(cy, (g.ny - 1) - cy), far_z = max(cz, (g.nz - 1) - cz);
    const int r_last = max(max(far_x, far_y), far_z);

    for (int r = r_first; r <= r_last; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.nx - 1);
        const int xl = cx - r, xr = r > 0 ? cx + r : -1;  // (ring 0: one cell, not twice)
        const bool x_ends = (xl >= 0 && xl < g.nx) || (xr >= 0 && xr < g.nx);
        // Row (z, y) of the ring, its cells starting at `base`.  On a face of the ring its cells x0..x1 are contiguous,
        // and so are their records: one run.  Through the ring's inside: the two end cells, where they are in the grid.
        auto scan_row = [&](int base, bool face) {
            if (face) {
                if (x0 <= x1) scan(cell_start[base + x0], cell_start[base + x1 + 1]);
                return;
            }
            if (xl >= 0 && xl < g.nx) scan(cell_start[base + xl], cell_start[base + xl + 1]);
            if (xr >= 0 && xr < g.nx) scan(cell_start[base + xr], cell_start[base + xr + 1]);
        };
        for (int z = z0; z <= z1; ++z) {
            const bool z_face = (z - cz == r) || (cz - z == r);
            const int slab = z * g.ny;
            if (z_face || x_ends) {
                for (int y = y0; y <= y1; ++y)
                    scan_row((slab + y) * g.nx, z_face || (y - cy == r) || (cy - y == r));
            } else {  // only the rows on the ring's two y faces hold cells of it
                const int ya = cy - r, yb = cy + r;
                if (ya >= 0 && ya < g.ny) scan_row((slab + ya) * g.nx, true);
                if (yb >= 0 && yb < g.ny) scan_row((slab + yb) * g.nx, true);
            }
        }
        if (r >= 1) {
            const float lb = ((float)r * g.h) * kRingMargin;
            if (lb * lb >= bound()) break;
        }
    }
}

inline int check_grid(const char* who, const gstex_nn_grid* grid, GridK& g) {
    GSTEX_REQUIRE(grid, "%s: null grid", who);
    GSTEX_REQUIRE(finite_f(grid->cell_size) && grid->cell_size > 0.0f, "%s: cell_size must be finite and > 0 (got %g)",
                  who, (double)grid->cell_size);
    GSTEX_REQUIRE(finite_f(grid->origin[0]) && finite_f(grid->origin[1]) && finite_f(grid->origin[2]),
                  "%s: the origin must be finite", who);
    GSTEX_REQUIRE(grid->nx >= 1 && grid->ny >= 1 && grid->nz >= 1, "%s: every dim must be >= 1 (got nx=%d, ny=%d, "
                  "nz=%d)", who, grid->nx, grid->ny, grid->nz);
    const long long cells = (long long)grid->nx * grid->ny * grid->nz;
    if (grid->nx > GSTEX_NN_MAX_AXIS_CELLS || grid->ny > GSTEX_NN_MAX_AXIS_CELLS ||
        grid->nz > GSTEX_NN_MAX_AXIS_CELLS || cells > GSTEX_NN_MAX_CELLS) {
        set_error("%s: too many cells (nx=%d, ny=%d, nz=%d; at most %d per axis and %d in all)", who, grid->nx,
                  grid->ny, grid->nz, GSTEX_NN_MAX_AXIS_CELLS, GSTEX_NN_MAX_CELLS);
        return GSTEX_ERR_UNSUPPORTED;
    }
    g.ox = grid->origin[0]; g.oy = grid->origin[1]; g.oz = grid->origin[2]; g.h = grid->cell_size;
    g.nx = grid->nx; g.ny = grid->ny; g.nz = grid->nz;
    return GSTEX_OK;
}

inline long long cells_of(const GridK& g) { return (long long)g.nx * g.ny * g.nz; }

}  // namespace gstex
