// nn_grid.h — the uniform grid of gstex_nn_grid as the kernels of neighbors.hip and cluster.hip see it: the kernel
// form of the struct, a query's unclamped cell, the ring-stop margin and the host-side argument check.  The ring walk
// itself is stated once per unit (neighbors.hip carries a top-k through it, cluster.hip a fixed radius).
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

inline bool finite_f(float x) { return x == x && x - x == 0.0f; }
inline bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

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
