// gstex_internal.h — host-side hooks between the library's translation units (not part of the C ABI): the spans the
// training prologue (trainstep.hip) zeroes inside its scan kernel so that the binning and the raster forward launched
// right after it skip their own fill launches.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gstex {

struct ZeroSpan {
    void* ptr;
    size_t bytes;  // a multiple of 16; ptr 16-byte aligned
};

// binning.hip: the per-tile pair counters of a gstex_bin_sort workspace (zeroed before its count kernel; a caller that
// has zeroed the span on the stream passes GSTEX_BIN_COUNT_ZEROED and no fill is launched)
ZeroSpan bin_count_span(void* workspace, int32_t n_tiles, int64_t n_isect);
// raster_fwd.hip: the span of a raster aux buffer the forward accumulates unit costs, launch order and the unit-order
// histogram into (zeroed before the forward; gstex_raster_fwd_args.aux_zeroed tells the forward it already is)
ZeroSpan raster_aux_zero_span(void* aux, int64_t n_isect, int32_t n_tiles, int32_t channels);
// raster_fwd.hip, diagnostic builds (GSTEX_STATS != 0) only: the forward unit's counter array (raster_diag.h), which
// gstex_debug_stats in raster_bwd.hip adds to its own.  Returns 0, or 2 when the copy failed.
int raster_fwd_debug_stats(unsigned long long* out);

}  // namespace gstex
