/*
 * gstex_hip.h — C-ABI of libgstex_hip.so, the MI355X (gfx950) textured-2DGS rasterizer.
 *
 * This is the drop-in boundary for the `gstex_cuda` native extension that the reference
 * (nvnhat95/GStex) imports but does not vendor (`.gitmodules:1-3`, submodules/GStex_cuda is
 * empty).  Each entry point below replaces one native op behind a reference call site:
 *
 *   gstex_project_points      <- gstex_cuda.get_aabb_2d.project_points      (nerfstudio/models/gstex.py:1077)
 *   gstex_aabb_2d(+_bwd)      <- gstex_cuda.get_aabb_2d.get_aabb_2d          (gstex.py:1079)
 *   gstex_num_tiles_hit       <- gstex_cuda.get_aabb_2d.get_num_tiles_hit_2d (gstex.py:1080)
 *   gstex_scan_offsets,
 *   gstex_bin_sort            <- tile binning + per-tile depth sort inside texture_gaussians
 *                                (args gstex.py:1136-1139,1158)
 *   gstex_raster_setup,
 *   gstex_raster_fwd          <- gstex_cuda.texture.texture_gaussians forward (gstex.py:1133-1162)
 *   gstex_raster_bwd,
 *   gstex_raster_setup_bwd    <- texture_gaussians backward (autograd, engine/trainer.py:460)
 *   gstex_sh_fwd / _bwd       <- gstex_cuda.sh.spherical_harmonics           (gstex.py:1109,1111)
 *   gstex_texture_sample(+_bwd) <- gstex_cuda.texture_sample.texture_sample  (models/jagged_texture.py:138)
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer to contiguous row-major fp32 / int32 memory, except
 *     `const gstex_camera*` and the `*_args` structs, which are HOST structs (read at call time) of
 *     device pointers.
 *   - `stream` is a hipStream_t (NULL = default stream). Calls only enqueue work: no allocation,
 *     no host synchronisation.
 *   - Scratch memory is caller-owned: query the size with the *_workspace_size function, allocate
 *     it (e.g. with the torch caching allocator) and pass it in.
 *   - Return value: 0 (GSTEX_OK) or a gstex_status; the message of the last failure on the calling
 *     thread is returned by gstex_last_error().
 */
#ifndef GSTEX_HIP_H
#define GSTEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 19: one exported symbol per operation.  The variant entry points of ABI 7-17 are folded into their base calls as
 * nullable arguments, flags or struct fields: gstex_raster_fwd / gstex_raster_bwd take argument structs (the _zero
 * variants' buffers are fields; aux_zeroed replaces the settings bit 28), gstex_raster_setup_bwd takes a struct with
 * fold_aabb (was _aabb), gstex_bin_sort takes tile_order and flags (was _ordered, _capped), gstex_scan_offsets takes a
 * nullable guard (was _guarded), gstex_adam_step takes flags, grad_scale and skip (was _ex, _scaled, _guarded).
 * ABI 18 (round 6): the hipGraph step support of ABI 16 (event-record nodes, gstex_adam_step_scheduled) and the
 * split-backward settings bit of ABI 15 are removed (measured slower).
 * The number counts incompatible changes: an addition that leaves every existing symbol's signature and meaning alone
 * keeps it, and is marked "added within ABI 19 (additive)" where it is declared (gstex_loss_target_*,
 * gstex_eval_metrics*, gstex_paint_*, gstex_raster_bwd_variant). */
#define GSTEX_ABI_VERSION 19

/* Per-record layout of the splat table written by gstex_raster_setup (floats). */
#define GSTEX_REC_FLOATS 32
/* Per-(tile, splat, quadrant) gradient partial row written by gstex_raster_bwd (floats). */
#define GSTEX_PARTIAL_FLOATS 32
#define GSTEX_PARTIAL_FLOATS_PHOTO 24
/* Per-splat fp64 row of a near-edge-on splat written by gstex_raster_setup into hp_records (doubles, ABI 18). */
#define GSTEX_HP_DOUBLES 12

/* settings bitfield (GStexModelConfig.settings, gstex.py:194-197) */
#define GSTEX_SETTING_AA_BLUR (1 << 9)   /* 2DGS screen-space low-pass */
#define GSTEX_SETTING_DIST_REG (1 << 10) /* 2DGS NDC depth-distortion output */
#define GSTEX_SETTING_EDIT (1 << 13)     /* texture_edit request (gstex.py:599) */
#define GSTEX_SETTING_EVAL_NORMAL (1 << 15) /* eval normal/edit render (gstex.py:1198): normal output unit-length, forward only */

typedef enum {
    GSTEX_OK = 0,
    GSTEX_ERR_INVALID_ARG = 1,
    GSTEX_ERR_LAUNCH = 2,
    GSTEX_ERR_UNSUPPORTED = 3,
    GSTEX_ERR_WORKSPACE = 4
} gstex_status;

/* Pinhole camera (a HOST struct holding DEVICE pointers, so no host sync is needed to read the
 * model's on-GPU matrices).  viewmat = first 3 rows of world->camera (OpenCV axes, after the y/z
 * flip of gstex.py:1031-1041), row-major DEVICE float[12].  c2w = its inverse, row-major DEVICE
 * float[16] (only the camera centre c2w[:3,3] is read; NULL = derive it from viewmat). */
typedef struct {
    const float* viewmat;
    const float* c2w;
    float fx, fy, cx, cy;
    int32_t H, W, block;
} gstex_camera;

const char* gstex_last_error(void);
int gstex_abi_version(void);

/* ---- per-splat preprocessing ---------------------------------------------------------- */
int gstex_project_points(int32_t n, const float* means, const gstex_camera* cam,
                         float* xys, float* depths, void* stream);
int gstex_project_points_bwd(int32_t n, const float* means, const gstex_camera* cam,
                             const float* v_xys, const float* v_depths, float* v_means,
                             void* stream);
int gstex_aabb_2d(int32_t n, const float* means, const float* scales, float glob_scale,
                  const float* quats, const gstex_camera* cam, float* centers, float* extents,
                  void* stream);
/* Writes the gradient of the AABB centre to v_means / v_scales / v_quats (every element; zero for
   splats with no centre gradient or culled). */
int gstex_aabb_2d_bwd(int32_t n, const float* means, const float* scales, float glob_scale,
                      const float* quats, const gstex_camera* cam, const float* v_centers,
                      float* v_means, float* v_scales, float* v_quats, void* stream);
int gstex_num_tiles_hit(int32_t n, const float* centers, const float* extents, int32_t H,
                        int32_t W, int32_t block, int32_t* num_tiles_hit, void* stream);
/* The three preprocessing outputs a render needs, in one pass (ABI 10): depths[n] (the view depth of
 * gstex_project_points), centers / extents[n][2] (gstex_aabb_2d) and num_tiles_hit[n]
 * (gstex_num_tiles_hit with cam->H, cam->W, cam->block), bit-identical to the three calls.  No
 * backward: a caller that needs the centre gradient uses gstex_raster_setup_bwd with fold_aabb. */
int gstex_preprocess(int32_t n, const float* means, const float* scales, float glob_scale,
                     const float* quats, const gstex_camera* cam, float* depths, float* centers,
                     float* extents, int32_t* num_tiles_hit, void* stream);

/* ---- binning + per-tile depth sort ---------------------------------------------------- */
size_t gstex_scan_workspace_size(int32_t n);
/* Read-back-free binning (ABI 13).  The reference sizes its pair buffers from the pair total on the host
 * (gstex.py:1045-1052, 1127: a device-to-host read and a stream synchronisation every render).  Capacity mode sizes
 * them from a capacity instead and keeps the total on the device:
 *   gstex_scan_offsets with a guard: the thread that writes the total offsets[n] also writes
 *     *step_flag = (total > capacity) ? 1.0f : 0.0f (first != 0: the step's first render; otherwise the larger of
 *     the two) and, when host_count != NULL, the total into host_count -- memory the device can write and the host
 *     reads (pinned, mapped) once the stream has passed the scan: no copy, no synchronisation;
 *   gstex_bin_sort with GSTEX_BIN_CAPPED: n_isect = the capacity (buffers, workspace); the kernels read
 *     the total from offsets[n], and a total above the capacity leaves every tile empty (nothing is written past the
 *     buffers);
 *   gstex_adam_step with skip: does nothing when *skip != 0 (an overflowed step's update
 *     is skipped on the device; the host grows the capacity when it sees the total).
 * The raster entry points take the capacity as n_isect (it only sizes the aux layout and the backward's grid, whose
 * surplus units exit at once). */
typedef struct gstex_pair_guard {
    int64_t capacity;
    float* step_flag;
    int32_t* host_count; /* nullable */
    int32_t first;
} gstex_pair_guard;
/* offsets[0..n] = exclusive prefix sum of num_tiles_hit; offsets[n] = total intersections.  guard (ABI 13; nullable =
 * the plain scan): the pair-capacity guard above, capacity >= 0. */
int gstex_scan_offsets(int32_t n, const int32_t* num_tiles_hit, int32_t* offsets,
                       void* workspace, size_t workspace_bytes, const gstex_pair_guard* guard, void* stream);
size_t gstex_bin_workspace_size(int32_t n, int64_t n_isect, int32_t n_tiles);
/* Emits one (tile, splat) pair per covered tile, buckets them per tile and sorts every tile's
 * list by (depth bits, splat id).  Outputs: tile_ranges[n_tiles][2] = [start, end) into
 * sorted_ids; sorted_ids[n_isect] = splat id; sorted_slots[n_isect] = emission index
 * offsets[id] + k (k = row-major rank of the tile inside the splat's tile rectangle).
 * tile_order (ABI 8; nullable = not written): tile_order[n_tiles], the largest-first launch order
 * gstex_tile_order would compute from the resulting tile_ranges (same keys, same ranking): the
 * tile sort already ranks the buckets, so the raster forward reuses that order instead of a
 * second ranking launch.
 * flags: GSTEX_BIN_CAPPED (ABI 13; needs tile_order): n_isect is the pair buffers' capacity and the total is read on
 * the device, see above.  GSTEX_BIN_COUNT_ZEROED: the caller has already zeroed the workspace's per-tile pair counters
 * on the stream (gstex_train_prologue does, inside its scan kernel), so no fill is launched.  Other bits are
 * rejected. */
#define GSTEX_BIN_CAPPED 1
#define GSTEX_BIN_COUNT_ZEROED 2
int gstex_bin_sort(int32_t n, int64_t n_isect, const float* centers, const float* extents,
                   const float* depths, const int32_t* offsets,
                   int32_t H, int32_t W, int32_t block, int32_t* tile_ranges,
                   int32_t* sorted_ids, int32_t* sorted_slots, int32_t* tile_order, int32_t flags,
                   void* workspace, size_t workspace_bytes, void* stream);
/* n device-writable host words (hipHostMalloc, mapped; zeroed): *host for the host, *device for
 * gstex_pair_guard.host_count.  Freed with gstex_host_words_free(host). */
int gstex_host_words_alloc(int32_t n, int32_t** host, int32_t** device);
int gstex_host_words_free(int32_t* host);

/* Lightweight events (ABI 14).  kind GSTEX_EVENT_TIMING: timing only, created with hipEventDisableSystemFence -- no
 * system-scope release / acquire (an L2 writeback and invalidate) when recorded, so a pair around a kernel measures it
 * without perturbing the loop it sits in (a default-event pair around each raster launch cost ~10 us of device time per
 * pair in bench.py's A/B); not for host synchronisation.  kind GSTEX_EVENT_ORDER: no timing, a device-scope release
 * (hipEventReleaseToDevice) -- for ordering one stream after another on the same device (gstex_stream_wait_event).
 * elapsed: milliseconds between two recorded, completed timing events. */
#define GSTEX_EVENT_TIMING 0
#define GSTEX_EVENT_ORDER 1
int gstex_event_create(int32_t kind, void** event);
int gstex_event_record(void* event, void* stream);
int gstex_event_elapsed(void* start, void* end, float* ms);
int gstex_stream_wait_event(void* stream, void* event);
int gstex_event_destroy(void* event);

/* Largest-first launch order of the tiles: tile_order[n_tiles] lists the tiles by descending
 * pair count (ties by tile index).  Pass it to gstex_raster_fwd / gstex_texture_edit, whose
 * workgroups the hardware dispatches in launch order round-robin over the 8 XCDs; NULL there
 * means row-major order.  Scheduling only: outputs do not depend on it.  Above 16384 tiles the
 * order is row-major. */
int gstex_tile_order(int32_t n_tiles, const int32_t* tile_ranges, int32_t* tile_order, void* stream);

/* ---- rasterizer --------------------------------------------------------------------- */
/* Builds the per-splat raster record table records[n][GSTEX_REC_FLOATS].
 * hp_records (ABI 18; nullable = none): a device double[n][GSTEX_HP_DOUBLES] buffer.  A splat whose normal is within
 * ~6 degrees of edge-on to its view direction (|n . d| < 0.1) is then marked near edge-on -- the sign bit of its
 * record opacity is set (every kernel reads the magnitude) -- and its row g receives the fp64 affine homography (A, B,
 * Pz), anchor and depth row; other rows are not written.  Pass the same buffer to gstex_raster_fwd and
 * gstex_raster_bwd, which evaluate those splats' pairs from it (the offset from the anchor and the homogeneous
 * point in fp64, rounded once: their fp32 evaluation is ill-conditioned).  gstex_texture_edit ignores
 * the marks (pass records built without hp_records). */
int gstex_raster_setup(int32_t n, const float* means, const float* scales, float glob_scale,
                       const float* quats, const float* rgbs, const float* opacities,
                       const float* centers, const float* uv0, const float* umap,
                       const float* vmap, const int32_t* texture_dims,
                       const int32_t* num_tiles_hit, const gstex_camera* cam, float* records,
                       double* hp_records, void* stream);
/* What the raster forward and its backward share (ABI 19): a caller fills it once for the forward and hands the same
 * value to the backward.  The argument structs are HOST structs of device pointers, read at call time. */
typedef struct gstex_raster_scene {
    gstex_camera cam;
    int32_t channels;        /* texture channels C, in [1, 8] */
    int32_t settings;        /* the reference's settings bits (GSTEX_SETTING_*); anything else is rejected */
    const float* background; /* a device float[3] (or NULL = black) added as T_final * background */
    const float* records;    /* gstex_raster_setup's table */
    const double* hp_records; /* nullable (ABI 18): gstex_raster_setup's near-edge-on rows -- the marked splats' pairs
                                 are then evaluated from them (p in fp64, rounded once); the backward must take the
                                 same decisions.  NULL: every pair from the fp32 record (the marks ignored). */
    const int32_t* tile_ranges;
    const int32_t* sorted_ids;
    const float* texture;    /* Texel values: the texels are read as tex_scale * texture + tex_bias (1, 0 = as stored),
                                so a caller that keeps SH-DC coefficients (gstex.py:1119 passes SH2RGB(texture_dc) =
                                0.28209 x + 0.5) can pass the store itself; the backward's v_texture is then the
                                gradient w.r.t. the stored values. */
    int64_t n_texels;
    float tex_scale;
    float tex_bias;
    float* state;            /* state[H*W][4] = {T_final, M1, M2, last_contributor (as int bits)}: written by the
                                forward, read by the backward */
    int64_t n_isect;         /* pairs in sorted_ids (capacity mode: the capacity) */
    void* aux;               /* forward: NULL = no backward follows; backward: required.  A gstex_raster_aux_bytes(
                                n_isect, n_tiles, channels) device workspace the forward fills for the backward -- its
                                per-wave cull bits (per tile, 8x8 pixel quadrant and tile-list position), per backward
                                unit (tile, quadrant, segment of 256 list positions) the number of splats it evaluated,
                                and per-pixel checkpoints (transmittance and accumulators) at the segment boundaries of
                                deep lists -- and the backward writes its launch order into.  Untouched in between. */
} gstex_raster_scene;
/* Forward composite. Outputs are [H][W][k] row-major.  out_depth, out_reg and out_normal may be
 * NULL together (geometric outputs not produced; the backward then takes no gradient for them). */
typedef struct gstex_raster_fwd_args {
    gstex_raster_scene scene;
    const int32_t* tile_order; /* nullable = row-major (gstex_tile_order) */
    float* out_img;
    float* out_depth;
    float* out_reg;
    float* out_alpha;
    float* out_tex;
    float* out_normal;
    /* zero_buf[0, zero_floats) and zero_buf2[0, zero_floats2) are zeroed too (ABI 11; NULL / 0 = none): the buffers the
     * backward accumulates into (the texel gradient, the fast mode's per-splat partials), cleared by the forward's grid
     * with streaming stores the raster work hides (no separate fills). */
    float* zero_buf;
    int64_t zero_floats;
    float* zero_buf2;
    int64_t zero_floats2;
    int32_t aux_zeroed;      /* non-zero (ABI 17; was settings bit 28): the aux span the forward accumulates its unit
                                costs, launch order and unit-order histogram into was zeroed by gstex_train_prologue
                                (args.raster_aux, same n_isect / tiles / channels) on the same stream, so the forward
                                skips its own fill.  Set it only after such a prologue call. */
} gstex_raster_fwd_args;
int gstex_raster_fwd(const gstex_raster_fwd_args* args, void* stream);
size_t gstex_raster_aux_bytes(int64_t n_isect, int32_t n_tiles, int32_t channels);
/* Launch order of n_units backward units: unit_key = cost (bits 0-23, clamped to 1023) | XCD group (bits 24-26).
 * Units of cost 0 get no position; the others are sorted by descending cost within their group and the groups
 * interleaved (k-th unit of group g at position 8 k + g: round-robin dispatch puts it on XCD g), or, when the
 * groups are too uneven (8 x the largest group > n_units), sorted by descending cost overall.  unit_order[n_units]
 * holds -1 at unused positions; order within equal costs is unspecified.  scratch =
 * gstex_unit_order_scratch_words() int32 of device workspace.  gstex_raster_bwd calls it on its aux. */
int gstex_unit_order(int32_t n_units, const int32_t* unit_key, int32_t* unit_order, int32_t* scratch,
                     void* stream);
size_t gstex_unit_order_scratch_words(void);
/* Backward composite. Needs the forward state and the forward's aux (required; the backward also writes its
 * launch order into it).  Any of v_img ... v_normal may be NULL (that output's gradient is zero).  Texel blocks
 * that run past n_texels (corrupt texture_dims) are neither read nor written.  One wave per backward unit (tile,
 * 8x8 pixel quadrant q, segment): for every pair (emission slot s) the quadrant contributes to, writes the row
 * partials[(4 s + q) * R ...] (n_isect * 4 rows of R floats allocated; rows of pairs a quadrant does not reach are
 * never written) and sets byte q of row_flags[s] (n_isect uint32 words, zeroed by this call on the stream);
 * accumulates (+=) texel gradients into v_texture[n_texels][C].  R = GSTEX_PARTIAL_FLOATS_PHOTO (24) when neither
 * v_depth nor v_normal is given and v_reg is NULL or distortion (settings bit 10) is off -- the photometric training
 * step -- else GSTEX_PARTIAL_FLOATS (32); pass the same R to gstex_raster_setup_bwd as row_floats.
 * row_flags == NULL (ABI 9, the fast mode): instead of rows, every (pair, quadrant) sum is added with float
 * atomics into partials[g * R ...], an (n_splats, R) accumulator the caller has zeroed -- no per-pair rows, no
 * summing pass in setup_bwd; the splat gradients then depend on the atomics' order in their last bits (as the
 * texel gradients always do).  With row_flags the splat gradients are bitwise reproducible. */
typedef struct gstex_raster_bwd_args {
    gstex_raster_scene scene; /* the forward's (hp_records included: the same pairs evaluated the same way) */
    const int32_t* sorted_slots;
    const float* v_img;
    const float* v_depth;
    const float* v_reg;
    const float* v_alpha;
    const float* v_tex;
    const float* v_normal;   /* must be NULL with settings bit 15 (the unit-normal eval render has no gradient) */
    float* partials;
    uint32_t* row_flags;     /* nullable = the fast mode */
    float* v_texture;
    /* zero_buf[0, zero_floats) is zeroed by the backward's grid (ABI 17; NULL / 0 = none): a persistent gradient
     * buffer of the NEXT step (gstex_amd.fused double-buffers the texel gradient: this backward accumulates into
     * v_texture and zeroes the other buffer, which the next step's backward accumulates into) -- instead of the
     * forward's zeroing (gstex_raster_fwd_args.zero_buf).  zero_buf must not be v_texture. */
    float* zero_buf;
    int64_t zero_floats;
} gstex_raster_bwd_args;
int gstex_raster_bwd(const gstex_raster_bwd_args* args, void* stream);
/* Which kernel build gstex_raster_bwd launches for these arguments -- added within ABI 19 (additive); a host-side
 * query, nothing is launched or validated.  GSTEX_BWD_TRAIN, the photometric training step's call, exactly when:
 * scene.channels == 3; no depth / normal / (enabled) distortion gradient; row_flags == NULL; v_img, v_alpha and
 * v_tex given; and v_tex == v_img, ONE upstream gradient for both outputs (at 3 channels the two layouts are the
 * same, and the loss's gradient for both is the same image: gstex_loss_bwd with d_tex == d_img).  That build reads
 * it once, carries no deterministic row path and runs at a higher occupancy; its sums are formed in the generic
 * build's order.  Every other call: GSTEX_BWD_GENERIC.  NULL args: -1. */
enum { GSTEX_BWD_GENERIC = 0, GSTEX_BWD_TRAIN = 1 };
int gstex_raster_bwd_variant(const gstex_raster_bwd_args* args);
/* Sums each splat's flagged partial rows (slot-major, quadrant-minor order: bitwise reproducible) and chains
 * them to the splat parameters. Outputs are overwritten.  partials is consumed: each splat's sums are written
 * over its first row (the rows are backward scratch, not read again). */
typedef struct gstex_raster_setup_bwd_args {
    int32_t n;
    float glob_scale;
    int32_t row_floats;      /* the raster backward's R */
    int32_t fold_aabb;       /* non-zero: gstex_aabb_2d_bwd folded in -- for callers whose centres came from
                                gstex_aabb_2d on these same means / scales / quats (glob_scale, camera), the centre
                                gradient is chained through the AABB centre here and added to v_means / v_scales /
                                v_quats (bit-identical to running gstex_aabb_2d_bwd separately and adding the two
                                results); v_centers is still written. */
    int64_t n_rows;          /* ABI 15: the pair capacity the rows were allocated for (n_rows * 4 rows), or -1 when
                                offsets[n] is known to fit; with capacity-sized pair buffers (GSTEX_BIN_CAPPED) a total
                                offsets[n] > n_rows means the binning left every tile empty, and every splat is then
                                chained as pair-free (zero gradients) without reading rows past the allocation. */
    gstex_camera cam;
    const float* means;
    const float* scales;
    const float* quats;
    const float* umap;
    const float* vmap;
    const int32_t* num_tiles_hit;
    const int32_t* offsets;
    float* partials;
    const uint32_t* row_flags; /* NULL: partials is the backward's (n, row_floats) per-splat accumulator
                                  (gstex_raster_bwd without row_flags), chained directly */
    float* v_means;
    float* v_scales;
    float* v_quats;
    float* v_rgbs;
    float* v_opacities;
    float* v_centers;
    float* v_uv0;
} gstex_raster_setup_bwd_args;
int gstex_raster_setup_bwd(const gstex_raster_setup_bwd_args* args, void* stream);

/* The raster's view-matrix gradient -- added within ABI 19 (additive).  v_viewmat[3][4] = dL/d(cam.viewmat), its 12
 * entries taken as free variables (gsplat's v_viewmat; no orthonormality constraint is applied), OVERWRITTEN.
 * The render depends on V = [R|t] only through each splat's camera-space vectors W0 = R (su t_u), W1 = R (sv t_v),
 * W2 = R mu + t, so  dL/dV[r][:3] = sum_i dW0_r a_i + dW1_r b_i + dW2_r mu_i  and  dL/dV[r][3] = sum_i dW2_r.  The
 * texture-affine sums and the normal sum of the rows take no part: umap / vmap and the normal are world-space.
 *   Raster mode (partials != NULL): call it after gstex_raster_setup_bwd, with that call's n, glob_scale, row_floats,
 * fold_aabb, n_rows, cam, means, scales, quats, num_tiles_hit, offsets, partials and row_flags (read for NULL-ness
 * only: NULL = the (n, row_floats) accumulator, row g; else the sums gstex_raster_setup_bwd wrote over each splat's
 * first row).  partials is read, not consumed.  fold_aabb: the rows' centre gradient is chained through the AABB
 * centre (gstex_aabb_2d on these splats) and added.  A splat without pairs contributes zero, and so does every splat
 * when n_rows >= 0 and offsets[n] > n_rows.  v_centers must be NULL.
 *   Centre-only mode (partials == NULL): v_centers[n][2] is chained through the AABB centre alone -- the viewmat
 * gradient of gstex_aabb_2d; num_tiles_hit / offsets / row_flags / row_floats / n_rows / fold_aabb are not read.
 * Culled splats (centre = extent = 0 in gstex_aabb_2d) contribute zero.
 *   The chain is evaluated in fp64, one thread per splat; the sum is deterministic and in two stages: each block of 256
 * splats reduces its 12 values in fp64 into row b of workspace, one final block sums the rows in a fixed order (no
 * atomics: the same inputs give the same bits).  workspace: gstex_raster_viewmat_bwd_workspace(n) bytes =
 * ceil(n / 256) * 12 doubles, 8-byte aligned, caller-owned scratch.  No allocation, no synchronisation. */
typedef struct gstex_raster_viewmat_bwd_args {
    int32_t n;
    float glob_scale;
    int32_t row_floats;
    int32_t fold_aabb;
    int64_t n_rows;
    gstex_camera cam;
    const float* means;
    const float* scales;
    const float* quats;
    const int32_t* num_tiles_hit;
    const int32_t* offsets;
    const float* partials;
    const uint32_t* row_flags;
    const float* v_centers;
    double* workspace;
    float* v_viewmat;
} gstex_raster_viewmat_bwd_args;
size_t gstex_raster_viewmat_bwd_workspace(int32_t n);
int gstex_raster_viewmat_bwd(const gstex_raster_viewmat_bwd_args* args, void* stream);

/* ---- spherical harmonics (degree <= 4) ------------------------------------------------- */
int gstex_sh_fwd(int32_t n, int32_t degree, int32_t n_coeffs, const float* viewdirs,
                 const float* coeffs, float* colors, void* stream);
int gstex_sh_bwd(int32_t n, int32_t degree, int32_t n_coeffs, const float* viewdirs,
                 const float* v_colors, float* v_coeffs, void* stream);
/* The view-direction gradient of gstex_sh_fwd / gstex_sh_rest_fwd -- added within ABI 19 (additive).
 * v_viewdirs[i] = sum_{k, c} v_colors[i][c] * coeffs[i][k][c] * dY_k/d(viewdirs[i]) over the active degree's bases,
 * OVERWRITTEN.  k0 = 0: coeffs[n][n_coeffs][3] holds bases 0 .. n_coeffs - 1 (gstex_sh_fwd's layout); k0 = 1: the
 * DC-less rest layout of gstex_sh_rest_fwd (row k holds basis k + 1).  Y_k is what the forward evaluates: the basis
 * polynomial at viewdirs[i] / |viewdirs[i]| for degree >= 1, so the result is tangential (the polynomial's gradient
 * with its radial part removed, divided by |viewdirs[i]|); degree 0 gives zero.  Evaluated in fp64 per splat. */
int gstex_sh_dirs_bwd(int32_t n, int32_t degree, int32_t k0, int32_t n_coeffs, const float* viewdirs,
                      const float* coeffs, const float* v_colors, float* v_viewdirs, void* stream);

/* ---- jagged texture resample ------------------------------------------------------------ */
int gstex_texture_sample(int64_t n_query, int32_t channels, const int32_t* query_dims,
                         const float* texture, int64_t n_texels, const float* uv, float* out,
                         void* stream);
int gstex_texture_sample_bwd(int64_t n_query, int32_t channels, const int32_t* query_dims,
                             int64_t n_texels, const float* uv, const float* v_out,
                             float* v_texture, void* stream);

/* texture_edit (gstex.py:579-606, viewer paint tool): traverse each pixel's splats as
 * gstex_raster_fwd does (records from gstex_raster_setup, same tile lists/order); every counted pair
 * whose hit depth z satisfies depth_lo <= z <= depth_hi adds, to each of its 4 bilinear texels with
 * weight b and compositing weight w = alpha * T,  b * w * (a*r, a*g, a*b, a, 1)  to out[texel][5]
 * (ACCUMULATES: zero out first).  edit_rgb [H][W][3], edit_alpha/depth_lo/depth_hi [H][W]. */
int gstex_texture_edit(const gstex_camera* cam, int32_t settings, const float* records,
                       const int32_t* tile_ranges, const int32_t* tile_order, const int32_t* sorted_ids,
                       const float* edit_rgb, const float* edit_alpha, const float* depth_lo,
                       const float* depth_hi, int64_t n_texels, float* out, void* stream);

/* Paint a stroke into the texels -- added within ABI 19 (additive).  GStexModel.draw_from_view (gstex.py:489-606) after
 * its depth render, as two calls on a caller-owned accumulator acc[n_texels][5] that is ALL ZERO on entry to the
 * scatter and all zero again after the blend (allocate and fill it once; a replay of K edits reuses it).
 *
 * gstex_paint_scatter: gstex_texture_edit's traversal, accumulators and guards (the same device function), on the
 * records, tile lists and tile order the depth render was made from.  Differences:
 *   - the depth window is formed in the kernel from the rendered depth[H][W]: lo = depth - eps, hi = depth + eps, one
 *     rounded fp32 operation each (the bits of depth_output -+ 1e-2 in torch, gstex.py:568-569);
 *   - the stroke is one [H][W][4] image, straight alpha in channel 3: fp32 in [0, 1] (GSTEX_GT_F32, 16-byte aligned)
 *     or uint8 (GSTEX_GT_U8, 4-byte aligned), value = (float)v / 255.0f (a true division, as gstex_loss_target);
 *   - a pixel whose stroke alpha is exactly 0 adds only the weight channel acc[.][4]: its other four products are +-0
 *     and would leave the sums as they are;
 *   - records may carry gstex_raster_setup's near-edge-on marks (hp_records): this traversal reads the opacity's
 *     magnitude only and evaluates every pair from the fp32 record, so marked and unmarked tables give the same bits.
 * settings: as gstex_texture_edit (gstex.py:599 passes 1 << 13 alone: no AA blur in the edit traversal, whatever the
 * depth render used).
 *
 * gstex_paint_blend: one thread per texel t in [0, n_texels) on its row (c0, c1, c2, a, wt).  Where a > 0, each line
 * one rounded fp32 operation (gstex.py:603-605):
 *     weight = a / (wt + 1e-6f);  rgb_k = c_k / (a + 1e-6f);  out_k = rgb_k * weight + cur_k * (1 - weight)
 * written in place into texture[t][3]; where a == 0 the reference's expression returns cur and nothing is written.
 * cur_k = texture[t][k] for (scale, shift) = (1, 0); otherwise cur_k = fma(texture[t][k], scale, shift) (the fused
 * multiply-add the raster forward applies tex_scale / tex_bias with) and the write is (out_k - shift) / scale: with
 * (SH_C0, 0.5) the call edits the SH-DC store itself and texels it does not paint keep their bits.  Every row that was
 * not all zero is stored back as zeros.  n_texels == 0 launches nothing. */
typedef struct gstex_paint_scatter_args {
    gstex_camera cam;
    int32_t settings;          /* GSTEX_SETTING_* bits gstex_texture_edit accepts; anything else is rejected */
    int32_t stroke_dtype;      /* GSTEX_GT_F32 or GSTEX_GT_U8 */
    float eps;                 /* half-width of the depth window, >= 0 (the reference: 1e-2) */
    const float* records;      /* gstex_raster_setup's table */
    const int32_t* tile_ranges;
    const int32_t* tile_order; /* nullable = row-major */
    const int32_t* sorted_ids;
    const void* stroke;        /* H*W*4 */
    const float* depth;        /* H*W: the depth render of the same records */
    int64_t n_texels;
    float* acc;                /* n_texels*5, zero on entry */
} gstex_paint_scatter_args;
int gstex_paint_scatter(const gstex_paint_scatter_args* args, void* stream);
typedef struct gstex_paint_blend_args {
    int64_t n_texels;
    float* acc;                /* n_texels*5: the scatter's sums; zero again on return */
    float* texture;            /* at least n_texels*3, edited in place */
    float scale;               /* finite, not 0 */
    float shift;               /* finite */
} gstex_paint_blend_args;
int gstex_paint_blend(const gstex_paint_blend_args* args, void* stream);

/* ---- splat activations (train-step support) ---------------------------- */
/* Per splat: quats_n = q/|q|; scales = (clamp(exp(s0),1e-9), clamp(exp(s1),1e-9), 1e-5*mean of those);
 * opacities = sigmoid(o); uv0 = 0.5, umap/vmap = mappings[:,0/1] * R(normalize(quats_n))[:, 0/1];
 * viewdirs = normalize(means - campos).  mappings is [n][mappings_stride] (>= 2); campos a device float[3];
 * quats / quats_n / v_quats 16-byte aligned.  The backward writes v_quats (raw quaternions), v_log_scales
 * (third axis 0: detached) and v_opac_logits; a NULL upstream gradient counts as zero and a NULL output
 * is skipped. */
int gstex_activate_fwd(int32_t n, const float* means, const float* quats, const float* log_scales,
                       const float* opac_logits, const float* mappings, int32_t mappings_stride,
                       const float* campos, float* quats_n, float* scales, float* opacities, float* uv0,
                       float* umap, float* vmap, float* viewdirs, void* stream);
int gstex_activate_bwd(int32_t n, const float* quats, const float* log_scales, const float* opacities,
                       const float* v_quats_n, const float* v_scales, const float* v_opacities,
                       float* v_quats, float* v_log_scales, float* v_opac_logits, void* stream);
/* SH colour from the non-DC coefficients only (the caller zeroes the DC term, gstex.py:1100):
 * coeffs_rest[n][n_rest][3] holds bases 1..n_rest; same result as gstex_sh_fwd on [0, coeffs_rest]. */
int gstex_sh_rest_fwd(int32_t n, int32_t degree, int32_t n_rest, const float* viewdirs,
                      const float* coeffs_rest, float* colors, void* stream);
int gstex_sh_rest_bwd(int32_t n, int32_t degree, int32_t n_rest, const float* viewdirs,
                      const float* v_colors, float* v_coeffs_rest, void* stream);

/* ---- photometric loss (train-step support) --------------------------------- */
/* rgb = clamp(img + tex[..., 0:3] + (1 - alpha) * background, 0, 1)      (gstex.py:1204-1205)
 * loss = (1 - ssim_lambda) * mean|gt - rgb| + ssim_lambda * (1 - SSIM(gt, rgb))  (gstex.py:1301-1322)
 * SSIM as pytorch_msssim: separable 11-tap window (window[11], host fp32), valid filtering,
 * C1 = 0.01^2, C2 = 0.03^2, mean over the (H-10) x (W-10) x 3 map.  Images are [H][W][k] row-major
 * device fp32; tex has C >= 3 channels (only 0..2 enter the loss).  loss_out (device float[3]) =
 * {loss, L1, SSIM}; rgb_out may be NULL.  The forward leaves in the workspace what the backward reads:
 * pass the same workspace to gstex_loss_bwd.  grad_loss is a device scalar (the loss's upstream
 * gradient); d_img, d_tex (channels >= 3 zero) and d_alpha are overwritten.  With C == 3, d_tex may be d_img (the
 * same address: the two gradients are the same image, written once; gstex_loss_target_bwd alike); with C > 3 that
 * is refused. */
size_t gstex_loss_workspace_size(int32_t H, int32_t W);
int gstex_loss_fwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex, const float* alpha,
                   const float* background, const float* gt, const float* window, float ssim_lambda,
                   float* rgb_out, float* loss_out, void* workspace, size_t workspace_bytes, void* stream);
int gstex_loss_bwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex, const float* alpha,
                   const float* background, const float* gt, const float* window, float ssim_lambda,
                   const float* grad_loss, float* d_img, float* d_tex, float* d_alpha, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The same loss on the target a dataset delivers -- added within ABI 19 (additive).
 * get_gt_img (gstex.py:1238-1247), composite_with_background (:1249-1260), the mask branch of get_loss_dict
 * (:1294-1299) and the MSE of get_metrics_dict's PSNR (:1262-1275) folded into the loss kernels' staging loop.
 * Each line is one individually rounded fp32 operation:
 *   g_c  = the stored value (F32) or (float)v / 255.0f (U8); with four channels a = channel 3, converted alike
 *   gt_c = g_c (3 channels), or a * g_c + (1 - a) * background_c (4: two rounded products, then the sum)
 *   rgb_c as gstex_loss_fwd (rgb_out is the unmasked clamped image)
 *   m    = the mask value (F32), v != 0 ? 1 : 0 (BOOL), or 1 without a mask;  X_c = gt_c * m,  Y_c = rgb_c * m
 *   L1 = mean|X - Y|, SSIM = SSIM(X, Y) as gstex_loss_fwd; MSE = mean (rgb_c - gt_c)^2, unmasked
 *   terms_out (device float[4]) = {(1 - ssim_lambda) L1 + ssim_lambda (1 - SSIM), L1, SSIM, MSE}
 *   (PSNR = -10 log10(MSE) is the caller's); gt_out (nullable, H*W*3) = gt.
 * Backward: dL/drgb_c = m * dL/dY_c, gated by the clamp; d_img, d_tex, d_alpha as gstex_loss_bwd.
 * The target is a HOST struct of DEVICE pointers.  An RGBA pixel is read in one load: gt must be 4-byte (U8) or
 * 16-byte (F32) aligned.  The workspace is gstex_loss_target_workspace_size bytes (0 when H or W <= 10), shared by
 * the forward and its backward. */
enum { GSTEX_GT_F32 = 0, GSTEX_GT_U8 = 1 };       /* U8: value = (float)v / 255.0f (a true division) */
enum { GSTEX_MASK_F32 = 0, GSTEX_MASK_BOOL = 1 }; /* BOOL: one byte per pixel, m = v != 0 ? 1.0f : 0.0f */
typedef struct gstex_loss_target {
    const void* gt;      /* H*W*gt_channels, row-major, channel last */
    const void* mask;    /* nullable = no mask; H*W */
    int32_t gt_dtype;    /* GSTEX_GT_* */
    int32_t gt_channels; /* 3, or 4: straight alpha in channel 3, composited on `background` */
    int32_t mask_dtype;  /* GSTEX_MASK_* (ignored when mask is NULL) */
    int32_t reserved;    /* must be 0 */
} gstex_loss_target;
size_t gstex_loss_target_workspace_size(int32_t H, int32_t W);
int gstex_loss_target_fwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex, const float* alpha,
                          const float* background, const gstex_loss_target* target, const float* window,
                          float ssim_lambda, float* rgb_out, float* gt_out, float* terms_out, void* workspace,
                          size_t workspace_bytes, void* stream);
int gstex_loss_target_bwd(int32_t H, int32_t W, int32_t C, const float* img, const float* tex, const float* alpha,
                          const float* background, const gstex_loss_target* target, const float* window,
                          float ssim_lambda, const float* grad_loss, float* d_img, float* d_tex, float* d_alpha,
                          void* workspace, size_t workspace_bytes, void* stream);

/* One view's evaluation metrics by the reference's protocol -- added within ABI 19 (additive).
 * get_image_metrics_and_images (gstex.py:1337-1403): the render is quantised to uint8 (:1379-1381) before PSNR and
 * SSIM are taken against the composited target; forward only (no gradient maps, no backward).
 * Each line is one individually rounded fp32 operation:
 *   rgb_c = as gstex_loss_fwd (outputs["rgb"], clamped)
 *   q_c   = (uint8)(255.0f * rgb_c)                  (truncation, as (255.0 * x).to(torch.uint8))
 *   y_c   = (float)q_c * (1.0f / 255.0f)             (as torch's device kernel evaluates .to(float32) / 255.0)
 *   gt_c  = as gstex_loss_target_fwd: the stored value (F32) or (float)v / 255.0f (U8); with four channels
 *           a * g_c + (1 - a) * background_c.  No mask: the reference's evaluation applies none.
 *   MSE     = mean (y_c - gt_c)^2
 *   SSIM    = SSIM(X = gt, Y = y) as gstex_loss_fwd (window, constants, valid filtering, fixed-order reduction)
 *   MSE_raw = mean (rgb_c - gt_c)^2                  (the unquantised value of get_metrics_dict)
 *   metrics_out (device float[4]) = {PSNR = -10 log10(MSE) (+inf for MSE = 0), SSIM, MSE, MSE_raw}
 * Optional outputs, each nullable: rgb_out (H*W*3 floats, rgb, unquantised), rgb_u8_out (H*W*3 bytes, q: the bytes
 * the reference writes to its PNGs, (val * 255).byte()), gt_out (H*W*3 floats, gt).
 * The target is the gstex_loss_target of gstex_loss_target_fwd with the same alignment rules; a non-NULL mask is
 * rejected, `reserved` must be 0.  The workspace is gstex_eval_metrics_workspace_size bytes (0 when H or W <= 10):
 * three floats per forward workgroup (ceil(W / 16) * ceil(H / 16) * 3 of them), nothing else. */
size_t gstex_eval_metrics_workspace_size(int32_t H, int32_t W);
int gstex_eval_metrics(int32_t H, int32_t W, int32_t C, const float* img, const float* tex, const float* alpha,
                       const float* background, const gstex_loss_target* target, const float* window,
                       float* rgb_out, uint8_t* rgb_u8_out, float* gt_out, float* metrics_out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- optimizer (train-step support) ----------------------------------- */
/* One launch of torch.optim.Adam (no weight decay, no amsgrad) over up to GSTEX_ADAM_MAX_TENSORS
 * fp32 tensors.  Per tensor the host supplies step_size = lr / (1 - beta1^t) and
 * bias_correction2_sqrt = sqrt(1 - beta2^t) for that tensor's own step t.  Updates param,
 * exp_avg and exp_avg_sq in place. */
#define GSTEX_ADAM_MAX_TENSORS 16
typedef struct gstex_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float step_size;
    float bias_correction2_sqrt;
} gstex_adam_tensor;
/* flags (0 = the reference's update; unknown bits are rejected): GSTEX_ADAM_ZERO_GRAD also writes zeros over each
 * gradient after reading it (so the next backward can accumulate into the same buffer without a separate fill; the
 * update may then run on a side stream, overlapped with the next step's preprocessing).  Not in the reference
 * (torch.optim.Adam + zero_grad). */
#define GSTEX_ADAM_ZERO_GRAD 1
/* flags bits 8..23: cap on the launch's workgroups (0 = one per 1024 elements), each looping over the chunks; a
 * capped grid (e.g. one workgroup per CU) still streams at near full HBM bandwidth while leaving most of every CU's
 * wave slots to kernels of another stream.  GSTEX_ADAM_GRID(n) builds the field. */
#define GSTEX_ADAM_GRID_SHIFT 8
#define GSTEX_ADAM_GRID(n) (((n) & 0xFFFF) << GSTEX_ADAM_GRID_SHIFT)
/* grad_scale in (0, 1] (ABI 7; 1 = none): every gradient is read as grad * grad_scale -- a data-parallel
 * step passes 1 / world_size and skips the separate averaging pass over the all-reduced gradient buffer (the same
 * fp32 product, so the update is bit-identical).  Replaces, with GStex's GradSync, the 1 / world averaging of the
 * reference's DDP (pipelines/base_pipeline.py:281-283).
 * skip (ABI 13; a device float, nullable = never): read first, and nothing is updated when it is
 * non-zero: the pair-capacity guard's step flag (gstex_scan_offsets with a guard), all-reduced with the gradients in
 * data-parallel training so that every rank skips the same steps. */
int gstex_adam_step(int32_t n_tensors, const gstex_adam_tensor* tensors, double beta1, double beta2,
                    double eps, int32_t flags, float grad_scale, const float* skip, void* stream);

/* ---- training-step prologue (ABI 17; not in the reference) ------------------------------------------------------
 * One host call for the launches a photometric training render makes before its raster forward: the outputs of
 * gstex_activate_fwd, gstex_preprocess (the camera without c2w), gstex_sh_rest_fwd and the guarded gstex_scan_offsets
 * -- bit-identical, computed by one per-splat kernel (the same device functions on the same values) and a one-launch
 * scan -- then gstex_raster_setup (glob_scale 1) and the capped gstex_bin_sort as called per op (gstex_amd.fused: the
 * trainer's render without ~0.2 ms of per-launch host overhead, which a step that starts on an idle device waits for,
 * and four launches fewer).  All pointers are device pointers; the buffers are sized as the per-op entry points
 * require (block = 16), scan_workspace as gstex_train_prologue_scan_bytes(n). */
typedef struct gstex_train_prologue_args {
    int32_t n;
    int32_t sh_degree;
    int32_t n_rest;
    int32_t map_cols;
    int64_t capacity;
    gstex_camera cam;
    gstex_pair_guard guard;
    const float* means;
    const float* quats;
    const float* log_scales;
    const float* opac_logits;
    const float* mappings;
    const float* campos;
    const float* features_rest;
    const int32_t* texture_dims;
    float* quats_n;
    float* scales;
    float* opacities;
    float* uv0;
    float* umap;
    float* vmap;
    float* viewdirs;
    float* depths;
    float* centers;
    float* extents;
    int32_t* num_tiles_hit;
    float* rgbs;
    int32_t* offsets;
    void* scan_workspace;
    size_t scan_workspace_bytes;
    float* records;
    int32_t* tile_ranges;
    int32_t* sorted_ids;
    int32_t* sorted_slots;
    int32_t* tile_order;
    void* bin_workspace;
    size_t bin_workspace_bytes;
    void* raster_aux;        /* nullable: the raster forward's aux buffer (gstex_raster_aux_bytes(capacity, n_tiles,
                                raster_channels)), whose accumulated span the prologue zeroes -- set
                                aux_zeroed in the args of the forward that follows */
    size_t raster_aux_bytes;
    int32_t raster_channels;
    double* hp_records;      /* nullable (ABI 18): gstex_raster_setup's near-edge-on fp64 rows, double[n][12] */
} gstex_train_prologue_args;
int gstex_train_prologue(const gstex_train_prologue_args* args, void* stream);
/* Bytes of scan_workspace gstex_train_prologue needs for n splats (>= gstex_scan_workspace_size(n): the fused
 * preprocessing kernel leaves one tile-count sum per 128 splats there for the one-launch offsets scan). */
size_t gstex_train_prologue_scan_bytes(int32_t n);

/* The photometric training render's backward after gstex_raster_bwd (fast mode: partials = the zeroed (n, 24)
 * per-splat accumulator rows it added into), in one call (ABI 17; gstex_amd.fused): gstex_raster_setup_bwd
 * (fold_aabb, glob_scale 1, the camera with c2w), then gstex_activate_bwd and gstex_sh_rest_bwd on its outputs -- one
 * kernel, the same device functions on the same values (bit-identical), when the SH rows fit its LDS staging.  v_* are the
 * parameter gradients (written, not accumulated); v_*_act and v_centers / v_uv0 are scratch of n rows each (the
 * activated parameters' gradients, as the per-op calls write them). */
typedef struct gstex_train_epilogue_args {
    int32_t n;
    int32_t sh_degree;
    int32_t n_rest;
    gstex_camera cam;
    const float* means;
    const float* scales;     /* activated (gstex_activate_fwd) */
    const float* quats_n;    /* normalised */
    const float* quats;      /* raw parameter */
    const float* log_scales;
    const float* opacities;  /* activated */
    const float* umap;
    const float* vmap;
    const float* viewdirs;
    const int32_t* num_tiles_hit;
    const int32_t* offsets;
    float* partials;
    float* v_means;
    float* v_quats;
    float* v_log_scales;
    float* v_opac_logits;
    float* v_features_rest;
    float* v_scales_act;
    float* v_quats_n;
    float* v_rgbs;
    float* v_opacities_act;
    float* v_centers;
    float* v_uv0;
} gstex_train_epilogue_args;
int gstex_train_epilogue(const gstex_train_epilogue_args* args, void* stream);

/* ---- adaptive density control -- added within ABI 19 (additive); not in the reference, which disables it ----------
 * Clone, split and prune of one-texel splats while training (3DGS section 5.2 as 2DGS uses it; DESIGN.md "Density
 * control").  Every value below is computed by individually rounded fp32 + - * / sqrt in the order DESIGN.md states,
 * and every decision compares against thresholds the host formed, so gstex_amd.density's eager twins reproduce the
 * three entry points bit for bit.
 *
 * gstex_density_accum: one launch per training step, after the backward.  For every splat with num_tiles_hit > 0:
 * grad_sum += |dL/d(NDC centre)| (from v_means = dL/dmeans, cam->viewmat, fx, fy, H, W), count += 1, max_extent =
 * max(max_extent, extents[i][0], extents[i][1]).  num_tiles_hit / extents: the step's render's (gstex_preprocess or
 * gstex_train_prologue outputs).  skip (nullable): the step's pair-guard flag; non-zero makes the launch a no-op on
 * the device, like gstex_adam_step's skip.  Only cam's viewmat, fx, fy, H and W are read. */
int gstex_density_accum(int32_t n, const float* means, const float* v_means, const gstex_camera* cam,
                        const int32_t* num_tiles_hit, const float* extents, const float* skip,
                        float* grad_sum, float* count, float* max_extent, void* stream);

/* kind[i] written by gstex_density_plan; rows[i] = 1 (KEEP), 2 (CLONE: the splat then its copy; SPLIT: two children
 * and no parent) or 0 (PRUNE). */
#define GSTEX_DENSITY_KEEP 0
#define GSTEX_DENSITY_CLONE 1
#define GSTEX_DENSITY_SPLIT 2
#define GSTEX_DENSITY_PRUNE 3
/* With m = max(log_scales[i][0], log_scales[i][1]); hot = count > 0 && grad_sum >= grad_threshold * count (false for
 * every splat when prune_only); big = m > log_big; faint = opac_logits[i] < logit_faint.  First match wins:
 *   faint -> PRUNE;  hot && big -> SPLIT, or PRUNE when size_prune && m - log_split > log_world;
 *   size_prune && (max_extent > max_screen_px || m > log_world) -> PRUNE;  hot -> CLONE;  otherwise KEEP.
 * The thresholds are fp32 values the host formed: log_big = log(percent_dense * extent), logit_faint =
 * logit(min_opacity), log_world = log(0.1 * extent), log_split = log(1.6); all must be finite. */
typedef struct gstex_density_plan_args {
    int32_t n;
    int32_t size_prune;
    int32_t prune_only;
    float grad_threshold;
    float log_big;
    float logit_faint;
    float max_screen_px;
    float log_world;
    float log_split;
    const float* log_scales;  /* (n, 3) */
    const float* opac_logits; /* (n) */
    const float* grad_sum;
    const float* count;
    const float* max_extent;
    int32_t* rows;
    int32_t* kind;
} gstex_density_plan_args;
int gstex_density_plan(const gstex_density_plan_args* args, void* stream);

/* One per-splat tensor of gstex_density_apply: src (n, width) scattered into dst (n_new, width), splat i's rows at
 * offsets[i] (the exclusive scan of rows: gstex_scan_offsets), in source order.  role COPY: every row is the source
 * row.  MOMENT (an Adam moment): a KEEP row and a CLONE's first row are the source row, a CLONE's second row and both
 * SPLIT children are zero.  MEANS (width 3): as COPY, but SPLIT child k of splat i gets, per component c,
 * mean[c] + ((R[c][0] * (s_u * z_k0)) + (R[c][1] * (s_v * z_k1))) with s = scales[i] (activated), R the rotation of
 * quats_n[i] and z = noise[i] (2, 2).  LOG_SCALES (width >= 2): as COPY, but the first two columns of SPLIT children
 * are log_s - log_split. */
#define GSTEX_DENSITY_ROLE_COPY 0
#define GSTEX_DENSITY_ROLE_MOMENT 1
#define GSTEX_DENSITY_ROLE_MEANS 2
#define GSTEX_DENSITY_ROLE_LOG_SCALES 3
#define GSTEX_DENSITY_MAX_TENSORS 24
typedef struct gstex_density_tensor {
    const float* src;
    float* dst;
    int32_t width; /* floats per splat row; 0 = skipped */
    int32_t role;
} gstex_density_tensor;
typedef struct gstex_density_apply_args {
    int32_t n;
    int32_t n_tensors;
    int64_t n_new;          /* offsets[n] as the host read it: rows of every dst; nothing is written past them */
    float log_split;
    const int32_t* rows;
    const int32_t* kind;
    const int32_t* offsets;
    const float* scales;    /* (n, 3) activated, gstex_activate_fwd; needed by a MEANS tensor */
    const float* quats_n;   /* (n, 4) normalised, gstex_activate_fwd; needed by a MEANS tensor */
    const float* noise;     /* (n, 2, 2); needed by a MEANS tensor */
    const gstex_density_tensor* tensors; /* HOST array of n_tensors entries */
} gstex_density_apply_args;
int gstex_density_apply(const gstex_density_apply_args* args, void* stream);

/* ---- mesh extraction: TSDF fusion and marching tetrahedra -- added within ABI 19 (additive); not in the reference,
 * whose lineage leaves it to Open3D (DESIGN.md "Mesh extraction") --------------------------------------------------
 * The volume is a dense grid (nz, ny, nx), x fastest: sample (i, j, k) sits at origin + voxel_size * (i, j, k) and has
 * the linear index v = (k * ny + j) * nx + i.  Caller-owned DEVICE arrays: tsdf[n_vox], weight[n_vox] and, nullable,
 * color[3][n_vox] (three planes); a fresh volume is all zeros.  Every dim must be >= 2 (INVALID_ARG) and 7 * n_vox
 * below 2^31 (UNSUPPORTED: a vertex is keyed by 7 * v + edge class).  Every value below is computed by individually
 * rounded fp32 + - * / in the order DESIGN.md states, so gstex_amd.mesh's eager twins reproduce the entry points bit
 * for bit. */
typedef struct gstex_tsdf_volume {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel_size;
    float* tsdf;
    float* weight;
    float* color; /* nullable */
} gstex_tsdf_volume;

#define GSTEX_TSDF_MAX_VIEWS 8
typedef struct gstex_tsdf_view {
    gstex_camera cam;   /* viewmat, fx, fy, cx, cy, H, W are read */
    const float* depth; /* (H, W): the raster's un-normalised depth, sum of w z */
    const float* alpha; /* (H, W) */
    const float* rgb;   /* (H, W, 3); nullable when the volume has no colour */
} gstex_tsdf_view;
/* gstex_tsdf_integrate: ONE launch fuses n_views (1..GSTEX_TSDF_MAX_VIEWS) views into the volume, one thread per
 * voxel; the voxel's (tsdf, weight, colour) stays in registers across the views, in view order, and is stored once,
 * and only if some view changed it.  Per view, with p the voxel's world position and (x, y, z) = viewmat p: skipped
 * unless z > near_z; u = fx * (x / z) + cx, v = fy * (y / z) + cy; skipped unless 0 <= u < W and 0 <= v < H; pixel
 * (r, c) = ((int)v, (int)u); a = alpha[r][c], skipped unless a >= alpha_min; d = depth[r][c] / a, skipped unless
 * d > 0 and (depth_trunc == 0 or d <= depth_trunc); s = d - z, skipped if s < -sdf_trunc; t = min(1, s / sdf_trunc);
 * tsdf = (tsdf * w + t) / (w + 1), colour alike, w = w + 1.  sdf_trunc, alpha_min and near_z must be > 0,
 * depth_trunc >= 0 (0 = off). */
typedef struct gstex_tsdf_integrate_args {
    gstex_tsdf_volume vol;
    int32_t n_views;
    float sdf_trunc;
    float alpha_min;
    float depth_trunc;
    float near_z;
    const gstex_tsdf_view* views; /* HOST array of n_views entries */
} gstex_tsdf_integrate_args;
int gstex_tsdf_integrate(const gstex_tsdf_integrate_args* args, void* stream);

/* Marching tetrahedra on the volume.  The cell with lower corner (i, j, k) (i < nx - 1, ...) is split into the six
 * Kuhn tetrahedra; a tetrahedron emits only if its four corners have weight > 0, a corner is inside iff tsdf < 0, and
 * a vertex lies on every edge whose ends differ: owned by the edge's lower corner A (upper corner B, B - A one of the
 * seven classes (1,0,0) (0,1,0) (0,0,1) (1,1,0) (0,1,1) (1,0,1) (1,1,1)), at pA + t * (pB - pA), t = tA / (tA - tB).
 * table: DEVICE int32[GSTEX_MESH_TABLE_WORDS], made by gstex_amd.mesh (the twin reads the same words): word
 * [tet * 16 + case] (case = sum of inside(corner k) << k) holds the triangle count in bits 24..25 and, for slot
 * s = 3 * triangle + index, the edge's two tetrahedron corners in bits 4s..4s+1 (lower) and 4s+2..4s+3 (upper); word
 * [96 + tet] holds the tetrahedron's corner k as dx | dy << 1 | dz << 2 in bits 3k..3k+2.
 *   gstex_mesh_extract_mark  edge_mask[v] = the classes of v's edges that carry a vertex (zeroed here first),
 *                            then vertex_count[v] = their number and face_count[v] = the faces of cell v (0 for
 *                            the voxels of the last row, column and slab, which are no cell's lower corner);
 *   gstex_scan_offsets over vertex_count and face_count (the caller), ONE read-back of the two totals;
 *   gstex_mesh_extract_emit  vertices (n_vertices, 3), nullable colors (n_vertices, 3) and faces (n_faces, 3):
 *                            vertices ascend in 7 * v(owner) + class, faces in (cell, tetrahedron, triangle), each
 *                            face's indices in the table's order.  Nothing is written past n_vertices / n_faces rows.
 * All work arrays are DEVICE int32 of n_vox (counts, mask) or n_vox + 1 (offsets) entries. */
#define GSTEX_MESH_TABLE_WORDS 102
typedef struct gstex_mesh_extract_args {
    gstex_tsdf_volume vol;
    const int32_t* table;
    int32_t* edge_mask;
    int32_t* vertex_count;
    int32_t* face_count;
    const int32_t* vertex_offsets; /* emit only */
    const int32_t* face_offsets;   /* emit only */
    int64_t n_vertices;            /* emit only: rows of vertices / colors */
    int64_t n_faces;               /* emit only: rows of faces */
    float* vertices;
    float* colors; /* nullable; needs vol.color */
    int32_t* faces;
} gstex_mesh_extract_args;
int gstex_mesh_extract_mark(const gstex_mesh_extract_args* args, void* stream);
int gstex_mesh_extract_emit(const gstex_mesh_extract_args* args, void* stream);

/* ---- mesh scoring: grid nearest neighbours and a mesh surface sampler -- added within ABI 19 (additive); not in the
 * reference (DESIGN.md "Mesh scoring and nearest neighbours") ----------------------------------------------------------
 * A uniform grid over a 3D point set.  origin is the component-wise minimum of the points, and the cell of p is, per
 * axis, (int)((p - origin) / cell_size) (one rounded subtraction, one rounded division) clamped to [0, n_axis - 1];
 * the linear cell index is (cz * ny + cy) * nx + cx.  For an exact query the dims must cover the points (no point
 * clamped): n_axis = (int)((max - origin) / cell_size) + 1 by the same two operations.  Every dim must be in
 * [1, GSTEX_NN_MAX_AXIS_CELLS] and nx * ny * nz at most GSTEX_NN_MAX_CELLS (UNSUPPORTED beyond either), point counts
 * below 2^31.  Every value is computed by individually rounded fp32 operations in the order DESIGN.md states. */
#define GSTEX_NN_MAX_CELLS (1 << 26)
#define GSTEX_NN_MAX_AXIS_CELLS 4096
#define GSTEX_NN_MAX_K 8
typedef struct gstex_nn_grid {
    float origin[3];
    float cell_size;
    int32_t nx, ny, nz;
} gstex_nn_grid;
/* Build: gstex_nn_grid_count zeroes cell_count[n_cells] and adds one per point (integer atomics); the caller scans it
 * with gstex_scan_offsets into cell_start[n_cells + 1]; gstex_nn_grid_place zeroes cursor[n_cells] and writes each
 * point into its cell's segment as one 16-byte record (x, y, z, the point's index as int32 bits): records (n, 4),
 * 16-byte aligned.  The order inside a cell is unspecified.  points: DEVICE (n, 3) fp32. */
int gstex_nn_grid_count(const gstex_nn_grid* grid, int64_t n, const float* points, int32_t* cell_count, void* stream);
int gstex_nn_grid_place(const gstex_nn_grid* grid, int64_t n, const float* points, const int32_t* cell_start,
                        int32_t* cursor, float* records, void* stream);
/* gstex_nn_query: for each query the k (1..GSTEX_NN_MAX_K) nearest points, exactly as brute force over all points
 * gives them: d2 = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x, ascending, ties to the lower point index; missing
 * neighbours are d2 = +inf, index = -1.  queries are records too, (n_queries, 4): (x, y, z, row); the results of a
 * query go to row `row` of d2 (n_queries, k) and index (n_queries, k), and the queries are best issued in the order of
 * their own grid cells (gstex_nn_grid_count / _place on them).  exclude_self != 0 skips the point whose index equals
 * the query's row.  max_radius (>= 0, +inf for none): points with d2 > max_radius * max_radius do not count.  One
 * thread per query walks Chebyshev rings of cells around the query's unclamped cell, intersected with the grid, until
 * ((float)r * cell_size) * (1 - 2^-10), squared, reaches min(k-th best d2, max_radius^2) (r >= 1) or the ring has
 * left the grid on every side.  No read-back. */
typedef struct gstex_nn_query_args {
    gstex_nn_grid grid;
    int64_t n_points;
    const int32_t* cell_start; /* (n_cells + 1) */
    const float* records;      /* (n_points, 4) */
    int64_t n_queries;
    const float* queries;      /* (n_queries, 4) */
    int32_t k;
    int32_t exclude_self;
    float max_radius;
    float* d2;      /* (n_queries, k) */
    int32_t* index; /* (n_queries, k) */
} gstex_nn_query_args;
int gstex_nn_query(const gstex_nn_query_args* args, void* stream);

/* A deterministic area sampler of a triangle mesh.  Face (a, b, c) with longest edge L gets n = max(1, ceil(L /
 * spacing)) and is split into n^2 congruent sub-triangles with one sample at each centroid: upright (i, j),
 * i + j <= n - 1, at barycentric u = (i + 1/3) / n of b and v = (j + 1/3) / n of c; inverted (i, j), i + j <= n - 2, at
 * ((i + 2/3) / n, (j + 2/3) / n); position (a + u * (b - a)) + v * (c - a) per component, weight area / n^2.  Order:
 * ascending face, then i, then j, upright before inverted.
 *   gstex_mesh_sample_mark  count[f] = n^2 (0 for a face with n > GSTEX_SAMPLE_MAX_N or an index outside the
 *                           vertices) and stats (zeroed here first): int32[4] = the 64-bit sum of n^2 over the valid
 *                           faces (low word, high word), the largest n (capped at 2^30), the number of faces with an
 *                           index outside [0, n_vertices);
 *   gstex_scan_offsets over count (the caller), ONE read-back of stats;
 *   gstex_mesh_sample_emit  samples (n_samples, 3), weights (n_samples), face_of (n_samples); nothing is written past
 *                           n_samples rows. */
#define GSTEX_SAMPLE_MAX_N 256
typedef struct gstex_mesh_sample_args {
    int64_t n_vertices;
    int64_t n_faces;
    const float* vertices; /* (n_vertices, 3) */
    const int32_t* faces;  /* (n_faces, 3) */
    float spacing;
    int32_t* count;         /* (n_faces); mark */
    int32_t* stats;         /* int32[4], 8-byte aligned; mark */
    const int32_t* offsets; /* (n_faces + 1); emit only */
    int64_t n_samples;      /* emit only: rows of the outputs */
    float* samples;
    float* weights;
    int32_t* face_of;
} gstex_mesh_sample_args;
int gstex_mesh_sample_mark(const gstex_mesh_sample_args* args, void* stream);
int gstex_mesh_sample_emit(const gstex_mesh_sample_args* args, void* stream);

/* ---- clustering the splats: DBSCAN under the squared 2-Wasserstein distance -- added within ABI 19 (additive); the
 * reference's dbscan_clustering/dbscan_ballquery.py (DESIGN.md "Clustering the splats") --------------------------------
 * A splat is a flat Gaussian: mean mu, unit quaternion (w, x, y, z) with rotation R, activated in-plane scales s0, s1
 * (the first two columns of scales (n, scale_cols >= 2); the third scale counts as zero).  Its shape is
 *   a = s0 R[:, 0] = s0 (1 - 2 (y y + z z), 2 (x y + w z), 2 (x z - w y)),
 *   b = s1 R[:, 1] = s1 (2 (x y - w z), 1 - 2 (x x + z z), 2 (y z + w x)),      T = s0 s0 + s1 s1,
 * and the distance of splats i and j is, every operation individually rounded in fp32 in this order,
 *   d2   = (dx dx + dy dy) + dz dz,  dx = mu_i.x - mu_j.x                                   (as gstex_nn_query)
 *   m00 = (a_i.x a_j.x + a_i.y a_j.y) + a_i.z a_j.z,  m01 = a_i . b_j,  m10 = b_i . a_j,  m11 = b_i . b_j  (same order)
 *   fro  = (m00 m00 + m11 m11) + (m01 m01 + m10 m10),   det = m00 m11 - m01 m10
 *   tr   = max((T_i + T_j) - 2 sqrtf(fro + 2 |det|), 0),   w2 = d2 + tr
 * which is the same for (i, j) and (j, i) bit for bit; w2 >= d2 holds in fp32, so the grid prunes on d2 <= eps.  j is a
 * neighbour of i iff j != i and w2 <= eps: eps is a threshold on the SQUARED distance, as in the reference.
 *   degree[i] = the number of neighbours; core: degree[i] >= min_pts (self not counted); clusters: the connected
 *   components of the cores; a cluster's id: 1 + the rank of its lowest core index among all clusters' lowest core
 *   indices (1..K); a splat that is no core takes the lowest id among its core neighbours, or -1 (noise).
 * Calls, on the grid of gstex_nn_grid_count / _place over the means (any cell size: the walk is gstex_nn_query's, with
 * eps in the place of max_radius^2):
 *   gstex_cluster_shapes   shapes (n, 8) = (a.xyz, T, b.xyz, 0) in the order of the grid's records, 16-byte aligned
 *   gstex_cluster_degree   degree[index] and parent[index] = index
 *   gstex_cluster_link     a core unites with every core neighbour of lower index: a lock-free union-find in parent
 *                          (find with path halving, the higher root hooked under the lower by compare-and-swap; parents
 *                          only ever decrease, so no walk can cycle and none waits for another lane)
 *   gstex_cluster_roots    parent[i] = its root; root_flag[i] = 1 for a core that is its own root, else 0
 *   gstex_scan_offsets over root_flag (the caller) -> offsets (n + 1); K = offsets[n], the ONE read-back
 *   gstex_cluster_assign   labels[i] in the caller's order
 * n == 0 is a no-op success; n >= 2^31, min_pts < 1, eps < 0 or not finite, null or misaligned pointers: INVALID_ARG. */
typedef struct gstex_cluster_args {
    gstex_nn_grid grid;
    int64_t n;
    const int32_t* cell_start; /* (n_cells + 1) */
    const float* records;      /* (n, 4) */
    const float* shapes;       /* (n, 8) */
    float eps;
    int32_t min_pts;
    int32_t* degree;        /* (n) */
    int32_t* parent;        /* (n) */
    const int32_t* offsets; /* (n + 1); assign only */
    int32_t* labels;        /* (n); assign only */
} gstex_cluster_args;
int gstex_cluster_shapes(int64_t n, const float* records, const float* scales, int32_t scale_cols, const float* quats,
                         float* shapes, void* stream);
int gstex_cluster_degree(const gstex_cluster_args* args, void* stream);
int gstex_cluster_link(const gstex_cluster_args* args, void* stream);
int gstex_cluster_roots(int64_t n, int32_t min_pts, const int32_t* degree, int32_t* parent, int32_t* root_flag,
                        void* stream);
int gstex_cluster_assign(const gstex_cluster_args* args, void* stream);
/* d2, tr and w2 (n_pairs each) of the pairs (n_pairs, 2) int32 of splat indices, n_pairs < 2^30, from the caller's own
 * arrays (means (n, 3), scales, quats (n, 4)); a pair with an index outside [0, n) gets NaN. */
int gstex_cluster_pair_w2(int64_t n, const float* means, const float* scales, int32_t scale_cols, const float* quats,
                          int64_t n_pairs, const int32_t* pairs, float* d2, float* tr, float* w2, void* stream);

/* ---- selecting splats: the jagged texel store compacted by a per-splat mask -- added within ABI 19 (additive); not in
 * the reference, whose clustering tool writes a new file (DESIGN.md "Selecting splats") -------------------------------
 * The texel store holds chart i's h_i * w_i texels of `channels` floats at rows [offset_i, offset_i + h_i * w_i), with
 * texture_dims (n, 3) int32 = (h, w, offset); blocks may lie in any order and the store may have spare rows past
 * n_texels.  Keeping the splats with keep[i] != 0, in their order:
 *   gstex_select_plan    rows[i] = keep ? 1 : 0, texels[i] = keep ? h * w : 0; *flag |= 1 when ANY row, kept or not, is
 *                        malformed: h < 0, w < 0, offset < 0, h * w > 2^31 - 1 or offset + h * w > n_texels (such a
 *                        row counts 0 texels).  The caller zeroes *flag before the call.
 *   gstex_scan_offsets over rows and over texels (the caller) -> row_off (n + 1), tex_off (n + 1); ONE read-back of
 *                        (n_new, T_new, flag) = (row_off[n], tex_off[n], *flag)
 *   gstex_select_dims    for a kept i, with j = row_off[i]: new_dims[j] = (h, w, tex_off[i]), src_off[j] = offset
 *   gstex_select_texels  for every pair k, kept splat j (new index), t < h_j * w_j and c < channels:
 *                          dst_k[(new_off_j + t) * channels + c] = src_k[(src_off_j + t) * channels + c]
 *                        with new_off_j = new_dims[j][2].  Every destination word below n_texels_new * channels is
 *                        written exactly once and none at or past it; no word at or past n_texels * channels is read.
 *                        The chart of destination texel t is the LAST j with new_off_j <= t, which passes over
 *                        zero-texel charts.  A texel that new_dims / src_off do not place inside the store (arrays that
 *                        are not a plan's) is left unwritten.  src == dst is refused.
 * Per-splat tensors go through gstex_density_apply with these rows, row_off as offsets and every kind KEEP.  No entry
 * point allocates or synchronises; n == 0 (plan, dims) and n_texels_new == 0 or n_tensors == 0 (texels) are no-op
 * successes.  Negative sizes, totals >= 2^31, channels outside [1, 8], n_tensors above the maximum, null or misaligned
 * pointers: INVALID_ARG. */
#define GSTEX_SELECT_MAX_TENSORS 4
typedef struct gstex_select_plan_args {
    int32_t n;
    int64_t n_texels;
    const uint8_t* keep;         /* (n) bytes, non-zero = keep */
    const int32_t* texture_dims; /* (n, 3) */
    int32_t* rows;               /* (n) */
    int32_t* texels;             /* (n) */
    int32_t* flag;               /* one word, zeroed by the caller */
} gstex_select_plan_args;
int gstex_select_plan(const gstex_select_plan_args* args, void* stream);

typedef struct gstex_select_dims_args {
    int32_t n;
    int32_t n_new; /* row_off[n] as the host read it: rows of new_dims and src_off; nothing is written past them */
    const uint8_t* keep;
    const int32_t* texture_dims;
    const int32_t* row_off; /* (n + 1) */
    const int32_t* tex_off; /* (n + 1) */
    int32_t* new_dims;      /* (n_new, 3) */
    int32_t* src_off;       /* (n_new) */
} gstex_select_dims_args;
int gstex_select_dims(const gstex_select_dims_args* args, void* stream);

typedef struct gstex_select_pair {
    const float* src; /* (>= n_texels, channels) */
    float* dst;       /* (>= n_texels_new, channels) */
} gstex_select_pair;
typedef struct gstex_select_texels_args {
    int32_t n_new;
    int32_t channels;
    int32_t n_tensors;
    int64_t n_texels_new; /* tex_off[n] as the host read it */
    int64_t n_texels;     /* rows of every src that may be read */
    const int32_t* new_dims;
    const int32_t* src_off;
    gstex_select_pair tensors[GSTEX_SELECT_MAX_TENSORS];
} gstex_select_texels_args;
int gstex_select_texels(const gstex_select_texels_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GSTEX_HIP_H */
