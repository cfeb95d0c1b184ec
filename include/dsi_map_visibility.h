/* The world map carved by free space: what a depth image says about the cells on its rays.  A filtered depth map states
 * where a surface is -- that is what the integrate calls take from it -- and that the space between the camera and that
 * surface is empty.  A cell that other views look straight through, at a surface behind it, is a floater: the
 * visibility-consistency test of depth-map fusion (Merrell et al. 2007).  The entry points here tally, per cell and over any
 * number of views, how often a view agreed with the cell, looked through it or saw a surface in front of it, and prune
 * by that tally.  DESIGN.md 7j "Visibility".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  The tally is a function of
 * the map and the list of observations alone, bit for bit whatever the table's size, the probing and the order of the
 * threads.  tests/map_visibility_reference.py restates everything here in numpy and Python ints. */
#ifndef DSI_MAP_VISIBILITY_H
#define DSI_MAP_VISIBILITY_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----
 * Double arithmetic, every operation rounded on its own, no FMA.  An OBSERVATION is a depth image -- depth float32
 * [height][width], row-major, and mask uint8 of the same shape or NULL --, its pinhole, its depth range, the pose T_v_w
 * (world -> view, as dsi_map_view_t's), a window and two tolerances.  Per occupied cell (every cell: there is no filter):
 *
 *   1. POINT.  p is the centroid exactly as dsi_map_extract returns it (float32), widened to double;
 *      X = ((r00 x + r01 y) + r02 z) + t0 and Y, Z alike (rule 2 of dsi_map_render).
 *   2. CLIPPED when X, Y or Z is not finite, or when Z >= min_depth && Z <= max_depth does not hold.
 *   3. PIXEL.  iu = floor(((fx * (X / Z)) + cx) + 0.5), iv alike.  The cell is OUTSIDE when the centre pixel is not in the
 *      image: 0 <= iu <= width - 1 && 0 <= iv <= height - 1, tested in double before anything becomes an integer (huge,
 *      infinite and NaN values fail).  A centre outside whose window reaches the image is still OUTSIDE.
 *   4. WINDOW.  The cell's pixels are (iu + dx, iv + dy), |dx|, |dy| <= window, each tested against the image on its own.
 *      A pixel is VALID iff mask is NULL or mask > 0, d = (double) depth is finite and min_depth <= d <= max_depth
 *      (dsx_map_integrate_depth's test).  The cell is UNSEEN when none of its pixels is valid.
 *   5. TOLERANCE.  tol = (rel_tol * Z) + abs_tol, lo = Z - tol, hi = Z + tol.  A valid pixel AGREES iff d >= lo && d <= hi,
 *      looks THROUGH the cell iff d > hi and sees a surface IN FRONT iff d < lo.
 *   6. VERDICT of the view on the cell: AGREE if any valid pixel agrees; else THROUGH if every valid pixel looks through it;
 *      else BEHIND.  This is conservative: at a depth edge one nearer pixel protects the cell.
 *   7. TALLY.  Three uint32 per slot, on the device in buffers that belong to the map: seen counts the views with a
 *      verdict, agree and through count their verdicts; behind is seen - agree - through.  Every slot is written by its
 *      own thread.  At most 2^32 - 1 views per tally: the next one is refused.
 *   8. INFO: exact integer counters of this view, n_cells = n_clipped + n_outside + n_unseen + n_agree + n_through +
 *      n_behind; beside them n_valid_pixels, the image's valid pixels, and views, the observations in the tally.
 *
 * LIFETIME.  The tally starts zeroed with the first observation after dsi_map_create, after dsx_map_visibility_clear and
 * after any change of the map: dsi_map_reset, every integrate call, a merge, an import, dsx_map_integrate_map and a prune
 * of any kind.  Until then observations accumulate; they may differ in size, camera and tolerances.  An observation
 * changes nothing else: the map's render, compare, classification, alignment step, labelling, self query and local-shape
 * pass stay valid.
 *
 * Bounds, judged before the map is looked at and before the GPU is touched: width, height, fx, fy, cx, cy, min_depth and
 * max_depth as dsi_map_view_t's; window is 0..3; abs_tol and rel_tol are finite and >= 0. */
typedef struct dsx_map_observation {
    int32_t width, height;        /* >= 1, width * height <= 2^26 */
    int32_t window;               /* 0..3: a cell is judged by the (2 window + 1)^2 pixels around its pixel */
    double fx, fy, cx, cy;        /* finite, fx and fy != 0 */
    double min_depth, max_depth;  /* finite, FLT_MIN <= min_depth < max_depth <= FLT_MAX */
    double abs_tol, rel_tol;      /* finite, >= 0 */
    double T_v_w[12];             /* world -> view, row-major [R | t] */
} dsx_map_observation_t;
typedef struct dsx_map_observe_info {
    uint64_t n_cells;  /* occupied cells; = the sum of the six below */
    uint64_t n_clipped, n_outside, n_unseen, n_agree, n_through, n_behind;
    uint64_t n_valid_pixels; /* of the image, by rule 4 */
    uint64_t views;          /* observations in the tally, this one included */
} dsx_map_observe_info_t;
typedef struct dsx_map_visibility_selection {
    uint32_t min_through;  /* >= 1 */
    uint32_t agree_weight; /* any */
    int32_t shrink;        /* 0 or 1; read by dsx_map_prune_visibility, only checked by the dry run */
} dsx_map_visibility_selection_t;
typedef struct dsx_map_visibility_select_info {
    uint64_t n_cells;   /* occupied cells before; = n_kept + n_removed */
    uint64_t n_kept;
    uint64_t n_removed; /* reason 1: carved */
    uint64_t capacity;  /* slots after the call */
} dsx_map_visibility_select_info_t;

/* One view from host arrays; the staging buffers belong to the map.  mask_host may be NULL, info may be NULL.
 * DSI_ERR_INVALID for NULL obs, a violated bound (judged first, with no map at hand), a NULL map, depth_host or a map whose
 * table overflowed earlier, and for the view after 2^32 - 1.  Synchronises. */
DSI_API int dsx_map_observe(dsi_map_t *map, const float *depth_host, const uint8_t *mask_host, const dsx_map_observation_t *obs,
                            dsx_map_observe_info_t *info);
/* The same of the filtered depth map and mask that the mapper's last dsi_mapper_get_depth_map_from_dsi /
 * dsi_mapper_filter_depth_map left on the device, read where they lie: bit for bit dsx_map_observe of the fetched maps.
 * The preconditions are dsi_map_integrate_mapper's: DSI_ERR_CONTEXT when map and mapper come from different contexts,
 * DSI_ERR_INVALID without a filtered depth map, for a plane-sharded mapper and unless obs->width, height are the
 * mapper's.  Synchronises. */
DSI_API int dsx_map_observe_mapper(dsi_map_t *map, dsi_mapper_t *mapper, const dsx_map_observation_t *obs, dsx_map_observe_info_t *info);
/* Zeroes the tally: the next observation is the first.  DSI_ERR_INVALID for a NULL map. */
DSI_API int dsx_map_visibility_clear(dsi_map_t *map);
/* The tally of every occupied cell, in the order of dsi_map_extract(1, 1); any output may be NULL.  dsi_map_extract's
 * capacity protocol: when capacity < *count nothing is written and DSI_ERR_INVALID comes back with *count set.  A non-NULL
 * reasons_host needs a dsx_map_visibility_select on this tally.  DSI_ERR_INVALID without a tally of the map as it stands (no
 * observation since the last change or clear).  Synchronises. */
DSI_API int dsx_map_visibility_fetch(dsi_map_t *map, uint64_t *keys_host, uint32_t *seen_host, uint32_t *agree_host, uint32_t *through_host,
                                     uint8_t *reasons_host, size_t capacity, size_t *count);
/* The dry run of the selection on the tally.  A cell's reason is 1 (carved) iff
 *     through >= min_through && (uint64) through > (uint64) agree_weight * agree,
 * otherwise 0 (kept).  Decides every occupied cell and counts; the map and everything derived from it stay as they are, and
 * further observations invalidate the reasons, not the tally.  The per-slot reasons stay on the device for
 * dsx_map_visibility_fetch.  info may be NULL.  DSI_ERR_INVALID for NULL sel, a violated bound, a NULL map and a map without
 * a tally.  Synchronises. */
DSI_API int dsx_map_visibility_select(dsi_map_t *map, const dsx_map_visibility_selection_t *sel, dsx_map_visibility_select_info_t *info);
/* Selects, then rebuilds as dsx_map_prune_pca does: the kept cells move into a fresh zeroed table with all their state.
 * With shrink the new capacity is the smallest 2^k, k >= 8, with 4 * kept <= 3 * 2^k; without it the capacity stays.
 * calls, accepted, rejected and growths keep their values.  Invalidates everything derived from the map, this tally
 * included.  If the new table cannot be allocated the map is unchanged (DSI_ERR_HIP).  Errors as
 * dsx_map_visibility_select's.  Synchronises. */
DSI_API int dsx_map_prune_visibility(dsi_map_t *map, const dsx_map_visibility_selection_t *sel, dsx_map_visibility_select_info_t *info);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_VISIBILITY_H */
