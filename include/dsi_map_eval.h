/* The world map scored in 3-D: ground-truth depth images turned into a map, and map-to-map distances (accuracy,
 * completeness and F-score as multi-view stereo takes them -- the curves of the reference's
 * scripts/precision_completeness.py:43-92, in space instead of in the image).  DESIGN.md 7j "Scoring the map in 3-D".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handles (dsi_map_t, dsi_gt_t), return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  "Rules 1-6"
 * below are the world map's, stated in dsi_engine.h.  All arithmetic is double, every product and sum rounded on its own
 * (no FMA).  tests/map_eval_reference.py restates everything here in numpy. */
#ifndef DSI_MAP_EVAL_H
#define DSI_MAP_EVAL_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- depth images into a map ----
 * One integrate call (one `windows` stamp) of a depth image seen by a pinhole camera at T_w_c (camera -> world, 12
 * doubles, row-major [R | t]).  A pixel (u, v) of depth d is integrated iff
 *   - mask_host is NULL or mask > 0, and
 *   - d is finite and d >= min_depth && d <= max_depth (NaN fails, and so does the projector's 0 for "no value").
 * Integer pixel coordinates are pixel centres (dsi_mapper_get_pointcloud's convention, render rule 4).  The point is
 * float32: x = (float) ((((double) u - cx) / fx) * (double) d), y = (float) ((((double) v - cy) / fy) * (double) d),
 * z = d.  It then goes through rules 1-4 in the routine dsi_map_integrate's points go through: the call is, bit for bit,
 * dsi_map_integrate of that float32 point list.  *n_points (may be NULL): the pixels integrated; *n_rejected (may be
 * NULL): those of them rejected by rule 3.
 * DSI_ERR_INVALID, decided before the GPU is touched and before the map is looked at, unless width, height >= 1,
 * width * height <= 2^26, fx and fy finite and != 0, cx and cy finite, FLT_MIN <= min_depth < max_depth <= FLT_MAX
 * (dsi_map_view_t's bounds).  The table grows by the map's rule with the call's point count bounded by width * height
 * (no counting pass); a call that would need more than 2^27 slots by that bound returns DSI_ERR_INVALID and leaves the
 * map as it was.  Like every integrate call it invalidates the map's render and compare.  Synchronises. */
DSI_API int dsx_map_integrate_depth(dsi_map_t *map, const float *depth_host, const uint8_t *mask_host, int32_t width,
                                    int32_t height, double fx, double fy, double cx, double cy, double min_depth,
                                    double max_depth, const double T_w_c[12], uint64_t *n_points, uint64_t *n_rejected);
/* The same of the depth map the projector last made, where it lies on the device, at the projector's width and height
 * and without a mask: only the counts travel.  DSI_ERR_CONTEXT when the map and the projector were created from
 * different contexts. */
DSI_API int dsx_map_integrate_depth_gt(dsi_map_t *map, dsi_gt_t *gt, double fx, double fy, double cx, double cy,
                                       double min_depth, double max_depth, const double T_w_c[12], uint64_t *n_points,
                                       uint64_t *n_rejected);

/* ---- map-to-map distances ----
 * For every cell of `a` with n >= min_points_a && windows >= min_windows_a:
 *   1. p = its centroid exactly as dsi_map_extract returns it (rule 5, rounded to float32), widened to double;
 *   2. per axis c = floor(p / leaf_b) (the IEEE divide of rule 2); reach = (int) ceil(radius / leaf_b), computed once on
 *      the host;
 *   3. the candidates are the cells of `b` with n >= min_points_b && windows >= min_windows_b whose index is c + o,
 *      |o| <= reach per axis (at most 7^3 lookups; an index with |c + o| > 2^20 - 2 is skipped).  For each, q = its
 *      centroid by rule 5 as float32, widened, and d2 = ((dx dx) + dy dy) + dz dz; the minimum d2 is kept;
 *   4. d = sqrt(min d2), correctly rounded.  The cell is MATCHED iff a candidate exists and d <= radius, else UNMATCHED;
 *   5. matched: hist[min((int) floor(d / w), n_bins - 1)] += 1 with w = radius / n_bins, and
 *      sum_q += (uint64) floor((d / radius) * 2^32) -- the mean distance is sum_q * radius / 2^32 / n_matched;
 *   6. per cell dist = (float) d, +inf when unmatched, kept on the device in a buffer that belongs to `a`.
 * The distance is the nearest among the cells within `reach`: the true nearest neighbour within `radius` unless a
 * centroid's float32 rounding moved it across a face of its own cell.  Every effect is an integer atomic and the lookups
 * only read: the result is a function of the two maps (and the options) alone.  a == b is legal (every distance is 0),
 * the leaves may differ, either map may be empty. */
typedef struct dsx_map_compare_opts {
    uint32_t min_points_a, min_windows_a;  /* dsi_map_extract's filter on a */
    uint32_t min_points_b, min_windows_b;  /* and on b */
    double radius;                         /* finite, > 0, with 1 <= ceil(radius / leaf_b) <= 3 */
    int32_t n_bins;                        /* 1..4096; radius / n_bins must not underflow to 0 */
} dsx_map_compare_opts_t;
typedef struct dsx_map_compare_info {
    uint64_t n_cells;      /* cells of a that passed its filter; = n_matched + n_unmatched */
    uint64_t n_matched, n_unmatched;
    uint64_t sum_q;        /* rule 5 */
    int32_t reach;
} dsx_map_compare_info_t;
/* hist_host: n_bins counts, may be NULL; info may be NULL.  DSI_ERR_INVALID for a NULL map or opts or a violated bound
 * (radius and n_bins are judged before the maps are looked at), DSI_ERR_CONTEXT when the maps were created from
 * different contexts -- all decided before the GPU is touched.  Synchronises. */
DSI_API int dsx_map_compare(dsi_map_t *a, dsi_map_t *b, const dsx_map_compare_opts_t *opts, uint64_t *hist_host,
                            dsx_map_compare_info_t *info);
/* (key, dist) of the last compare in which `a` was the first map, for the cells of that compare's filter on a, in
 * dsi_map_extract's order; either output may be NULL.  dsi_map_extract's capacity protocol: when capacity < *n nothing
 * is written, *n is the size needed and the call returns DSI_ERR_INVALID.  DSI_ERR_INVALID before the first compare and
 * after dsi_map_reset or any integrate call on a.  A change to b after the compare does NOT invalidate it: the result
 * belongs to the maps as they stood when they were compared.  Synchronises. */
DSI_API int dsx_map_compare_fetch(dsi_map_t *a, float *dist_host, uint64_t *keys_host, size_t capacity, size_t *n);

#ifdef __cplusplus
}
#endif
#endif /* DSI_MAP_EVAL_H */
