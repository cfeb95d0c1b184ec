/* The world map's k nearest cells: which cells lie near a point of the caller's, and how far; and on top of that query
 * PCL's StatisticalOutlierRemoval for the map itself -- a cell leaves when the mean distance to its k nearest neighbours
 * is large against the map's own mean and deviation of that quantity.  DESIGN.md 7j "Neighbours and statistical outliers".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  The result is a function of
 * the map and the options alone, bit for bit whatever the table's size, the probing and the order of the threads.
 * tests/map_knn_reference.py restates everything here in numpy. */
#ifndef DSI_MAP_KNN_H
#define DSI_MAP_KNN_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----
 * "Rules 1-6" are the map's in dsi_engine.h.  Double arithmetic, every operation rounded on its own, no FMA.
 *
 * NEIGHBOURS of a query point p (three doubles; a float32 query is widened):
 *   1. per axis c = floor(p / leaf) (the IEEE divide of rule 2);
 *   2. reach = (int) ceil(radius / leaf), computed once on the host, 1 <= reach <= 3;
 *   3. the candidates are the cells with n >= min_points && windows >= min_windows at index c + o, |o| <= reach per axis;
 *      an index with |c + o| > 2^20 - 2 is skipped, tested in double as dsx_map_compare does: a NaN or huge c has no
 *      candidates;
 *   4. per candidate: q = its centroid by rule 5 as float32, widened; d2 = ((dx dx) + dy dy) + dz dz; d = sqrt(d2),
 *      correctly rounded; it is ADMITTED iff d <= radius;
 *   5. the admitted candidates are ordered by (d2, key) ascending -- a total order, so the scan order cannot matter --;
 *      the first k are the result, found = min(k, admitted).
 * As in dsx_map_compare this is the true k-NN within radius with one exception: a cell's centroid is rounded to float32,
 * and the rounding may have moved it across a face of its own cell (to the face itself: by at most one float32 ulp of the
 * coordinate).  The box of step 3 is laid around cell INDICES, so such a centroid, when it lies within radius of p by a
 * margin smaller than that ulp in a cell just outside the box, is not seen.
 *
 * SELF QUERY (dsx_map_knn): every cell that passes the filter is a query, p = its own extracted centroid.  The cell itself
 * is excluded BY KEY, not by offset 0: its rounded centroid may floor into a neighbour's index.  With d_1 .. d_found the
 * distances in rank order:
 *      m = (((d_1 + d_2) + ...) + d_found) / found          q = (uint64) floor((m / radius) * 2^30)   (q <= 2^30)
 * A cell is SCORED iff found >= min_found, otherwise ISOLATED.  Over the scored cells these exact integers are reduced:
 * N, sum_q and sum_q2 = sum q^2 (128 bits, two 64-bit words, low then high).
 *
 * THRESHOLD (dsx_map_knn_threshold; host only):
 *      V     = N * sum_q2 - sum_q^2                                     (an exact integer >= 0, below 2^115)
 *      mu    = (double) sum_q / (double) N
 *      sigma = N >= 2 ? sqrt((double) V / ((double) N * (double) (N - 1))) : 0        (PCL's sample deviation)
 *      T     = mu + std_mult * sigma
 *      T_q   = T >= 2^30 ? 2^30 : T < 0 ? 0 : (uint64) floor(T)
 * The integer-to-double conversions round to nearest even.  N == 0 gives mu = sigma = 0 and T_q = 2^30.  (T < 0 needs
 * std_mult < 0, which switches criterion 3 off; the 0 only keeps the conversion defined.)
 *
 * SELECTION (dsx_map_knn_select, dsx_map_prune_knn).  A cell's reason is the FIRST that holds, or 0 (kept):
 *   1. the cell fails the query's filter;
 *   2. found < min_found (isolated);
 *   3. std_mult >= 0 and q > T_q.
 * Bounds of the options, judged before the map is looked at and before the GPU is touched: k is 1..16; min_found is 1..k;
 * radius is finite and > 0, and with the map at hand reach is 1..3; std_mult is finite (< 0 switches criterion 3 off);
 * shrink is 0 or 1. */
typedef struct dsx_map_knn_opts {
    uint32_t min_points, min_windows; /* the candidates' filter, and the self query's queries */
    int32_t k;                        /* 1..16 */
    int32_t min_found;                /* 1..k; read by the self query, only checked by dsx_map_knn_points */
    double radius;                    /* finite, > 0, at most three leaves */
} dsx_map_knn_opts_t;
typedef struct dsx_map_knn_info {
    uint64_t n_cells;     /* queries: the cells that pass the filter; = n_scored + n_isolated */
    uint64_t n_unqueried; /* occupied cells that the filter leaves out */
    uint64_t n_scored;    /* N */
    uint64_t n_isolated;
    uint64_t sum_q;
    uint64_t sum_q2[2];   /* low, high */
    int32_t reach;
} dsx_map_knn_info_t;
typedef struct dsx_map_knn_selection {
    double std_mult; /* finite; < 0: criterion 3 off */
    int32_t shrink;  /* 0 or 1; read by dsx_map_prune_knn, only checked by the dry run */
} dsx_map_knn_selection_t;
typedef struct dsx_map_knn_select_info {
    uint64_t n_cells;      /* occupied cells before; = n_kept + sum n_removed */
    uint64_t n_kept;
    uint64_t n_removed[3]; /* by the FIRST reason that holds, in the order above */
    uint64_t T_q;
    double mu, sigma;
    uint64_t capacity;     /* slots after the call */
} dsx_map_knn_select_info_t;

/* The neighbours of n float32 host points (stride_floats 3 or 4 floats apart, at most 2^27 per call: dsi_map_integrate's
 * convention).  keys_host [n][k]: the neighbours' keys in rank order, padded with 0; dist_host [n][k]: (float) d, padded
 * with +inf; found_host [n].  Any output may be NULL.  Reads the map only: its render, compare, alignment step,
 * classification, labelling and self query stay valid.  n == 0 and an empty map are legal; a non-finite query has
 * found = 0.  DSI_ERR_INVALID for NULL opts, a violated bound, a NULL map, NULL points with n > 0 and a map whose table
 * overflowed earlier.  Synchronises. */
DSI_API int dsx_map_knn_points(dsi_map_t *map, const float *xyz_host, size_t stride_floats, size_t n, const dsx_map_knn_opts_t *opts,
                               uint64_t *keys_host, float *dist_host, uint8_t *found_host);
/* The self query of the map as it stands.  Per slot found, q and (float) m stay on the device, in buffers that belong to
 * the map (allocated on first use, 9 bytes per slot, freed by dsi_map_destroy), until the map changes: dsi_map_reset, any
 * integrate call, a merge, an import or a prune of any kind invalidates it.  Changes nothing else.  info may be NULL.
 * Errors as dsx_map_knn_points'.  Synchronises. */
DSI_API int dsx_map_knn(dsi_map_t *map, const dsx_map_knn_opts_t *opts, dsx_map_knn_info_t *info);
/* The threshold above from the self query's moments: host only, no context needed; sum_q2 is two words, low then high.
 * Any output may be NULL.  DSI_ERR_INVALID for a NULL sum_q2, a std_mult that is not finite and moments that no self
 * query can return (N > 2^27, sum_q > N * 2^30, sum_q2 > N * 2^60 or V < 0). */
DSI_API int dsx_map_knn_threshold(uint64_t N, uint64_t sum_q, const uint64_t sum_q2[2], double std_mult, double *mu, double *sigma,
                                  uint64_t *T_q);
/* The dry run of the selection on the self query: decides every occupied cell and counts; the map and everything derived
 * from it stay as they are.  The per-slot reasons stay on the device for dsx_map_knn_fetch.  info may be NULL.
 * DSI_ERR_INVALID for NULL sel, a violated bound, a NULL map and a map without a valid self query.  Synchronises. */
DSI_API int dsx_map_knn_select(dsi_map_t *map, const dsx_map_knn_selection_t *sel, dsx_map_knn_select_info_t *info);
/* (key, found, (float) m, q, reason) of every query of the self query, in the order of dsi_map_extract under the query's
 * filter; any output may be NULL.  m is +inf and q is 0 where found is 0.  dsi_map_extract's capacity protocol: when
 * capacity < *count nothing is written and DSI_ERR_INVALID comes back with *count set.  A non-NULL reasons_host needs a
 * dsx_map_knn_select on this query.  DSI_ERR_INVALID without a valid self query.  Synchronises. */
DSI_API int dsx_map_knn_fetch(dsi_map_t *map, uint64_t *keys_host, uint8_t *found_host, float *mean_host, uint32_t *q_host,
                              uint8_t *reasons_host, size_t capacity, size_t *count);
/* Selects, then rebuilds as dsx_map_prune does: the kept cells move into a fresh zeroed table with all their state (n,
 * S[3], windows, stamp).  With shrink the new capacity is the smallest 2^k, k >= 8, with 4 * kept <= 3 * 2^k; without it
 * the capacity stays.  calls, accepted, rejected and growths keep their values.  Invalidates the map's render, compare,
 * alignment step, classification, labelling and self query.  If the new table cannot be allocated the map is unchanged
 * (DSI_ERR_HIP).  Errors as dsx_map_knn_select's.  Synchronises. */
DSI_API int dsx_map_prune_knn(dsi_map_t *map, const dsx_map_knn_selection_t *sel, dsx_map_knn_select_info_t *info);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_KNN_H */
