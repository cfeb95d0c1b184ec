/* Pruning the world map: cells leave it by point count, window count, age, a box around the vehicle and neighbour
 * support, and the table is rebuilt (and, on request, shrunk) around the cells that stay.  DESIGN.md 7j "Pruning".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  All arithmetic is integer,
 * or double with every operation rounded on its own: the result is a function of the map and the options alone, whatever
 * the table's size, the probing and the order of the threads.  tests/map_prune_reference.py restates everything here in
 * numpy. */
#ifndef DSI_MAP_PRUNE_H
#define DSI_MAP_PRUNE_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----
 * Every decision is taken on the map as it stands when the call begins; nothing is removed before every cell is decided.
 * A cell's reason is the FIRST criterion that fails, or 0 (kept):
 *   1. n < min_points;
 *   2. windows < min_windows;
 *   3. max_age >= 0 and calls - stamp > max_age.  calls is dsi_map_info's; stamp is the serial (1-based) of the last
 *      integrate call that put an accepted point into the cell: age 0 is the last call.  An empty integrate call is a
 *      call: it ages every cell by one;
 *   4. use_box and the centroid -- exactly as dsi_map_extract returns it (rule 5, float32), widened to double -- lies
 *      outside the closed box on some axis: p < box_lo or p > box_hi, compared in double;
 *   5. reach > 0 and fewer than min_neighbors OTHER cells that survive criteria 1-4 lie among those whose cell index
 *      differs by at most reach per axis -- (2 reach + 1)^3 - 1 read-only lookups; an index with |c + o| > 2^20 - 2 is
 *      skipped.  A neighbour that criterion 5 itself removes still counts: one pass, as PCL's radius outlier filter.
 * Bounds of the options, judged before the map is looked at and before the GPU is touched: use_box and shrink are 0 or
 * 1; with use_box no bound is NaN and box_lo <= box_hi per axis (+-inf is legal; the box is ignored when use_box == 0);
 * reach is 0, 1 or 2; with reach > 0, 1 <= min_neighbors <= (2 reach + 1)^3 - 1; with reach == 0, min_neighbors == 0.
 * min_points <= 1 and min_windows <= 1 switch criteria 1 and 2 off (every cell holds a point of some call). */
typedef struct dsx_map_prune_opts {
    uint32_t min_points, min_windows; /* criteria 1, 2 (0 and 1 switch them off) */
    int64_t max_age;                  /* criterion 3: < 0 off */
    int32_t use_box;                  /* criterion 4: 0 or 1 */
    double box_lo[3], box_hi[3];      /* no NaN, lo <= hi per axis, +-inf legal; ignored when use_box == 0 */
    int32_t reach;                    /* criterion 5: 0 off, 1 or 2 */
    uint32_t min_neighbors;           /* reach > 0: 1 .. (2 reach + 1)^3 - 1; reach == 0: must be 0 */
    int32_t shrink;                   /* 0 or 1 */
} dsx_map_prune_opts_t;
typedef struct dsx_map_prune_info {
    uint64_t n_cells;      /* occupied cells before; = n_kept + sum n_removed */
    uint64_t n_kept;
    uint64_t n_removed[5]; /* by the FIRST criterion that fails, in the order above */
    uint64_t capacity;     /* slots after the call */
} dsx_map_prune_info_t;

/* The dry run: classifies every cell and counts; the map, its render and its compare stay as they are.  The per-slot
 * reasons stay on the device, in a buffer that belongs to the map, for dsx_map_prune_fetch.  info may be NULL.
 * DSI_ERR_INVALID for a NULL map or opts, a violated bound, and a map whose table overflowed earlier.  Synchronises. */
DSI_API int dsx_map_prune_classify(dsi_map_t *map, const dsx_map_prune_opts_t *opts, dsx_map_prune_info_t *info);
/* (key, reason) of every occupied cell of the last dsx_map_prune_classify, in dsi_map_extract(1, 1)'s order; either
 * output may be NULL.  dsi_map_extract's capacity protocol: when capacity < *n nothing is written and DSI_ERR_INVALID
 * comes back with *n set.  DSI_ERR_INVALID before the first classify and after dsi_map_reset, any integrate call or a
 * dsx_map_prune.  Synchronises. */
DSI_API int dsx_map_prune_fetch(dsi_map_t *map, uint8_t *reason_host, uint64_t *keys_host, size_t capacity, size_t *n);
/* Classifies, then rebuilds: the kept cells move into a fresh zeroed table with all their state (n, S[3], windows,
 * stamp).  With shrink the new capacity is the smallest 2^k, k >= 8, with 4 * kept <= 3 * 2^k; without it the capacity
 * stays.  Afterwards dsi_map_info's occupied == n_kept; calls, accepted, rejected and growths keep their values, so
 * ages go on counting; a removed cell that a later call reaches starts from zero.  Always invalidates the map's render,
 * compare and classification, as an integrate call does.  If the new table cannot be allocated the map is unchanged
 * (DSI_ERR_HIP).  info may be NULL.  Errors as dsx_map_prune_classify's.  Synchronises. */
DSI_API int dsx_map_prune(dsi_map_t *map, const dsx_map_prune_opts_t *opts, dsx_map_prune_info_t *info);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_PRUNE_H */
