/* The world map's connected components: which cells hang together, and pruning by component -- keep the largest structures,
 * drop the small floating clusters that support themselves under dsx_map_prune's neighbour criterion.  DESIGN.md 7j
 * "Components".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  All arithmetic is integer:
 * the result is a function of the map and the options alone, whatever the table's size, the probing and the order of the
 * threads.  tests/map_components_reference.py restates everything here in numpy and scipy. */
#ifndef DSI_MAP_COMPONENTS_H
#define DSI_MAP_COMPONENTS_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----
 * NODES are the cells with n >= min_points && windows >= min_windows (dsi_map_extract's filter); the other occupied cells
 * are UNLABELLED.  Two nodes are ADJACENT when their cell indices differ by an offset o != 0 of the connectivity:
 *      6   |o|_inf = 1 and |o|_1 = 1        (faces)
 *     18   |o|_inf = 1 and |o|_1 <= 2       (faces and edges)
 *     26   |o|_inf = 1                      (faces, edges and corners)
 *    124   |o|_inf <= 2                     (the 5 x 5 x 5 box)
 * Any other connectivity is refused.  An index with |c + o| > 2^20 - 2 has no key and is skipped, as in dsx_map_prune's
 * criterion 5.  A COMPONENT is a class of the transitive closure; its LABEL is the smallest packed key (rule 6 of
 * dsi_engine.h) among its cells; it has `cells` (their number) and `points` (the sum of their n), both 64 bits wide.
 *
 * SELECTION (dsx_map_components_select, dsx_map_prune_components).  A cell's reason is the FIRST that holds, or 0 (kept):
 *   1. the cell is unlabelled;
 *   2. its component has cells < min_cells;
 *   3. its component has points < min_component_points;
 *   4. keep_largest > 0 and its component is not among the keep_largest first of the components that pass 2 and 3,
 *      ordered by cells descending, then label ascending.
 * Bounds of the options, judged before the map is looked at and before the GPU is touched: connectivity is 6, 18, 26 or
 * 124; keep_largest is 0..16; shrink is 0 or 1.  min_cells and min_component_points of 0 or 1 switch their criterion off
 * (every component holds a cell, every cell a point). */
typedef struct dsx_map_components_opts {
    uint32_t min_points, min_windows; /* the nodes' filter */
    int32_t connectivity;             /* 6, 18, 26 or 124 */
} dsx_map_components_opts_t;
typedef struct dsx_map_components_info {
    uint64_t n_cells;       /* nodes */
    uint64_t n_unlabelled;  /* occupied cells that the filter leaves out */
    uint64_t n_components;
    uint64_t n_singletons;  /* components of one cell */
    uint64_t largest_label, largest_cells, largest_points; /* the first by criterion 4's order; all 0 for an empty map */
} dsx_map_components_info_t;
typedef struct dsx_map_components_selection {
    uint64_t min_cells;            /* criterion 2 (0 and 1 switch it off) */
    uint64_t min_component_points; /* criterion 3 (0 and 1 switch it off) */
    int32_t keep_largest;          /* criterion 4: 0 off, 1..16 */
    int32_t shrink;                /* 0 or 1; read by dsx_map_prune_components, only checked by the dry run */
} dsx_map_components_selection_t;
typedef struct dsx_map_components_select_info {
    uint64_t n_cells;      /* occupied cells before; = n_kept + sum n_removed */
    uint64_t n_kept;
    uint64_t n_removed[4]; /* by the FIRST reason that holds, in the order above */
    uint64_t n_components_kept;
    uint64_t capacity;     /* slots after the call */
} dsx_map_components_select_info_t;

/* Labels the map as it stands.  The labelling stays on the device, in buffers that belong to the map (allocated on first
 * use, about 25 bytes per slot, freed by dsi_map_destroy), until the map changes: dsi_map_reset, any integrate call, a
 * merge, an import or a prune invalidates it.  Changes nothing else: the map, its render, its compare, its alignment step
 * and its prune classification stay valid.  info may be NULL.  DSI_ERR_INVALID for NULL opts, a violated bound, a NULL map
 * and a map whose table overflowed earlier.  Synchronises. */
DSI_API int dsx_map_components(dsi_map_t *map, const dsx_map_components_opts_t *opts, dsx_map_components_info_t *info);
/* (key, label, reason) of every node of the labelling, in the order of dsi_map_extract under the labelling's filter; any
 * output may be NULL.  dsi_map_extract's capacity protocol: when capacity < *count nothing is written and DSI_ERR_INVALID
 * comes back with *count set.  A non-NULL reasons_host needs a dsx_map_components_select on this labelling.
 * DSI_ERR_INVALID without a valid labelling.  Synchronises. */
DSI_API int dsx_map_components_fetch(dsi_map_t *map, uint64_t *keys_host, uint64_t *labels_host, uint8_t *reasons_host, size_t capacity,
                                     size_t *count);
/* (label, cells, points) of every component of the labelling, in the table's order (sort by label for a fixed order); any
 * output may be NULL.  The same capacity protocol and errors.  Synchronises. */
DSI_API int dsx_map_components_list(dsi_map_t *map, uint64_t *labels_host, uint64_t *cells_host, uint64_t *points_host, size_t capacity,
                                    size_t *count);
/* The dry run of the selection on the labelling: decides every occupied cell and counts; the map and everything derived
 * from it stay as they are.  The per-slot reasons stay on the device for dsx_map_components_fetch.  info may be NULL.
 * DSI_ERR_INVALID for NULL sel, a violated bound, a NULL map and a map without a valid labelling.  Synchronises. */
DSI_API int dsx_map_components_select(dsi_map_t *map, const dsx_map_components_selection_t *sel, dsx_map_components_select_info_t *info);
/* Selects, then rebuilds as dsx_map_prune does: the kept cells move into a fresh zeroed table with all their state (n,
 * S[3], windows, stamp).  With shrink the new capacity is the smallest 2^k, k >= 8, with 4 * kept <= 3 * 2^k; without it
 * the capacity stays.  calls, accepted, rejected and growths keep their values.  Invalidates the map's render, compare,
 * alignment step, classification and labelling.  If the new table cannot be allocated the map is unchanged (DSI_ERR_HIP).
 * Errors as dsx_map_components_select's.  Synchronises. */
DSI_API int dsx_map_prune_components(dsi_map_t *map, const dsx_map_components_selection_t *sel, dsx_map_components_select_info_t *info);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_COMPONENTS_H */
