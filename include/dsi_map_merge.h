/* Merging world maps and moving their exact state: one map appended to another on the device, and a map's raw cells
 * (key, n, S[3], windows, stamp) exported to and imported from host arrays.  DESIGN.md 7j "Merging".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  All arithmetic is integer:
 * the result is a function of the two maps alone, whatever the tables' sizes, the probing and the order of the threads.
 * tests/map_merge_reference.py restates everything here in numpy. */
#ifndef DSI_MAP_MERGE_H
#define DSI_MAP_MERGE_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule: a merge appends ----
 * Merging src into dst yields, bit for bit, the map that had made dst's integrate calls and then src's integrate calls:
 * keys, n, S[3], windows, stamp and the counters calls, accepted, rejected.  With off = dst's calls before the merge, for
 * every cell of src (a cell that dst lacks starts from zeros):
 *     n += n_src;   S[a] += S_src[a];   windows += windows_src;   stamp = max(stamp, stamp_src + off)
 * then calls += src.calls, accepted += src.accepted, rejected += src.rejected.  dst's table doubles first until
 * occupied + src's cells <= 3/4 of its slots.  src is unchanged and keeps its render, compare and classification; dst
 * loses its own, as after an integrate call.
 * What follows from the rule:
 *   - importing a state into an empty map with calls == 0 restores it exactly, ages (dsi_map_prune.h criterion 3) included;
 *   - merging an empty map with calls == k ages every cell of dst by k;
 *   - a pruned dst followed by a merge equals the pruned map followed by src's calls: a removed cell starts from zero;
 *   - for maps filled round-robin from one stream of windows, n, S, windows and the centroids are exactly those of the
 *     single map, but the stamps follow the rule above -- every call of src counts as later than every call of dst --
 *     and not the interleaved history.
 * Refused with DSI_ERR_INVALID unless another code is given, judged before dst is touched, so that dst stays as it is
 * bit for bit; dsi_last_error names the offending thing: a NULL map, state or array; dst == src; maps of different
 * contexts (DSI_ERR_CONTEXT); a leaf that is not bit-equal; a table that overflowed earlier; dst.calls + src.calls or
 * dst.accepted + src.accepted above 2^32 - 1 (stamps and n are 32 bits wide, and n <= accepted); dst's cells + src's
 * cells needing more than 2^27 slots; a table that cannot be allocated (DSI_ERR_HIP). */
typedef struct dsx_map_state {
    double leaf;
    uint64_t n_cells, calls, accepted, rejected;
} dsx_map_state_t; /* 40 bytes */
typedef struct dsx_map_merge_info {
    uint64_t n_src_cells; /* = n_new + n_common */
    uint64_t n_new;       /* cells that dst lacked */
    uint64_t n_common;
    uint64_t capacity;    /* dst's slots after the call */
    uint64_t growths;     /* the doublings this call made in dst's table */
} dsx_map_merge_info_t; /* 40 bytes */

/* Every occupied cell with its raw state, in dsi_map_extract(0, 0)'s order (the table's; sort by key on the host) and
 * with its capacity protocol: when capacity < *count nothing is written to the arrays and DSI_ERR_INVALID comes back
 * with *count set.  keys, n, windows, stamp: one per cell; sums: three per cell (x y z).  Any array may be NULL.  state
 * (may be NULL) is always filled when map and count are given.  Changes nothing and invalidates nothing.  Synchronises. */
DSI_API int dsx_map_export(dsi_map_t *map, dsx_map_state_t *state, uint64_t *keys, uint32_t *n, uint64_t *sums,
                           uint32_t *windows, uint32_t *stamp, size_t capacity, size_t *count);
/* dsx_map_merge with host arrays as src: the arrays are built into a scratch table on the device, which validates them,
 * and that table goes through the merge.  Nothing is trusted from the host.  Beyond the refusals above: all five arrays
 * are needed when n_cells > 0; per cell, a key 0, a packed coordinate outside [1, 2^21 - 3], a duplicate key, n == 0,
 * windows == 0, windows > n, windows > stamp, stamp == 0, stamp > calls or some S[a] > n * 2^32; per state,
 * accepted < the sum of n, a leaf that is not finite and > 0, n_cells > 2^27.  info may be NULL.  Synchronises. */
DSI_API int dsx_map_import(dsi_map_t *dst, const dsx_map_state_t *state, const uint64_t *keys, const uint32_t *n,
                           const uint64_t *sums, const uint32_t *windows, const uint32_t *stamp, dsx_map_merge_info_t *info);
/* src appended to dst on the device, by the rule above; both on one context.  info may be NULL.  Synchronises. */
DSI_API int dsx_map_merge(dsi_map_t *dst, dsi_map_t *src, dsx_map_merge_info_t *info);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_MERGE_H */
