/* The world map's local shape: a principal component analysis of every cell's neighbourhood.  It gives a normal where the
 * neighbourhood is planar, a tangent where it is linear, says which of the two it is -- or neither: scattered cells are
 * noise that no count of neighbours can tell from structure -- and prunes by that label.  DESIGN.md 7j "Local shape".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  The result is a function of
 * the map and the options alone, bit for bit whatever the table's size, the probing and the order of the threads.
 * tests/map_pca_reference.py restates everything here in numpy and Python ints. */
#ifndef DSI_MAP_PCA_H
#define DSI_MAP_PCA_H

#include "dsi_engine.h"
#include "dsi_map_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----
 * Double arithmetic, every operation rounded on its own, no FMA.  A QUERY is every cell with n >= min_points &&
 * windows >= min_windows; p is its centroid as dsi_map_extract returns it (float32), widened to double.
 *
 *   1. NEIGHBOURS.  Steps 1-4 of dsi_map_knn.h's rule give the admitted set A of p (reach = ceil(radius / leaf) on the host,
 *      1..3; the candidates pass the same filter); the cell itself is excluded BY KEY.  k == 0: the neighbourhood is all
 *      of A (the radius search; at most (2 reach + 1)^3 - 1 = 342 cells).  k in 1..16: the first k of A by (d2, key) (the
 *      k-search inside the radius).  found is the neighbourhood's size.  The cell itself is always a member, as in PCL's
 *      searches: m = found + 1.
 *   2. QUANTISED OFFSETS.  quantum = leaf * 2^-10.  Per neighbour with centroid q (float32, widened) and per axis
 *      D = llrint((q - p) / quantum): the IEEE subtraction, the IEEE divide, ties to even.  |q - p| <= radius <= 3 leaf, so
 *      |D| <= 3073.  The cell's own D is 0.
 *   3. INTEGER MOMENTS.  s[a] = sum D[a]; ss[ab] = sum D[a] D[b] for ab = xx, xy, xz, yy, yz, zz (in this order);
 *      C[ab] = m ss[ab] - s[a] s[b].  |s| <= 342 * 3073 < 2^21, |ss| <= 342 * 3073^2 < 2^32, |C| < 2^41: int64 suffices and
 *      every C[ab] converts to double exactly.  Integer sums commute: the moments do not depend on the order of the scan.
 *   4. EIGEN-SOLVE.  A = (double) C as a full symmetric 3 x 3 matrix, V = I.  8 sweeps of cyclic Jacobi over
 *      (p, q) = (0,1) (0,2) (1,2) with dsx_map_align_solve's update (dsi_map_align.h), k running over 0..2: a pair whose
 *      A[p][q] is exactly 0 is skipped, otherwise
 *          theta = (A[q][q] - A[p][p]) / (2 A[p][q]);  t = sign(theta) / (|theta| + sqrt(theta theta + 1))  (sign(0) = +1);
 *          c = 1 / sqrt(t t + 1);  s = t c;
 *          for k: (A[k][p], A[k][q]) = (c A[k][p] - s A[k][q], s A[k][p] + c A[k][q]);   -- columns, from the old pair
 *          for k: (A[p][k], A[q][k]) = (c A[p][k] - s A[q][k], s A[p][k] + c A[q][k]);   -- then rows
 *          for k: (V[k][p], V[k][q]) = (c V[k][p] - s V[k][q], s V[k][p] + c V[k][q]).
 *      As there, both triangles of A are carried: they differ in their last bits once a pair has been rotated.
 *      lambda = A's diagonal, each clamped below at 0.  i0 = the index of the first minimum, i2 = the index of the first
 *      maximum among the other two, i1 = the remaining index: lambda0 <= lambda1 <= lambda2 are lambda[i0], [i1], [i2].
 *      normal = V's column i0 divided by its norm sqrt(((x x + y y) + z z)); tangent = column i2, normalised the same way.
 *   5. DETERMINED OR NOT (the scale-free test of the align solver).  With S = (lambda0 + lambda1) + lambda2: the normal
 *      is determined iff lambda1 - lambda0 > 2^-26 S (flags bit 0), the tangent iff lambda2 - lambda1 > 2^-26 S (bit 1).
 *      An undetermined vector is still the solver's column: a member of the eigenspace, of no meaning of its own.
 *   6. SIGN.  Canonical: the component of largest magnitude is made positive; among equal magnitudes the first counts.
 *      The tangent always takes the canonical sign.  The normal does unless orient == 1: then w = viewpoint - p per
 *      axis, dot = ((n0 w0 + n1 w1) + n2 w2) of the canonically signed normal; it is negated when dot < 0 and kept
 *      when dot >= 0 (dot == 0: the canonical sign).  The map stores no viewing directions.
 *   7. LABEL.  sigma_i = sqrt(lambda_i), correctly rounded.  The label is the first maximum of
 *      (sigma2 - sigma1, sigma1 - sigma0, sigma0): 1 linear, 2 planar, 3 scattered (the dimensionality feature of
 *      Demantke et al. without its common divisor).  A query with found < min_found is SPARSE: label 0, no solve, flags 0,
 *      vectors 0, eigenvalues +inf.
 *   8. PER-SLOT RESULTS, on the device in buffers that belong to the map: normal and tangent as 3 float32 each (the
 *      doubles rounded), eval[3] float32 with eval_i = (float) ((lambda_i / ((double) m (double) m)) (quantum quantum)) --
 *      the population covariance's eigenvalues in the map's unit squared, ascending --, members = m as uint16, label and
 *      flags as uint8 (40 bytes per slot), and with keep_moments the nine integers s[3], ss[6] as int64 (72 more).
 *   9. INFO: exact integer counters.
 * Bounds of the options, judged before the map is looked at and before the GPU is touched: k is 0..16; min_found is
 * 2..max(k, 2), and 2..342 for k == 0; radius is finite and > 0, and with the map at hand reach is 1..3; orient and
 * keep_moments are 0 or 1; the viewpoint is finite (also when orient is 0). */
typedef struct dsx_map_pca_opts {
    uint32_t min_points, min_windows; /* the queries' filter, and the candidates' */
    int32_t k;                        /* 0: every admitted cell; 1..16: the k nearest of them */
    int32_t min_found;                /* 2..max(k, 2); k == 0: 2..342 */
    double radius;                    /* finite, > 0, at most three leaves */
    int32_t orient;                   /* 1: the normal looks at the viewpoint */
    int32_t keep_moments;             /* 1: s and ss stay on the device for dsx_map_pca_fetch */
    double viewpoint[3];              /* finite */
} dsx_map_pca_opts_t;
typedef struct dsx_map_pca_info {
    uint64_t n_cells;     /* queries: the cells that pass the filter */
    uint64_t n_unqueried; /* occupied cells that the filter leaves out */
    uint64_t n_sparse;    /* queries with found < min_found; n_cells = n_sparse + sum n_label */
    uint64_t n_label[3];  /* linear, planar, scattered */
    uint64_t n_normal_determined, n_tangent_determined;
    uint64_t sum_members; /* sum of m over the queries, the sparse ones included */
    int32_t reach;
} dsx_map_pca_info_t;
/* One cell's solve.  normal_d, tangent_d and lambda (ascending, clamped) are the doubles of steps 4-6; the rest is the row
 * of step 8. */
typedef struct dsx_pca_row {
    double normal_d[3], tangent_d[3], lambda[3];
    float normal[3], tangent[3], eval[3];
    uint8_t label, flags;
} dsx_pca_row_t;
#define DSX_PCA_LINEAR 1u    /* the bits of keep_labels: 1 << (label - 1) */
#define DSX_PCA_PLANAR 2u
#define DSX_PCA_SCATTERED 4u
typedef struct dsx_map_pca_selection {
    uint32_t keep_labels;  /* 1..7: a mask over the labels 1..3 */
    int32_t remove_sparse; /* 0 or 1 */
    int32_t shrink;        /* 0 or 1; read by dsx_map_prune_pca, only checked by the dry run */
} dsx_map_pca_selection_t;
typedef struct dsx_map_pca_select_info {
    uint64_t n_cells;      /* occupied cells before; = n_kept + sum n_removed */
    uint64_t n_kept;
    uint64_t n_removed[3]; /* by the FIRST reason that holds, in the order below */
    uint64_t capacity;     /* slots after the call */
} dsx_map_pca_select_info_t;

/* The pass above over the map as it stands.  The per-slot results stay on the device until the map changes:
 * dsi_map_reset, any integrate call, a merge, an import or a prune of any kind invalidates them.  Changes nothing else:
 * the map's render, compare, alignment step, classification, labelling and self query stay valid.  info may be NULL.
 * DSI_ERR_INVALID for NULL opts, a violated bound (judged first, with no map at hand), a NULL map and a map whose table
 * overflowed earlier.  Synchronises. */
DSI_API int dsx_map_pca(dsi_map_t *map, const dsx_map_pca_opts_t *opts, dsx_map_pca_info_t *info);
/* The rows of every query of the pass, in the order of dsi_map_extract under the query's filter; any output may be NULL.
 * normal_host, tangent_host, eval_host: [count][3]; moments_host: [count][9], s[3] then ss[6].  dsi_map_extract's capacity
 * protocol: when capacity < *count nothing is written and DSI_ERR_INVALID comes back with *count set.  A non-NULL
 * moments_host needs a pass with keep_moments, a non-NULL reasons_host a dsx_map_pca_select on this pass.  DSI_ERR_INVALID
 * without a valid pass.  Synchronises. */
DSI_API int dsx_map_pca_fetch(dsi_map_t *map, uint64_t *keys_host, float *normal_host, float *tangent_host, float *eval_host,
                              uint16_t *members_host, uint8_t *label_host, uint8_t *flags_host, int64_t *moments_host,
                              uint8_t *reasons_host, size_t capacity, size_t *count);
/* Steps 3-7 from one cell's integers: host only, no context needed.  m = found + 1; s[3]; ss[6]; quantum > 0 and finite;
 * p the cell's centroid and viewpoint, read when orient == 1 (both may be NULL otherwise).  There is no min_found here:
 * whether a row is sparse is the pass's decision, and a sparse row has no solve.  DSI_ERR_INVALID for a NULL s, ss or
 * out, a quantum that is not finite and > 0, an orient outside 0..1, a non-finite or NULL viewpoint or p with orient == 1,
 * and moments that no pass can return: m outside 1..343, |s[a]| > (m - 1) * 3073, an ss[aa] outside 0..(m - 1) * 3073^2,
 * |ss[ab]| beyond that bound, or a negative C[aa]. */
DSI_API int dsx_pca_solve(uint32_t m, const int64_t s[3], const int64_t ss[6], double quantum, int32_t orient, const double viewpoint[3],
                          const double p[3], dsx_pca_row_t *out);
/* The dry run of the selection on the pass.  A cell's reason is the FIRST that holds, or 0 (kept):
 *   1. the cell fails the query's filter;
 *   2. it is sparse and remove_sparse (a sparse cell that stays is kept: it has no label to judge);
 *   3. its label's bit is not in keep_labels.
 * Decides every occupied cell and counts; the map and everything derived from it stay as they are.  The per-slot reasons
 * stay on the device for dsx_map_pca_fetch.  info may be NULL.  DSI_ERR_INVALID for NULL sel, a violated bound, a NULL
 * map and a map without a valid pass.  Synchronises. */
DSI_API int dsx_map_pca_select(dsi_map_t *map, const dsx_map_pca_selection_t *sel, dsx_map_pca_select_info_t *info);
/* Selects, then rebuilds as dsx_map_prune_knn does: the kept cells move into a fresh zeroed table with all their state.
 * With shrink the new capacity is the smallest 2^k, k >= 8, with 4 * kept <= 3 * 2^k; without it the capacity stays.
 * calls, accepted, rejected and growths keep their values.  Invalidates the map's render, compare, alignment step,
 * classification, labelling, self query and this pass.  If the new table cannot be allocated the map is unchanged
 * (DSI_ERR_HIP).  Errors as dsx_map_pca_select's.  Synchronises. */
DSI_API int dsx_map_prune_pca(dsi_map_t *map, const dsx_map_pca_selection_t *sel, dsx_map_pca_select_info_t *info);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_PCA_H */
