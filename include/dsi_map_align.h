/* Aligning world maps: the rigid motion that carries one map onto another, estimated by ICP whose every device effect is
 * an integer sum, and one map re-integrated into another's frame on the device.  DESIGN.md 7j "Aligning".
 *
 * These entry points live beside the core boundary of dsi_engine.h, in the same library, under the prefix dsx_: they
 * take its handle dsi_map_t, return its DSI_ERR_* codes and leave dsi_abi_version() as it is.  "Rules 1-5" below are the
 * world map's, stated in dsi_engine.h; "compare rules" are dsx_map_compare's, stated in dsi_map_eval.h.  All floating
 * arithmetic is double, every product and sum rounded on its own (no FMA), and a dot product is taken as
 * ((a0 b0 + a1 b1) + a2 b2).  A pose is 12 doubles, row-major [R | t].  tests/map_align_reference.py restates everything
 * here in numpy and Python ints. */
#ifndef DSI_MAP_ALIGN_H
#define DSI_MAP_ALIGN_H

#include "dsi_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one correspondence pass ----
 * T is the current estimate of the frame of `a` expressed in the frame of `b`.  For every cell of `a` with
 * n >= min_points_a && windows >= min_windows_a:
 *   1. p = its centroid exactly as dsi_map_extract returns it (rule 5, rounded to float32), widened to double;
 *   2. p' = T p by rule 1: p'[r] = ((T[4r] p0 + T[4r+1] p1) + T[4r+2] p2) + T[4r+3];
 *   3. per axis c = floor(p' / leaf_b); reach = (int) ceil(radius / leaf_b), computed once on the host.  A non-finite p'
 *      has a non-finite c and therefore no candidates;
 *   4. the candidates are the cells of `b` with n >= min_points_b && windows >= min_windows_b whose index is c + o,
 *      |o| <= reach per axis (an index with |c + o| > 2^20 - 2 is skipped).  For each, q = its centroid by rule 5 as
 *      float32, widened, d = p' - q per axis and d2 = ((dx dx) + dy dy) + dz dz;
 *   5. the correspondence is the candidate of least d2, and among equal d2 the one of the smaller key: a total order, so
 *      neither the probing nor the order of the offsets matters;
 *   6. the cell is MATCHED iff a candidate exists and sqrt(d2) <= radius (the IEEE square root), else UNMATCHED.
 * Quantisation of a matched pair: quantum = leaf_b * 2^-10 (exact: a power of two times leaf_b), per axis
 *   U = llrint(p' / quantum), V = llrint(q / quantum), the IEEE divide rounded to the nearest integer, ties to even.
 * Why nothing below overflows.  A centroid of b is at most (2^20 - 1) leaf_b in magnitude before its rounding to float32
 * (|c| <= 2^20 - 2, fraction < 1), and that rounding (relative 2^-24) keeps it below 2^20 leaf_b: |q / quantum| < 2^30, so
 * |V| < 2^30.  A matched pair has |p' - q| <= sqrt(d2) <= radius <= 3 leaf_b per axis (reach <= 3), i.e. at most 3072
 * quanta, and the two roundings add less than one more: |U - V| <= 3073 and |U| < 2^30 + 3073.  Both fit 32 bits; a
 * product U[r] V[c] is below 2^61 in magnitude; a map holds at most 2^27 cells, so a sum of U or V stays below 2^58, a sum
 * of the products' high words (each below 2^30) below 2^57, a sum of their low words (each below 2^32) below 2^59, and
 * e2, whose terms are at most 3 * 3073^2 < 2^25, below 2^52.
 * The moments, integers accumulated over the matched cells:
 *   n_cells = n_matched + n_unmatched     the cells of a that passed its filter
 *   su[r] = sum U[r], sv[c] = sum V[c]    (int64)
 *   P = U[r] V[c] (int64) is split as hi = P >> 32 (arithmetic shift: floor(P / 2^32)) and lo = P & 0xffffffff;
 *   suv_hi[3 r + c] = sum hi (int64), suv_lo[3 r + c] = sum lo (uint64): sum P = suv_hi * 2^32 + suv_lo, exactly
 *   e2 = sum over the cells and the axes of (U - V)^2 (uint64)
 * and quantum and reach are copied in for the solver and the caller.  Integer sums commute: the moments are a function
 * of the two maps, the options and T alone, whatever the tables' sizes, the probing and the order of the threads.
 * Per cell, key_b (the correspondence's key; 0 when unmatched) and (float) sqrt(d2) (+inf when unmatched) are kept on
 * the device in buffers that belong to `a`, for dsx_map_align_fetch.  The lookups only read: a == b is legal, the leaves
 * may differ, either map may be empty. */
typedef struct dsx_map_align_opts {
    uint32_t min_points_a, min_windows_a;  /* dsi_map_extract's filter on a */
    uint32_t min_points_b, min_windows_b;  /* and on b */
    double radius;                         /* finite, > 0, with 1 <= ceil(radius / leaf_b) <= 3 */
    /* the loop's (dsx_map_align); dsx_map_align_step does not look at them */
    int32_t max_iterations;                /* 1..64 */
    int32_t reserved;                      /* 0 */
    uint64_t min_matched;                  /* a pass that matches fewer cells ends the loop with DSI_ERR_INVALID */
    double eps_rot, eps_trans;             /* finite, >= 0: radians and the map's unit of length */
} dsx_map_align_opts_t; /* 56 bytes */
typedef struct dsx_map_align_moments {
    uint64_t n_cells, n_matched, n_unmatched;
    int64_t su[3], sv[3];
    int64_t suv_hi[9];
    uint64_t suv_lo[9];
    uint64_t e2;
    double quantum;
    int32_t reach, reserved;
} dsx_map_align_moments_t; /* 240 bytes */
/* DSI_ERR_INVALID for a NULL opts, T, moments or map, a non-finite entry of T, a violated bound on radius or a table
 * that overflowed in an earlier call (opts and T are judged before the maps are looked at); DSI_ERR_CONTEXT when the maps
 * were created from different contexts -- all decided before the GPU is touched.  Synchronises. */
DSI_API int dsx_map_align_step(dsi_map_t *a, dsi_map_t *b, const dsx_map_align_opts_t *opts, const double T[12],
                               dsx_map_align_moments_t *moments);
/* (key_a, key_b, dist) of the last step in which `a` was the first map (the last pass of a dsx_map_align included), for
 * the cells of that step's filter on a, in dsi_map_extract's order; any output may be NULL.  dsi_map_extract's capacity
 * protocol: when capacity < *n nothing is written, *n is the size needed and the call returns DSI_ERR_INVALID.
 * DSI_ERR_INVALID before the first step and after dsi_map_reset, any integrate call, a merge into or a prune of a.  A
 * change to b after the step does NOT invalidate it.  Synchronises. */
DSI_API int dsx_map_align_fetch(dsi_map_t *a, uint64_t *keys_a, uint64_t *keys_b, float *dist, size_t capacity, size_t *n);

/* ---- host-only routines: no device is touched ---- */
/* out = A o B: R = A_R B_R, every entry a dot product of a row of A_R and a column of B_R, and
 * t[r] = ((A[4r] B[3] + A[4r+1] B[7]) + A[4r+2] B[11]) + A[4r+3].  out may alias A or B.  DSI_ERR_INVALID for NULL. */
DSI_API int dsx_pose_compose(const double A[12], const double B[12], double out[12]);

typedef struct dsx_map_align_solve_info {
    uint64_t n_matched;
    double rms;           /* sqrt((double) e2 * quantum^2 / (double) n_matched): of the pairs as they were matched */
    double angle, trans;  /* of T_delta: atan2-based rotation angle in radians, and the norm of its translation */
    double lambda[2];     /* the two largest eigenvalues of Horn's matrix */
} dsx_map_align_solve_info_t; /* 48 bytes */
/* The rigid motion T_delta minimising sum |R U + t - V|^2 over the matched pairs (in the map's unit: U, V times quantum),
 * from the moments alone:
 *   1. centred in integers: C[r][c] = n sum P - su[r] sv[c] (__int128; below 2^114 in magnitude), each converted to
 *      double once and multiplied by quantum^2 / n^2 (n as double; the factor computed once as (quantum quantum) / (n n));
 *      call the results Sxx = S[0][0], Sxy = S[0][1], ... (row: the axis of U, column: the axis of V);
 *   2. Horn's 4 x 4 symmetric matrix N, whose eigenvector of the largest eigenvalue is the unit quaternion (w, x, y, z)
 *      of R.  Its diagonal is (Sxx + Syy) + Szz, (Sxx - Syy) - Szz, (Syy - Sxx) - Szz, (Szz - Sxx) - Syy, and
 *      N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx, N12 = Sxy + Syx, N13 = Szx + Sxz, N23 = Syz + Szy.
 *      The eigenproblem is solved by 16 sweeps of cyclic Jacobi over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V = I
 *      at the start; a pair whose A[p][q] is exactly 0 is skipped, otherwise
 *          theta = (A[q][q] - A[p][p]) / (2 A[p][q]);  t = sign(theta) / (|theta| + sqrt(theta theta + 1))  (sign(0) = +1);
 *          c = 1 / sqrt(t t + 1);  s = t c;
 *          for k = 0..3: (A[k][p], A[k][q]) = (c A[k][p] - s A[k][q], s A[k][p] + c A[k][q]);   -- columns, from the old pair
 *          for k = 0..3: (A[p][k], A[q][k]) = (c A[p][k] - s A[q][k], s A[p][k] + c A[q][k]);   -- then rows
 *          for k = 0..3: (V[k][p], V[k][q]) = (c V[k][p] - s V[k][q], s V[k][p] + c V[k][q]).
 *      The eigenvalues are A's diagonal; the largest is the first maximum, the second the first maximum of the rest.  No
 *      LAPACK, no Eigen: every caller of this library gets the same bits;
 *   3. the quaternion is V's column of the largest eigenvalue divided by its norm sqrt(((w w + x x) + y y) + z z), negated
 *      when w < 0; R is pose_matrix's expression of it (r00 = 1 - 2 (y y + z z), r01 = 2 (x y - w z), r02 = 2 (x z + w y),
 *      r10 = 2 (x y + w z), r11 = 1 - 2 (x x + z z), r12 = 2 (y z - w x), r20 = 2 (x z - w y), r21 = 2 (y z + w x),
 *      r22 = 1 - 2 (x x + y y)); t = mean(V) - R mean(U) with mean[r] = ((double) sum[r] / n) quantum and R mean(U) a dot
 *      product per row; angle = 2 atan2(sqrt((x x + y y) + z z), w), trans = sqrt((t0 t0 + t1 t1) + t2 t2).
 * DSI_ERR_INVALID, T_delta untouched and dsi_last_error naming the cause, when n_matched < 3 or when the largest
 * eigenvalue is not separated from the second: unless lambda[0] - lambda[1] > 2^-26 (((|A00| + |A11|) + |A22|) + |A33|).
 * The test is scale-free (a common factor of the point sets multiplies both sides alike); it refuses pairs whose
 * centred U or V are collinear or coincide, for which the rotation about the line is not determined (the two largest
 * eigenvalues are then equal), and it keeps planar sets, whose N has separated eigenvalues.  2^-26 is the square root of
 * the double's epsilon: where the gap is smaller relative to the matrix than that, Jacobi's eigenvector has no correct
 * digits left in half of its bits.  info (may be NULL) is filled on success, and on the separation refusal too. */
DSI_API int dsx_map_align_solve(const dsx_map_align_moments_t *moments, double T_delta[12], dsx_map_align_solve_info_t *info);

/* ---- the loop ----
 * T = T_init; up to opts->max_iterations rounds of: step(a, b, T); solve; T = compose(T_delta, T).  It ends
 *   - converged, DSI_OK, when a round's T_delta has angle <= eps_rot and trans <= eps_trans (that T_delta is applied);
 *   - DSI_OK, not converged, after max_iterations rounds;
 *   - DSI_ERR_INVALID when a step matches fewer than min_matched cells, or its solve is refused: T_out is then the last
 *     good pose (T_init in the first round), info->stopped says which and info is filled as far as the loop got.
 * One synchronisation per round, for the moment block.  The per-cell correspondences of the last step stay for
 * dsx_map_align_fetch.  T_out may alias T_init. */
typedef struct dsx_map_align_info {
    int32_t iterations;  /* steps run */
    int32_t converged;   /* 1 or 0 */
    int32_t stopped;     /* 0: converged or out of rounds; 1: too few matched cells; 2: the solve was refused */
    int32_t reach;
    uint64_t n_cells;
    uint64_t n_matched_first, n_matched_last;
    double rms_first, rms_last;      /* solve's rms of the first and of the last step solved */
    double angle_last, trans_last;   /* of the last T_delta applied */
} dsx_map_align_info_t; /* 72 bytes */
/* Refusals as dsx_map_align_step's, plus max_iterations outside 1..64 and eps_rot or eps_trans not finite or < 0. */
DSI_API int dsx_map_align(dsi_map_t *a, dsi_map_t *b, const dsx_map_align_opts_t *opts, const double T_init[12], double T_out[12],
                          dsx_map_align_info_t *info);

/* ---- one map into another's frame ----
 * One integrate call (one `windows` stamp) on dst whose points are src's cells with n >= min_points && windows >=
 * min_windows, each as its float32 centroid (rule 5), under the pose T: bit for bit dsi_map_integrate of
 * dsi_map_extract(src, min_points, min_windows)'s xyz under T.  It runs on the device, through the routine every
 * integrate call goes through, and only the counts travel.  The leaves may differ.  *n_points (may be NULL): the cells
 * integrated; *n_rejected (may be NULL): those of them rejected by rule 3.  dst's table grows by the map's rule with the
 * call's point count bounded by src's occupied cells (no counting pass); a call that would need more than 2^27 slots by
 * that bound returns DSI_ERR_INVALID.  Refused before the GPU is touched, both maps unchanged: a NULL map or T, a
 * non-finite T, dst == src, maps of different contexts (DSI_ERR_CONTEXT), a table that overflowed earlier.  Like every
 * integrate call it invalidates dst's render, compare, classification and alignment; src keeps its own.  Synchronises. */
DSI_API int dsx_map_integrate_map(dsi_map_t *dst, dsi_map_t *src, const double T[12], uint32_t min_points, uint32_t min_windows,
                                  uint64_t *n_points, uint64_t *n_rejected);

#ifdef __cplusplus
}
#endif

#endif /* DSI_MAP_ALIGN_H */
