/*
 * dsi_engine.h -- C ABI of the MI355X-native DSI construction / fusion / arg-max
 * engine (libdsi_engine.so, hand-written HIP for gfx950).
 *
 * This is the drop-in boundary for the hot path of tub-rip/dvs_mcemvs:
 *     MapperEMVS::evaluateDSI -> fillVoxelGrid -> Grid3D::accumulateGridValueAt,
 *     Grid3D voxel-wise fusion, Grid3D::collapseMaxZSlice.
 * The reference has no FFI layer (it is one C++ process); each entry point below
 * names the reference C++ member it replaces (file:line relative to the
 * reference checkout).  include/dsi_engine.hpp re-creates the reference's class
 * and method names (Grid3D, EMVS::MapperEMVS, ...) on top of this ABI.
 *
 * Conventions
 *  - plain pointers and sizes only; every function returns a dsi_status_t
 *    (0 = ok) and never aborts or throws (the reference glog-CHECK-aborts);
 *    dsi_last_error() gives a thread-local message for the last failure.
 *  - volumes are fp32, layout volume[x + Nx*(y + Ny*z)] (cartesian3dgrid.h:34-35).
 *  - "host" pointers are ordinary CPU memory; "_dev" pointers are HIP device
 *    memory on the context's GPU.
 *  - all work of one context is issued on that context's HIP stream, in call
 *    order; functions that return host data synchronise, the others are
 *    asynchronous.  Distinct contexts may be used from distinct threads.
 *  - there is NO CPU fallback: creating a context fails when no gfx950 device
 *    (or no HIP device at all) is present.
 */
#ifndef DSI_ENGINE_H
#define DSI_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define DSI_API __attribute__((visibility("default")))
#else
#define DSI_API
#endif

#define DSI_ENGINE_ABI_VERSION 10
#define DSI_PACKET_SIZE 1024 /* mapper_emvs_stereo.hpp:152 packet_size_ */

typedef enum {
    DSI_OK = 0,
    DSI_ERR_INVALID = 1,       /* bad argument (null pointer, non-positive size, ...) */
    DSI_ERR_TOO_FEW_EVENTS = 2,/* evaluateDSI returns false: events.size() < 1024 (mapper_emvs_stereo.cpp:71-75) */
    DSI_ERR_HIP = 3,           /* a HIP runtime call failed */
    DSI_ERR_SHAPE = 4,         /* grids of different dimensions (reference: std::out_of_range from .at()) */
    DSI_ERR_BAD_OP = 5,        /* "Improper fusion method selected" (process1.cpp:155-157) */
    DSI_ERR_NO_DEVICE = 6,     /* no usable gfx950 GPU */
    DSI_ERR_CONTEXT = 7,       /* objects belong to different devices (or a batch to another context) */
    DSI_ERR_COMM = 8           /* RCCL could not be loaded or a collective call failed */
} dsi_status_t;

/* camera-fusion op codes = --stereo_fusion values (main.cpp:89, process1.cpp:136-158) */
typedef enum {
    DSI_FUSE_MIN = 1,  /* Grid3D::minTwoGrids            cartesian3dgrid.h:111-117 */
    DSI_FUSE_HM = 2,   /* Grid3D::harmonicMeanTwoGrids   cartesian3dgrid.h:119-127 */
    DSI_FUSE_GM = 3,   /* Grid3D::geometricMeanTwoGrids  cartesian3dgrid.h:150-156 */
    DSI_FUSE_AM = 4,   /* Grid3D::arithmeticMeanTwoGrids cartesian3dgrid.h:158-164 */
    DSI_FUSE_RMS = 5,  /* Grid3D::rmsTwoGrids            cartesian3dgrid.h:141-148 */
    DSI_FUSE_MAX = 6   /* Grid3D::maxTwoGrids            cartesian3dgrid.h:184-190 */
} dsi_fuse_op_t;

/* accumulate / finalize modes.  0 and 1 are the reference's temporal-fusion accumulators.
 * 2..5 are the n-ary forms of the 2-ary camera-fusion ops, which the reference does not have:
 * it applies GM / AM / RMS to two cameras only and silently ignores a third one
 * (process1.cpp:169-191).  They follow SURVEY.md 8(d) cfg 5 / 8(e): each is an accumulation
 * that is a plain sum, min or max over the maps -- i.e. directly an RCCL ncclSum / ncclMin /
 * ncclMax all-reduce across GPUs (dsi_acc_reduce_op) -- followed by a local finalize:
 *   LOG_SUM  acc += log v            finalize exp(acc / n)    geometric mean; 0 if any v is 0
 *   SQ_SUM   acc += v*v              finalize sqrt(acc / n)   root mean square
 *   MIN/MAX  acc = min/max(acc, v)   finalize: nothing
 * For n = 2: MIN / MAX / SUM(AM) equal the reference's 2-ary ops bit for bit; LOG_SUM equals
 * sqrt(a*g) (geometricMeanTwoGrids) within 16 ulp for values in [2^-20, 2^20] (1e-5 relative
 * over the whole float range: the accumulator is an fp32 sum of fp32 logarithms) and SQ_SUM
 * equals rmsTwoGrids within 2 ulp; tests/test_gpu_parity.py states and checks both.  log and exp
 * are spelled out in IEEE double operations, so GPU and CPU oracle agree bit for bit. */
typedef enum {
    DSI_ACC_SUM = 0,     /* addTwoGrids / computeAMfromSum            cartesian3dgrid.h:64-70, 87-93 */
    DSI_ACC_INV_SUM = 1, /* addInverseOfTwoGrids / computeHMfromSumOfInv cartesian3dgrid.h:72-86 */
    DSI_ACC_LOG_SUM = 2, /* n-ary geometricMeanTwoGrids               cartesian3dgrid.h:150-156 */
    DSI_ACC_SQ_SUM = 3,  /* n-ary rmsTwoGrids                         cartesian3dgrid.h:141-148 */
    DSI_ACC_MIN = 4,     /* n-ary minTwoGrids                         cartesian3dgrid.h:111-117 */
    DSI_ACC_MAX = 5,     /* n-ary maxTwoGrids                         cartesian3dgrid.h:184-190 */
    /* Only for the one-pass forms dsi_grid_fuse_n / dsi_mapper_depth_map_of_fusion_n with n = 2, 4 or 8 (not an
     * accumulation: dsi_grid_accumulate* / _finalize reject it): the geometric mean as the balanced TREE of the
     * reference's own 2-ary op, sqrt(sqrt(a b) sqrt(c d)) for n = 4 -- what calling geometricMeanTwoGrids
     * (cartesian3dgrid.h:150-156) on pairs of grids and then on the results gives, bit for bit (n = 2 IS that
     * member).  A plain HBM stream (~2 fp32 operations per source), where LOG_SUM costs ~100 fp64 operations. */
    DSI_ACC_GM_TREE = 6
} dsi_acc_mode_t;

/* how an accumulator of a given mode combines across GPUs */
typedef enum { DSI_REDUCE_SUM = 0, DSI_REDUCE_MIN = 1, DSI_REDUCE_MAX = 2 } dsi_reduce_op_t;

/* which voting kernel MapperEMVS::fillVoxelGrid is replaced by */
typedef enum {
    DSI_VOTE_AUTO = 0,
    DSI_VOTE_GLOBAL_ATOMIC = 1, /* thread = event, global_atomic_add_f32 into the DSI */
    DSI_VOTE_LDS_BANDS = 2,     /* plane x row-band privatised in LDS as Q33.31 fixed point (ds_add_u64), coalesced flush */
    DSI_VOTE_FUSED_ARGMAX = 3   /* reported only: the same bands, fused with the camera fusion and the arg-max
                                   (dsi_mapper_depth_map_of_events); not selectable with dsi_mapper_set_vote_algo */
} dsi_vote_algo_t;

typedef struct dsi_context dsi_context_t; /* one GPU + one HIP stream + scratch */
typedef struct dsi_grid dsi_grid_t;       /* device-resident Grid3D */
typedef struct dsi_mapper dsi_mapper_t;   /* device-resident MapperEMVS */
typedef struct dsi_batch dsi_batch_t;     /* device-resident, packetised events of one evaluateDSI call */

DSI_API const char *dsi_last_error(void);
DSI_API int dsi_abi_version(void);
/* 0: the production library (libdsi_engine.so).  1: the EXPERIMENTS flavour (libdsi_engine_experiments.so, built with
 * -DDSI_TIMING_EXPERIMENTS by `python -m dvs_mcemvs_amd.build --experiments`), which also reads the environment knobs
 * of the timing experiments quoted in NOTEBOOK.md and exports dsi_test_* hooks -- some of which make the DSIs WRONG on
 * purpose; never ship or benchmark it.  The production library reads no environment and exports no dsi_test_*. */
DSI_API int dsi_build_flavour(void);
/* number of HIP devices visible, or 0 (never fails) */
DSI_API int dsi_device_count(void);

/* ------------------------------------------------------------------ context */
DSI_API int dsi_context_create(int device_id, dsi_context_t **out);
/* fails with DSI_ERR_CONTEXT (and destroys nothing) while grids, mappers or batches created from the context are
 * alive: each holds a pointer to it.  Destroy them first. */
DSI_API int dsi_context_destroy(dsi_context_t *ctx);
DSI_API int dsi_context_synchronize(dsi_context_t *ctx);
/* the hipStream_t all work of this context is issued on */
DSI_API void *dsi_context_stream(dsi_context_t *ctx);
DSI_API int dsi_context_device(dsi_context_t *ctx);
/* device-side ordering between two contexts (streams) of one GPU: work queued on ctx after this call
 * starts only when everything queued on `other` before this call has finished.  The host does not
 * wait.  (The reference is single-threaded; this lets each MapperEMVS own a stream, e.g. the two
 * cameras of process_1, and meet at the fusion.) */
DSI_API int dsi_context_wait_for(dsi_context_t *ctx, dsi_context_t *other);
/* HIP-event stopwatch on the context's stream (bench.py: the replacement of the
 * std::chrono timers at process1.cpp:72-85,132-166). stop synchronises. */
DSI_API int dsi_context_timer_start(dsi_context_t *ctx);
DSI_API int dsi_context_timer_stop(dsi_context_t *ctx, float *elapsed_ms);
/* a timeline of HIP events on the context's stream: _mark records one (asynchronous); _read waits for the last
 * one, returns the n-1 intervals between consecutive marks in milliseconds (the first `capacity` of them) and
 * clears the timeline.  bench.py marks every step to report the spread of the per-step times. */
DSI_API int dsi_context_timeline_mark(dsi_context_t *ctx);
DSI_API int dsi_context_timeline_read(dsi_context_t *ctx, float *intervals_ms, size_t capacity, size_t *n_intervals);

/* ------------------------------------------------------------------- Grid3D */
/* Grid3D::Grid3D(dimX,dimY,dimZ) + allocate + resetGrid (cartesian3dgrid.cpp:30-46) */
DSI_API int dsi_grid_create(dsi_context_t *ctx, int nx, int ny, int nz, dsi_grid_t **out);
/* same, over caller-owned device memory of nx*ny*nz floats, 16-byte aligned (not zeroed, not freed) */
DSI_API int dsi_grid_wrap(dsi_context_t *ctx, int nx, int ny, int nz, void *data_dev, dsi_grid_t **out);
DSI_API int dsi_grid_destroy(dsi_grid_t *g);
/* Grid3D::getDimensions (cartesian3dgrid.h:230-235) */
DSI_API int dsi_grid_dims(const dsi_grid_t *g, int *nx, int *ny, int *nz);
/* Grid3D::resetGrid (cartesian3dgrid.cpp:67-70) */
DSI_API int dsi_grid_reset(dsi_grid_t *g);
/* Grid3D::getPointerToSlice(0) (cartesian3dgrid.h:237-240), as a device pointer */
DSI_API void *dsi_grid_device_ptr(dsi_grid_t *g);
DSI_API int dsi_grid_upload(dsi_grid_t *g, const float *host);
DSI_API int dsi_grid_download(dsi_grid_t *g, float *host);
/* dst = op(dst, src), in place, op in 1..6 (cartesian3dgrid.h:111-190) */
DSI_API int dsi_grid_fuse2(dsi_grid_t *dst, const dsi_grid_t *src, int op);
/* dst = op(a, b) in one pass: exactly what the reference's sequence
 * "dst.resetGrid(); dst.addTwoGrids(a); dst.<op>TwoGrids(b)" (process1.cpp:126-158,
 * process2.cpp:159-189) leaves in dst, without the two extra sweeps over the volume */
DSI_API int dsi_grid_fuse2_into(dsi_grid_t *dst, const dsi_grid_t *a, const dsi_grid_t *b, int op);
/* Grid3D::harmonicMeanTwoGrids(grid2, n) (cartesian3dgrid.h:130-139) */
DSI_API int dsi_grid_fuse_hm_n(dsi_grid_t *dst, const dsi_grid_t *src, int n);
/* dst = identity element of the mode: 0 for the four sums (what the reference's resetGrid()
 * before the temporal loop does, process2.cpp:203), +inf for MIN, -inf for MAX */
DSI_API int dsi_grid_accumulate_begin(dsi_grid_t *dst, int mode);
/* Grid3D::addTwoGrids / addInverseOfTwoGrids (cartesian3dgrid.h:64-78) and the n-ary modes,
 * mode = dsi_acc_mode_t */
DSI_API int dsi_grid_accumulate(dsi_grid_t *dst, const dsi_grid_t *src, int mode);
/* Grid3D::computeAMfromSum / computeHMfromSumOfInv (cartesian3dgrid.h:80-93) and the n-ary modes */
DSI_API int dsi_grid_finalize(dsi_grid_t *dst, int mode, int n);
/* dst = n-ary fusion of srcs[0..n) in ONE pass over the volumes: exactly dsi_grid_accumulate_begin(dst,
 * mode); dsi_grid_accumulate(dst, srcs[i], mode) for i = 0..n-1; dsi_grid_finalize(dst, mode, n) -- same
 * operations in the same order, hence the same bits -- with (n+1)*4 instead of (3n+2)*4 bytes of
 * traffic per voxel.  2 <= n <= 8; dst must not be one of the sources. */
DSI_API int dsi_grid_fuse_n(dsi_grid_t *dst, const dsi_grid_t *const *srcs, int n, int mode);
/* dsi_reduce_op_t of a mode (never fails for a valid mode; -1 otherwise) */
DSI_API int dsi_acc_reduce_op(int mode);
/* Grid3D::collapseMaxZSlice (cartesian3dgrid.cpp:115-137): conf[ny*nx] f32,
 * idx[ny*nx] u8, first maximum wins.  Host outputs; synchronises. */
DSI_API int dsi_grid_collapse_max_z(dsi_grid_t *g, float *conf_host, uint8_t *idx_host);
/* same, device outputs, asynchronous.  planes_dev (nz floats) + depth_dev may be
 * NULL; when given, depth_dev[p] = planes_dev[idx[p]]
 * (MapperEMVS::convertDepthIndicesToValues, mapper_emvs_stereo.cpp:302-313). */
DSI_API int dsi_grid_collapse_max_z_dev(dsi_grid_t *g, float *conf_dev, uint8_t *idx_dev,
                                const float *planes_dev, float *depth_dev);
/* Grid3D::computeMeanSquare (cartesian3dgrid.cpp:164-174), accumulated in double */
DSI_API int dsi_grid_mean_square(dsi_grid_t *g, double *out);

/* focus measures of getDepthMapFromDSI's `method` switch (mapper_emvs_stereo.cpp:348-364) */
typedef enum {
    DSI_FOCUS_LOCAL_VAR = 0,   /* Grid3D::collapseZSliceByLocalVar         cartesian3dgrid.cpp:327-365 */
    DSI_FOCUS_LOCAL_MS = 1,    /* Grid3D::collapseZSliceByLocalMeanSquare  cartesian3dgrid.cpp:368-402 */
    DSI_FOCUS_GRAD_MAG = 2,    /* Grid3D::collapseZSliceByGradMag          cartesian3dgrid.cpp:192-244 */
    DSI_FOCUS_LAPLACIAN = 3,   /* Grid3D::collapseZSliceByLaplacianMag     cartesian3dgrid.cpp:247-284 */
    DSI_FOCUS_DOG = 4          /* Grid3D::collapseZSliceByDoG              cartesian3dgrid.cpp:287-324 */
} dsi_focus_method_t;
/* Focus-based collapse: per z-slice a 2-D focus measure, then the first plane of strictly largest focus per pixel
 * (conf starts at +0 and idx at 0: values <= 0 and NaN are never taken); GradMag and LaplacianMag return the square
 * root of the selected focus.  Arithmetic: DESIGN.md "Focus-based collapses".  half_patchsize (0..8, else
 * DSI_ERR_INVALID) is read by GradMag only (the reference's default is 1).  method outside 0..4: DSI_ERR_BAD_OP;
 * dimZ > 256: DSI_ERR_INVALID (u8 indices).  Host outputs conf[ny*nx] f32, idx[ny*nx] u8; synchronises. */
DSI_API int dsi_grid_collapse_focus(dsi_grid_t *g, int method, int half_patchsize, float *conf_host, uint8_t *idx_host);
/* same, device outputs, asynchronous; planes_dev / depth_dev as dsi_grid_collapse_max_z_dev */
DSI_API int dsi_grid_collapse_focus_dev(dsi_grid_t *g, int method, int half_patchsize, float *conf_dev, uint8_t *idx_dev,
                                        const float *planes_dev, float *depth_dev);
/* Grid3D::collapseMinZSlice (cartesian3dgrid.cpp:139-161): val[ny*nx] f32, idx[ny*nx] u8, first minimum wins
 * (std::min_element).  dimZ > 256: DSI_ERR_INVALID.  Host outputs; synchronises. */
DSI_API int dsi_grid_collapse_min_z(dsi_grid_t *g, float *val_host, uint8_t *idx_host);
/* Grid3D::computeLocalFocusInPlace (cartesian3dgrid.cpp:417-483): dst = per z-slice local focus of src --
 * focus_method 1 the Gaussian (sigma 0.5) local mean square, any other value the local standard deviation.
 * dst == src is the reference's in-place call: the result is written to a scratch volume of dst's context and copied
 * back, so no reader of the grid sees it half written.  Same shape, same device.  Asynchronous. */
DSI_API int dsi_grid_local_focus(dsi_grid_t *dst, const dsi_grid_t *src, int focus_method);

/* ---- the rest of Grid3D (arithmetic and definitions: DESIGN.md 7d) ---- */
/* Voxel-wise members that are NOT camera fusions (no --stereo_fusion value selects them): their own enum; dsi_fuse_op_t and
 * every call that takes it are unchanged. */
typedef enum {
    DSI_GRID_OP_SUBTRACT = 1,       /* Grid3D::subtractTwoGrids       cartesian3dgrid.h:95-101   a - g */
    DSI_GRID_OP_RATIO = 2,          /* Grid3D::ratioTwoGrids          cartesian3dgrid.h:103-109  a / (|g| + 0.1f), in double */
    DSI_GRID_OP_QUADRATIC_MEAN = 3, /* Grid3D::quadraticMeanTwoGrids  cartesian3dgrid.h:166-174  sqrt(0.5 (a a + g g)) */
    DSI_GRID_OP_CUBIC_MEAN = 4      /* Grid3D::cubicMeanTwoGrids      cartesian3dgrid.h:176-184  cbrt(0.5 (a a a + g g g)) */
} dsi_grid_op_t;
/* dst = op(dst, src), in place, op = dsi_grid_op_t.  dst == src is legal and gives op(a, a) (the reference takes grid2 by
 * value).  DSI_ERR_SHAPE: different dimensions; DSI_ERR_CONTEXT: different devices; DSI_ERR_BAD_OP: op not in 1..4. */
DSI_API int dsi_grid_binary_op(dsi_grid_t *dst, const dsi_grid_t *src, int op);
/* Grid3D::getMinMax (cartesian3dgrid.cpp:177-188) = std::minmax_element over the flat array: the FIRST smallest and the
 * LAST largest element; -0.f == +0.f, so position decides and the value returned carries that element's bits.  min_pos /
 * max_pos may be NULL.  A volume holding NaN gives an unspecified result (still DSI_OK).  Synchronises. */
DSI_API int dsi_grid_min_max(dsi_grid_t *g, float *min_val, float *max_val, uint64_t *min_pos, uint64_t *max_pos);
/* Grid3D::getSlice (cartesian3dgrid.cpp:72-113), row-major rows x cols floats:
 *   dim_idx 0: ny x nz, out[v*nz+u] = vol(slice, v, u);  1: nx x nz, out[v*nz+u] = vol(v, slice, u);  2: the ny x nx plane.
 * dim_idx > 2 or slice_idx outside the dimension: DSI_ERR_INVALID.  Host output; synchronises. */
DSI_API int dsi_grid_get_slice(dsi_grid_t *g, unsigned slice_idx, unsigned dim_idx, float *slice_host);
/* same, device output, asynchronous */
DSI_API int dsi_grid_get_slice_dev(dsi_grid_t *g, unsigned slice_idx, unsigned dim_idx, float *slice_dev);
/* Grid3D::accumulateZSliceAt (cartesian3dgrid.h:195-204): vol(ix, iy, iz) += img(iy, ix) for iy < rows, ix < cols (row-major
 * host image).  rows <= ny, cols <= nx, iz < nz, else DSI_ERR_INVALID; an image smaller than the plane is legal. */
DSI_API int dsi_grid_accumulate_z_slice(dsi_grid_t *g, unsigned iz, const float *img_host, int rows, int cols);
/* Grid3D::getGridValueAt(p) / setGridValueAt / accumulateGridValueAt(p, fval) (cartesian3dgrid.h:40-58): single voxels,
 * ordered on the context's stream; p >= nx*ny*nz: DSI_ERR_INVALID (the reference: std::out_of_range).  Synchronise. */
DSI_API int dsi_grid_value_at(dsi_grid_t *g, uint64_t p, float *out);
DSI_API int dsi_grid_set_value_at(dsi_grid_t *g, uint64_t p, float v);
DSI_API int dsi_grid_accumulate_value_at(dsi_grid_t *g, uint64_t p, float v);
/* What Grid3D::imwriteSlices (cartesian3dgrid_IO.cpp:39-76) computes before it writes files: EVERY slice of one orientation
 * as an 8-bit image, slice after slice, each of dsi_grid_get_slice's shape -- nx*ny*nz bytes.  normalize_by_minmax != 0:
 * (v - min) / (max - min) * 255 with the volume's extremes; 0: cv::normalize(NORM_MINMAX, 0, 255) per slice.  Rounded to
 * nearest (ties to even), clamped to 0..255, NaN -> 0.  dim_idx > 2: DSI_ERR_INVALID.  Host output; synchronises. */
DSI_API int dsi_grid_slices_u8(dsi_grid_t *g, unsigned dim_idx, int normalize_by_minmax, uint8_t *out_host);
/* same, device output (4-byte aligned, else DSI_ERR_INVALID), asynchronous */
DSI_API int dsi_grid_slices_u8_dev(dsi_grid_t *g, unsigned dim_idx, int normalize_by_minmax, uint8_t *out_dev);

/* ---- volume filters: cartesian3dgrid_filter.cpp and gaussianiir3d.cpp (arithmetic and kernels: DESIGN.md 7i) ----
 * Each result lands in the grid's own storage (dsi_grid_device_ptr does not change; a second volume, where one is needed,
 * is scratch of the grid's context).  Every product is an fp32 multiply rounded on its own, then an fp32 add, subnormals
 * included: bit for bit what the reference's CPU loops compute.  Asynchronous unless stated. */
/* Grid3D::laplacianInPlace (laplacian3D, cartesian3dgrid_filter.cpp:72-110): per voxel Dxx = (v[+x] - 2 v) + v[-x], likewise
 * Dyy, Dzz, neighbours by index clamping (homogeneous Neumann); the voxel becomes (Dxx + Dyy) + Dzz. */
DSI_API int dsi_grid_laplacian(dsi_grid_t *g);
/* Grid3D::smoothInPlace (diffuse, cartesian3dgrid_filter.cpp:19-69): explicit Euler steps v + dt ((Dxx + Dyy) + Dzz) of the heat
 * equation, in fp32 dt = min(0.5f / 12.f, 0.5f t) with t = 0.5f sigma sigma, ceil(t / dt) steps, each from the previous step's
 * volume.  steps_out (may be NULL) receives the step count.  sigma <= 0 or not finite (the reference divides 0 by 0 there),
 * sigma so small that sigma^2 underflows, or more than 1e6 steps (sigma > 288): DSI_ERR_INVALID. */
DSI_API int dsi_grid_smooth_diffuse(dsi_grid_t *g, float sigma, int *steps_out);
/* Grid3D::smoothInPlaceIIR3D = the 3-sigma gaussianiir3d (gaussianiir3d.cpp:143-251; the member passes numsteps = 3):
 * Alvarez-Mazorra recursive Gaussian, per line and step p[0] *= b; p[i] += nu p[i-1]; p[n-1] *= b; p[i-1] += nu p[i]; x lines,
 * then y, then z, then every voxel times the fp32 product of the axes' post-scales.  The recurrence is evaluated sequentially
 * along every line.  Any sigma <= 0 or numsteps <= 0: the grid is left unchanged, DSI_OK (the reference returns silently);
 * numsteps > 16: DSI_ERR_INVALID. */
DSI_API int dsi_grid_smooth_iir(dsi_grid_t *g, float sigma_x, float sigma_y, float sigma_z, int numsteps);
/* computeMeanStd, which the reference calls and never defines; here: mean = sum v / N and stddev = sqrt(sum (v - mean)^2 / N)
 * (two passes, population deviation), accumulated in double over a fixed tree: two calls return the same bits.  Synchronises. */
DSI_API int dsi_grid_mean_std(dsi_grid_t *g, double *mean, double *stddev);
/* Grid3D::computeMoranIndexGaussianWeights (cartesian3dgrid_filter.cpp:113-199): spatial autocorrelation of the grid under
 * Gaussian weights.  sigma < 0.2 becomes 0.2f; z = the standardized grid (fp32), s = z through the IIR filter (sigma, sigma,
 * sigma, 3 steps), c = the centre of a unit impulse in a k^3 volume through the same filter, k = 2 (2 ceil(3 sigma)) + 1;
 * I = sum z (s - c z) / ((1 - c)(N - 1) + 1e-6), the sum in double.  The grid is not modified.  A grid of zero (or non-finite)
 * deviation, NaN or sigma >= 1000: DSI_ERR_INVALID.  Synchronises. */
DSI_API int dsi_grid_moran_index(dsi_grid_t *g, float sigma, double *out);

/* ---------------------------------------------------------- multi-GPU (RCCL) */
/* The temporal fusion of process_2 (process2.cpp:211-242: one accumulate per sub-interval, one
 * finalize) and of the sliding window (main.cpp:177) shards by time slice: every GPU accumulates
 * its slices locally, then ONE all-reduce of the accumulator over xGMI replaces the rest of the
 * loop.  The engine calls RCCL itself (librccl is loaded on first use; nothing
 * above this ABI needs torch or MPI).  Two ways to form a communicator:
 *   - one process, n GPUs (the reference is one process): dsi_comm_create_all over n contexts on n
 *     distinct devices; collectives through the *_all entry points (one group call);
 *   - one process per GPU: rank 0 calls dsi_comm_unique_id and hands the 128 bytes to the other
 *     ranks by any side channel (file, socket, MPI, a torch.distributed store), then every rank
 *     calls dsi_comm_create_rank.
 * A collective on a grid is issued on that grid's context stream, ordered like any other grid
 * operation; the host does not wait. */
typedef struct dsi_comm dsi_comm_t;
#define DSI_COMM_ID_BYTES 128
DSI_API int dsi_comm_unique_id(uint8_t id[DSI_COMM_ID_BYTES]);
DSI_API int dsi_comm_create_rank(dsi_context_t *ctx, const uint8_t id[DSI_COMM_ID_BYTES], int nranks, int rank,
                                 dsi_comm_t **out);
/* out receives n communicators, out[i] on contexts[i]'s device (n distinct devices) */
DSI_API int dsi_comm_create_all(dsi_context_t *const *contexts, int n, dsi_comm_t **out);
DSI_API int dsi_comm_destroy(dsi_comm_t *comm);
DSI_API int dsi_comm_rank(const dsi_comm_t *comm);
DSI_API int dsi_comm_size(const dsi_comm_t *comm);
/* what RCCL ITSELF reports for this communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), as opposed
 * to what it was created with: bench.py prints it per rank as the proof of the rank count.  Any pointer may be NULL. */
DSI_API int dsi_comm_query(const dsi_comm_t *comm, int *nranks, int *rank, int *device);
/* in-place all-reduce of a grid over the communicator, op = dsi_reduce_op_t (use
 * dsi_acc_reduce_op(mode) for an accumulator).  The grid must live on the communicator's device. */
DSI_API int dsi_grid_allreduce(dsi_comm_t *comm, dsi_grid_t *g, int op);
/* the same for the n ranks of one process (comms from dsi_comm_create_all, grids[i] on comms[i]) */
DSI_API int dsi_grid_allreduce_all(dsi_comm_t *const *comms, dsi_grid_t *const *grids, int n, int op);

/* --------------------------------------------------------------- MapperEMVS */
typedef struct {
    int sensor_width;   /* cam.fullResolution() (mapper_emvs_stereo.cpp:34-36) */
    int sensor_height;
    float K[4];         /* fx, fy, cx, cy of the projection matrix (mapper_emvs_stereo.cpp:46-48) */
    int dim_x;          /* ShapeDSI (mapper_emvs_stereo.hpp:40-65); 0 = sensor size (:216-217) */
    int dim_y;
    int dim_z;          /* <= 256 (main.cpp:156) */
    float min_depth;
    float max_depth;
    float fov_deg;      /* < 10: use the camera focal length (mapper_emvs_stereo.cpp:219-229) */
    int inverse_depth;  /* 0: LinearDepthVector (CMake default), 1: -DUSE_INVERSE_DEPTH */
    const float *lut;   /* host, 2*W*H floats, entry y*W+x = undistorted (u,v)
                           (precomputeRectifiedPoints, mapper_emvs_stereo.cpp:256-299); NULL = identity */
    /* Plane sharding (multi-GPU): this mapper owns planes
     * [plane_begin, plane_begin + plane_count) of the dim_z planes defined above; its DSI has
     * plane_count planes.  z0 stays plane 0 of the FULL depth vector (mapper_emvs_stereo.cpp:111,163)
     * and planes are independent in fillVoxelGrid (:168), so the shard's DSI equals those planes of
     * the unsharded DSI bit for bit.  plane_count == 0: all planes from plane_begin on. */
    int plane_begin;
    int plane_count;
} dsi_mapper_config_t;

/* MapperEMVS::MapperEMVS(cam, dsi_shape) (mapper_emvs_stereo.cpp:29-64, setupDSI :208-241) */
DSI_API int dsi_mapper_create(dsi_context_t *ctx, const dsi_mapper_config_t *cfg, dsi_mapper_t **out);
DSI_API int dsi_mapper_destroy(dsi_mapper_t *m);
/* public member MapperEMVS::dsi_ (mapper_emvs_stereo.hpp:116); owned by the mapper */
DSI_API dsi_grid_t *dsi_mapper_grid(dsi_mapper_t *m);
/* virtual camera {fx,fy,cx,cy} (:231-239), plane depths raw_depths_vec_ (:213-214;
 * raw_depths needs dim_z floats) and the resolved dimensions; any pointer may be NULL */
DSI_API int dsi_mapper_geometry(const dsi_mapper_t *m, float *Kv, float *raw_depths, int *nx, int *ny, int *nz);
/* first plane this mapper owns (0 unless plane-sharded); raw_depths / nz above describe the owned planes */
DSI_API int dsi_mapper_plane_begin(const dsi_mapper_t *m);
/* the WHOLE depth vector of the ShapeDSI (dim_z floats; global arg-max index -> depth of a plane-sharded
 * DSI); either pointer may be NULL */
DSI_API int dsi_mapper_full_depths(const dsi_mapper_t *m, float *raw_depths, int *dim_z);
DSI_API int dsi_mapper_set_vote_algo(dsi_mapper_t *m, int algo);
/* tuning knobs of DSI_VOTE_LDS_BANDS; 0 = automatic */
DSI_API int dsi_mapper_set_band_params(dsi_mapper_t *m, int band_rows, int chunks, int block_threads);
/* DSI_VOTE_LDS_BANDS has two lane mappings: one packet's run per wave pass (long runs) or the
 * runs of 64 packets packed back to back into the lanes (short runs: wide / tall grids).
 * mode -1 = automatic (by expected run length: 7 or 5), 0 = per packet, 1 = packed,
 * 2 = groups of consecutive packets sorted together (one long run per group),
 * 3 = packed with the compiled (not hand-scheduled) wave loop, for A/B tests,
 * 4 = groups with the hand-scheduled wave loop (long runs for wide grids),
 * 5 = packed with a vector (prefix-sum + tail-bit) slot -> record mapping instead of the scalar run
 *     bookkeeping (short runs: wide grids), hand-scheduled batches,
 * 6 = mapping 5 all compiled, for A/B tests,
 * 7 = mapping 1 with DEALT passes: the waves of a workgroup draw their passes from a counter instead of taking
 *     every 16th one (the automatic choice wherever mapping 1 used to be chosen),
 * 8 = OPT-IN, never chosen automatically: mapping 7 on PAIRED 32-bit cells -- one 64-bit LDS atomic updates the two cells
 *     (x, x + 1) of a row, a vote is two atomics instead of four (the voting kernels are bound by the LDS atomic unit).
 *     The price is the numerical contract: the weights of cartesian3dgrid.h:261-270 are added as ROUNDED Q.19 integers
 *     (error <= 2^-20 per vote, about that of the reference's own fp32 "+=") instead of the exact Q33.31 sums every other
 *     mapping keeps -- a record whose weight on a cell is below 2^-20 adds nothing, so bursts of events on one sub-pixel
 *     location can lose up to 2^-20 per record on the neighbouring cells --, the DSI is no longer bit-identical to
 *     theirs, and a 32-bit cell holds 8,192 full votes per work
 *     item: the voting kernel reports any cell that reached HALF of that (dsi_mapper_paired_overflow), in which case the
 *     caller repeats the call with another mapping.  1024-thread workgroups, the evaluate / fillVoxelGrid path only. */
DSI_API int dsi_mapper_set_packed_lanes(dsi_mapper_t *m, int mode);
/* lane mapping 8: *overflowed <- 1 if a paired cell of the last vote reached 2^31 (4,096 full votes: half its capacity;
 * beyond 8,192 a cell wraps, so a set flag means "the DSI may be wrong, vote again with an exact mapping").  0 for every
 * other mapping.  Synchronises. */
DSI_API int dsi_mapper_paired_overflow(dsi_mapper_t *m, int *overflowed);
/* Lane mappings 5 / 6 (wide grids) read, per (band, plane, packet), the run of the packet's records the band must look
 * at.  As a table that is bands x planes x packets words -- 6.1 GB per camera at 1024 x 1024 x 256 with 100 M events, 3.9 ms to
 * write -- so from min_packets packets per call on the voting kernel derives the runs itself, per pass, from the
 * packets' transposed row tables (the same runs: fillVoxelGrid's loop mapper_emvs_stereo.cpp:168-203 visits the same
 * events either way, and the DSI is bit-identical).  min_packets < 0 = the default (8192), 0 = always, a huge value = never. */
DSI_API int dsi_mapper_set_inline_cuts(dsi_mapper_t *m, long long min_packets);

/* MapperEMVS::fillVoxelGrid(event_locations_z0, camera_centers)
 * (mapper_emvs_stereo.cpp:151-205) -- the exact-parity test point.  xy_z0: 2 floats
 * per event (elements [0],[1] of each Vector4f), n_packets*1024 events; centers: 3
 * floats per packet.  Host inputs.  Accumulates into the mapper's grid WITHOUT
 * resetting it (the reset is evaluateDSI's, :145). */
DSI_API int dsi_mapper_fill_voxel_grid(dsi_mapper_t *m, const float *xy_z0, const float *centers, size_t n_packets);

/* Device-resident input of one evaluateDSI call: raw events (pixel x,y; timestamps are not needed
 * past packetisation, and polarity only by dsi_batch_event_image, which takes it separately) plus the packetisation done by
 * mapper_emvs_stereo.cpp:88-105: packet k covers events
 * [packet_first[k], packet_first[k]+1024) (packet_first == NULL: k*1024) and has
 * pose Rt[12k..12k+11] = R (row-major 3x3) then t of T_ev_rv, already cast to float.
 * An event whose pixel lies outside the sensor of the mapper that evaluates the batch has no
 * rectification-LUT entry (the reference would index past its matrix, :134); with a LUT it is
 * dropped -- it votes on no plane -- instead of being looked up out of bounds. */
DSI_API int dsi_batch_create(dsi_context_t *ctx, const uint16_t *x, const uint16_t *y, size_t n_events,
                     const uint32_t *packet_first, const float *Rt, size_t n_packets, dsi_batch_t **out);
/* Host-fed streams (a 50 ms window every 50 ms, main.cpp:177): page-locked host memory lets the
 * upload run as one DMA without the runtime's staging copies, and lets the host go on while it
 * runs.  dsi_host_alloc returns such memory (hipHostMalloc; any context of the process may use it).
 * dsi_batch_create_async is dsi_batch_create for arrays that live in it: it returns as soon as the
 * copies are queued on the copy stream.  The arrays must stay unchanged until the upload is done --
 * dsi_batch_uploaded(b) (non-blocking: 1 done, 0 in flight), or any later synchronisation of a
 * context that evaluated the batch. */
DSI_API int dsi_host_alloc(size_t bytes, void **out);
DSI_API int dsi_host_free(void *p);
DSI_API int dsi_batch_create_async(dsi_context_t *ctx, const uint16_t *x, const uint16_t *y, size_t n_events,
                           const uint32_t *packet_first, const float *Rt, size_t n_packets, dsi_batch_t **out);
DSI_API int dsi_batch_uploaded(const dsi_batch_t *b);
DSI_API int dsi_batch_destroy(dsi_batch_t *b);
DSI_API size_t dsi_batch_num_packets(const dsi_batch_t *b);

/* MapperEMVS::evaluateDSI past the pose lookup: per-packet camera centre and H_z0
 * (:108-126), per-event LUT + z0 warp (:129-142), resetGrid (:145), fillVoxelGrid
 * (:146).  Asynchronous on the context's stream. */
DSI_API int dsi_mapper_evaluate_batch(dsi_mapper_t *m, const dsi_batch_t *batch);

/* MapperEMVS::evaluateDSI(events, trajectory, T_rv_w) (mapper_emvs_stereo.cpp:67-148),
 * host inputs.  Events: pixel coordinates and timestamps in seconds, time-sorted.
 * Trajectory: n_poses control poses T_w_c as {tx,ty,tz,qw,qx,qy,qz} at ascending
 * times (LinearTrajectory, trajectory.hpp:81-128; SE(3) interpolation with
 * minkindr semantics).  T_rv_w: same 7-double layout.  Returns
 * DSI_ERR_TOO_FEW_EVENTS where the reference returns false.  n_voted (optional)
 * receives the number of events actually voted (packets * 1024). */
DSI_API int dsi_mapper_evaluate(dsi_mapper_t *m, const uint16_t *x, const uint16_t *y, const double *ts,
                        size_t n_events, const double *traj_times, const double *traj_poses,
                        size_t n_poses, const double *T_rv_w, size_t *n_voted);

/* host-side packetisation + pose pipeline of evaluateDSI, exposed so that callers can
 * build a dsi_batch_t once and keep it resident.  packet_first (capacity
 * n_events/1024+1) and Rt (12 floats per packet) are outputs; *n_packets the count.
 * Returns DSI_ERR_TOO_FEW_EVENTS for n_events < 1024. */
DSI_API int dsi_packetize(const double *ts, size_t n_events, const double *traj_times,
                  const double *traj_poses, size_t n_poses, const double *T_rv_w,
                  uint32_t *packet_first, float *Rt, size_t *n_packets);
/* the same with the timestamps read where they lie in an array of structs (the reference holds
 * std::vector<dvs_msgs::Event>, mapper_emvs_stereo.cpp:91: events[current_event_ + packet_size_/2].ts): event i's
 * timestamp is the double at ts_first + i * stride_bytes.  Only one timestamp per packet is read (mapper_emvs_stereo.cpp:88-99),
 * so a caller need not copy n_events doubles out of its structs first. */
DSI_API int dsi_packetize_strided(const void *ts_first, size_t stride_bytes, size_t n_events, const double *traj_times,
                          const double *traj_poses, size_t n_poses, const double *T_rv_w,
                          uint32_t *packet_first, float *Rt, size_t *n_packets);
/* LinearTrajectory::getPoseAt (trajectory.hpp:92-126); returns DSI_ERR_INVALID when
 * the reference returns false (no extrapolation). out = 7 doubles. */
DSI_API int dsi_pose_at(const double *traj_times, const double *traj_poses, size_t n_poses, double t, double *out);

/* arg-max + depth of the mapper's own grid: collapseMaxZSlice (cartesian3dgrid.cpp:115-137)
 * + convertDepthIndicesToValues (mapper_emvs_stereo.cpp:302-313) applied to the raw
 * (pre-filter) indices.  Host outputs (any may be NULL); synchronises. */
DSI_API int dsi_mapper_depth_map(dsi_mapper_t *m, float *depth_host, float *conf_host, uint8_t *idx_host);
/* the same for any grid of the mapper's shape (e.g. a fused DSI); asynchronous variant
 * keeps results in the mapper's device buffers until dsi_mapper_fetch_depth_map */
DSI_API int dsi_mapper_depth_map_of(dsi_mapper_t *m, dsi_grid_t *g);
/* getDepthMapFromDSI's switch (mapper_emvs_stereo.cpp:348-369): method 0..4 (dsi_focus_method_t; GradMag with
 * half_patchsize 1, the reference's default) is the focus-based collapse of g + convertDepthIndicesToValues, any
 * other value exactly dsi_mapper_depth_map_of(m, g).  The raw map stays in the mapper like dsi_mapper_depth_map_of's
 * (dsi_mapper_filter_depth_map / dsi_mapper_fetch_depth_map apply unchanged). */
DSI_API int dsi_mapper_depth_map_of_focus(dsi_mapper_t *m, dsi_grid_t *g, int method);
/* depth map of op(a, b) (op = dsi_fuse_op_t) WITHOUT materialising the fused DSI: exactly what
 * "fused.resetGrid(); fused.addTwoGrids(a); fused.<op>TwoGrids(b)" (process1.cpp:126-158) followed by
 * dsi_mapper_depth_map_of(m, fused) gives, bit for bit, in one pass over a and b.  For streams of
 * windows that only keep the depth map (main.cpp:177-302). */
DSI_API int dsi_mapper_depth_map_of_fusion(dsi_mapper_t *m, const dsi_grid_t *a, const dsi_grid_t *b, int op);
/* the n-ary form: depth map of dsi_grid_fuse_n(srcs, n, mode) (mode = dsi_acc_mode_t; the n-camera
 * generalisation of process1.cpp:126-191, SURVEY 8d cfg 5) without materialising the fused DSI --
 * the same per-voxel operations in the same order, so the same bits as fuse-then-collapse. */
DSI_API int dsi_mapper_depth_map_of_fusion_n(dsi_mapper_t *m, const dsi_grid_t *const *srcs, int n, int mode);
/* The depth map of n = 1, 2 or 3 cameras' events WITHOUT building their DSIs: bit for bit what
 *     for c in 0..n-1: dsi_mapper_evaluate_batch(mappers[c], batches[c]);                 (process1.cpp:76-117)
 *     n == 2: dsi_mapper_depth_map_of_fusion(out, grid(mappers[0]), grid(mappers[1]), op);  (:126-166, :222 -> mapper_emvs_stereo.cpp:368)
 *     n == 1: dsi_mapper_depth_map_of(out, grid(mappers[0]))
 *     n == 3: the trinocular rig of process1.cpp:105-117, :169-191 -- fused = op(grid 0, grid 1), then
 *             op 1: min(fused, grid 2), op 2: harmonicMeanTwoGrids(grid 2, 3), op 6: max(fused, grid 2),
 *             ops 3, 4, 5: camera 2 is ignored like the reference does ("case 3: break;"), its events are
 *             not even voted -- followed by dsi_mapper_depth_map_of(out, fused)
 * leaves in out's depth-map buffers (dsi_mapper_fetch_depth_map*), computed by one kernel that votes a
 * (band, plane) of each camera into LDS, applies the 2-ary op per voxel and keeps the running arg-max
 * in registers -- no DSI is written or read (at 512x512x200 a window saves 840 MB of HBM traffic).  For
 * streams that keep only the depth maps (the --full_seq loop, main.cpp:177-302).  The mappers' grids
 * are NOT touched (they keep whatever an earlier evaluate left there); `out` may be one of the
 * mappers; all must share one context and one DSI shape; the cameras need distinct mappers.  op =
 * dsi_fuse_op_t (ignored for n == 1).  A batch without packets stands for an all-zero DSI (evaluateDSI
 * returned false, mapper_emvs_stereo.cpp:71-75).  Asynchronous on the context's stream. */
DSI_API int dsi_mapper_depth_map_of_events(dsi_mapper_t *out, dsi_mapper_t *const *mappers,
                                           const dsi_batch_t *const *batches, int n, int op);
/* The same for the n-camera rigs the reference's process_1 has no switch for (BASELINE configs[4]: four cameras,
 * geometric mean): bit for bit what
 *     for c in 0..n-1: dsi_mapper_evaluate_batch(mappers[c], batches[c]);
 *     dsi_mapper_depth_map_of_fusion_n(out, {grid(mappers[c])}, n, mode)
 * leaves in out's depth-map buffers, by the one kernel that votes, fuses and keeps the running arg-max -- no DSI written
 * (at 1024 x 1024 x 256: 4 GiB not written and not read back).  mode = DSI_ACC_GM_TREE, the balanced tree of
 * Grid3D::geometricMeanTwoGrids (cartesian3dgrid.h:150-156): sqrt(sqrt(c0 c1) sqrt(c2 c3)); n = 4, or 2 (where the tree IS
 * the reference's 2-ary op).  Everything else as dsi_mapper_depth_map_of_events. */
DSI_API int dsi_mapper_depth_map_of_events_n(dsi_mapper_t *out, dsi_mapper_t *const *mappers,
                                             const dsi_batch_t *const *batches, int n, int mode);
/* Alg. 2 of one window (process_2 / process_5, process2.cpp:98-289) without a DSI: bit for bit the depth maps of
 * mapper_fused.dsi_ ("time_camera") and of mapper_fused_camera_time.dsi_ ("camera_time") after the reference's
 *     for k in 0..n_sub-1: evaluateDSI(camera 0, batches[2k]); evaluateDSI(camera 1, batches[2k+1]);
 *                          s_k = fuse(0 + dsi0, dsi1) by stereo_fusion; temporal accumulation of s_k, dsi0, dsi1
 *     finalisation (temporal_fusion 2: n_sub / sum of 1 / (0.01 + x), 4: sum / n_sub; 1, 3, 5, 6: all grids stay zero)
 *     camera_time = fuse(0 + left, right) by the converse switch (stereo_fusion 3 and 4 swapped, process2.cpp:266-289)
 * computed by one kernel that votes the 2 n_sub batches of each (band, plane) into LDS and keeps the accumulators and the
 * running arg-max in registers.  cams[0] / cams[1]: the two cameras' mappers (calibration; their grids are not touched);
 * batches: k-major, packetised against T_rv_w = T_w_l(ts)^-1 (dsi_alg2_subintervals gives the event ranges);
 * out_camera_time NULL: camera_time is not computed.  n_sub 1..8.  The batches' tables live in scratch of
 * out_time_camera.  Results stay in the output mappers' depth-map buffers (dsi_mapper_fetch_depth_map*,
 * dsi_mapper_filter_depth_map, dsi_mapper_get_pointcloud).  DSI_ERR_BAD_OP: stereo_fusion not in 1..6; DSI_ERR_INVALID:
 * n_sub not in 1..8 or a NULL argument; DSI_ERR_SHAPE / DSI_ERR_CONTEXT as dsi_mapper_depth_map_of_events.  Asynchronous. */
DSI_API int dsi_mapper_depth_map_of_events_alg2(dsi_mapper_t *out_time_camera, dsi_mapper_t *out_camera_time,
                                                dsi_mapper_t *const *cams, const dsi_batch_t *const *batches, int n_sub,
                                                int stereo_fusion, int temporal_fusion);
/* Host only: the event ranges of Alg. 2's sub-intervals for one camera of n_events events.  ranges[4 k .. 4 k + 3] =
 * (begin0, end0, begin1, end1): sub-interval k is events [begin0, end0) followed by [begin1, end1) (empty unless wrapped).
 * per = n_events / n_sub (the tail is dropped); process_method 2, and camera 0 of 5: [k per, (k + 1) per)
 * (process2.cpp:46-47, :105-107); camera 1 of process_method 5: from (n_sub / 2) per on, wrapping around the end of the
 * events when idx + per >= n_events (process5.cpp:89-93, :135-150). */
DSI_API int dsi_alg2_subintervals(size_t n_events, int n_sub, int process_method, int camera, size_t *ranges);
/* Host only: the planner of the Alg. 2 streams (process.WindowStream, dsi::full_sequence_depth_maps_alg2).  1: a window of
 * n_events events (both cameras), n_sub sub-intervals and nx DSI columns goes through dsi_mapper_depth_map_of_events_alg2;
 * 0: through the materialising process_2 (n_sub > 8, rows too wide for the kernel's registers, or more events per
 * sub-interval than the measured break-even). */
DSI_API int dsi_alg2_plan(int n_sub, size_t n_events, int nx, int camera_time);
DSI_API int dsi_mapper_fetch_depth_map(dsi_mapper_t *m, float *depth_host, float *conf_host, uint8_t *idx_host);
/* the same without waiting: the copies are queued (on the context's copy stream, behind the arg-max
 * only -- not behind later work of the compute stream); the outputs (page-locked memory from
 * dsi_host_alloc) are valid after dsi_mapper_fetch_wait */
DSI_API int dsi_mapper_fetch_depth_map_async(dsi_mapper_t *m, float *depth_host, float *conf_host,
                                             uint8_t *idx_host);
/* the same copies queued on the context's COMPUTE stream, in order behind whatever it already holds -- for pipelines that
 * give every window in flight its own context (main.cpp:177 as a stream: include/dsi_process.hpp full_sequence_depth_maps)
 * and fetch right after the window's kernels: no second stream per context (the runtime maps streams onto four hardware
 * queues by default; contexts with two streams each made windows' uploads and copies queue behind other windows' kernels).
 * Valid after dsi_mapper_fetch_wait, like the _async form. */
DSI_API int dsi_mapper_fetch_depth_map_in_order(dsi_mapper_t *m, float *depth_host, float *conf_host, uint8_t *idx_host);
DSI_API int dsi_mapper_fetch_wait(dsi_mapper_t *m);

/* Plane sharding (one DSI too big or too slow for one GPU): every rank's mapper owns a
 * plane range (dsi_mapper_config_t.plane_begin / plane_count) and grid g holds that range of the
 * (fused) DSI.  collapseMaxZSlice of the whole DSI = local collapse, then ONE all-reduce(MAX) of
 * 64-bit keys (confidence bits << 8 | 255 - global plane index: larger confidence wins, on equal
 * confidence the smaller index -- the first-maximum rule of std::max_element,
 * cartesian3dgrid.cpp:115-137), then index -> depth over the FULL depth vector.  Results stay in
 * the mapper's device buffers (dsi_mapper_fetch_depth_map), identical on every rank. */
DSI_API int dsi_mapper_depth_map_sharded(dsi_mapper_t *m, dsi_grid_t *g, dsi_comm_t *comm);
DSI_API int dsi_mapper_depth_map_sharded_all(dsi_mapper_t *const *mappers, dsi_grid_t *const *grids,
                                             dsi_comm_t *const *comms, int n);

/* The last step of the temporal fusion across GPUs (process2.cpp:211-242 sharded by time slice) with half the
 * xGMI bytes of dsi_grid_allreduce + dsi_grid_finalize + dsi_mapper_depth_map_of: the accumulator `acc` (every
 * rank's local dsi_grid_accumulate results, mode = dsi_acc_mode_t) is REDUCE-SCATTERED by planes -- rank r of n
 * receives the reduced planes [r q, (r+1) q), q = dimZ / n; the dimZ mod n planes left over are all-reduced --,
 * each rank finalises (mode, n_maps) and arg-maxes the planes it owns, and one all-reduce(MAX) of the packed
 * (confidence, plane) keys (8 bytes per pixel) gives every rank the depth map of the fused DSI
 * (dsi_mapper_fetch_depth_map*).  `acc` is consumed: afterwards only the owned planes hold (finalised) values.
 * The mapper must own the whole depth vector.  (reduce-scatter + local finalize / arg-max +
 * gather of the small maps.) */
DSI_API int dsi_mapper_depth_map_reduce_scattered(dsi_mapper_t *m, dsi_grid_t *acc, dsi_comm_t *comm, int mode,
                                                  int n_maps);
DSI_API int dsi_mapper_depth_map_reduce_scattered_all(dsi_mapper_t *const *mappers, dsi_grid_t *const *accs,
                                                      dsi_comm_t *const *comms, int n, int mode, int n_maps);

/* The same three steps with the transport left to the caller, and the partition arithmetic they share (pure host
 * functions, no GPU needed): dsi_mapper_depth_map_reduce_scattered is
 *     reduce (sum / min / max over the ranks) of planes [own_begin, +own_count) to their owner and of planes
 *         [tail_begin, +tail_count) to everybody                                  <- dsi_scatter_plan, ncclReduceScatter + ncclAllReduce
 *     dsi_mapper_depth_map_scattered_local: finalize + arg-max of the owned planes -> packed keys
 *     MAX of the keys over the ranks                                              <- ncclAllReduce(MAX)
 *     dsi_mapper_depth_map_from_keys: keys -> confidence / index / depth
 * so that a caller with another transport (the 2-rank tests carry the two exchanges through host memory; MPI) runs
 * exactly the code the RCCL path runs around its collectives. */
typedef struct {
    int q;          /* planes per rank of the reduce-scatter part: dimZ / nranks */
    int own_begin;  /* this rank's reduce-scatter range: [rank q, (rank + 1) q) */
    int own_count;
    int tail_begin; /* the dimZ mod nranks planes left over: all-reduced, every rank owns them */
    int tail_count;
} dsi_scatter_plan_t;
DSI_API int dsi_scatter_plan(int dim_z, int nranks, int rank, dsi_scatter_plan_t *out);
/* plane sharding (dsi_mapper_config_t.plane_begin / plane_count): contiguous balanced ranges, the first
 * dimZ mod nranks ranks own one plane more */
DSI_API int dsi_plane_range(int dim_z, int nranks, int rank, int *begin, int *count);
/* the arg-max key of a pixel, confidence bits << 8 | 255 - (idx_local + plane_begin), on host arrays: what
 * k_pack_argmax / k_unpack_argmax compute on the device (MAX over shards = collapseMaxZSlice over all planes) */
DSI_API int dsi_argmax_keys_pack(const float *conf, const uint8_t *idx_local, size_t n, int plane_begin, uint64_t *keys);
DSI_API int dsi_argmax_keys_unpack(const uint64_t *keys, size_t n, float *conf, uint8_t *idx_global);
DSI_API int dsi_mapper_depth_map_scattered_local(dsi_mapper_t *m, dsi_grid_t *acc, int nranks, int rank, int mode,
                                                 int n_maps);
/* the mapper's packed arg-max keys (dimY * dimX words), host <-> device; synchronise */
DSI_API int dsi_mapper_argmax_keys_download(dsi_mapper_t *m, uint64_t *keys_host);
DSI_API int dsi_mapper_argmax_keys_upload(dsi_mapper_t *m, const uint64_t *keys_host);
DSI_API int dsi_mapper_depth_map_from_keys(dsi_mapper_t *m);

/* Exact tie resolver: makes the arg-max index map the reference's on every pixel -- VERIFIED EMPIRICALLY per call, not
 * guaranteed a priori (see premise_ok).
 * The engine sums a voxel's votes exactly (64-bit fixed point, rounded once); the reference adds them in fp32 in event
 * order, rounding after every vote (cartesian3dgrid.h:261-270 inside mapper_emvs_stereo.cpp:197-201).  The two sums
 * agree to ~1e-5, so the first-maximum plane (cartesian3dgrid.cpp:132-134) can differ only in columns whose best
 * planes are closer than that -- and there the depth is off by a whole plane.  This call finds the columns of the
 * fused DSI  op(grid(mappers[0]), grid(mappers[1]))  (n == 1: of grid(mappers[0])) that have two or more planes within
 * rel_gap of the column's maximum, re-sums exactly those voxels of every camera in the REFERENCE's order (per camera
 * one pass that asks, per packet and contending voxel, which events the plane transfer takes into the voxel's 2 x 2
 * neighbourhood and votes those with the reference's coordinates, accept test and weights; the recorded votes sorted
 * by (voxel, event index) and added one by one in fp32), re-applies the fusion op, re-picks the first maximum and
 * patches confidence / index / depth in `out`'s depth-map buffers -- all on the device; the host reads counters only.
 * Preconditions: grid(mappers[i]) holds dsi_mapper_evaluate_batch(mappers[i], batches[i]); `out` holds the depth map
 * of that fusion (dsi_mapper_depth_map_of / _of_fusion / _of_events).  n = 1 or 2; op = dsi_fuse_op_t.
 * rel_gap 0 = 2.5e-4: 15x the largest difference ever observed between the two summation orders (1.6e-5) and 2.5x the
 * tolerance every voxel of every parity test is held to.  The rigorous worst case of a voxel, (votes - 1) * 2^-24
 * (max_rel_bound), EXCEEDS that gap for voxels with more than ~4,200 votes, so the gap is a premise, and the call
 * checks it: max_order_diff is the largest |engine value - reference-order value| / max(1, value) over the voxels it
 * re-summed -- the column maxima of the near-tie columns, the most-voted voxels of the volume among them.  If it reaches
 * rel_gap / 8 the pass is repeated with a four times wider gap (gap_widenings, at most 3); premise_ok = 0 when even the
 * last pass did not hold it: the call still returns DSI_OK, the caller decides.  A WIDENED pass that asks for more votes
 * than the pass can record (a workgroup's segment table, the sort key) does not turn into an error either: the last
 * completed pass's patch and statistics stand, premise_ok = 0.  Optional and off the throughput path (elapsed_ms).
 * Synchronises. */
typedef struct {
    float rel_gap;          /* in (0 = 2.5e-4); out: the gap of the last pass (wider than asked for after gap_widenings) */
    int near_tie_pixels;    /* out: columns with >= 2 contending planes */
    int candidate_voxels;   /*      contending voxels re-summed (per camera) */
    int candidate_planes;   /*      distinct planes among them */
    long long votes;        /*      votes re-summed, all cameras */
    int changed_pixels;     /*      pixels whose plane index a pass changed, SUMMED over the passes (a widened pass counts against
                                    the already patched map: with gap_widenings > 0 a pixel can be counted more than once) */
    double max_rel_bound;   /*      see above */
    double max_order_diff;  /*      see above */
    float elapsed_ms;       /*      wall time of the call */
    int gap_widenings;      /*      passes repeated with a 4 x wider gap because max_order_diff reached rel_gap / 8 (0..3) */
    int premise_ok;         /*      1: 8 * max_order_diff < rel_gap held in the last pass.  0: it did not even at the widest gap
                                    tried -- the index map is then NOT known to equal the reference's */
    int columns_bounded;    /*      near-tie columns (of the last pass) whose gap also covers the WORST-CASE reordering error of
                                    their own most-voted contender, 2 ((votes) 2^-24 + 2^-22): for those no plane with at most
                                    that many votes can have been left out wrongly.  (Planes outside the gap with more votes than
                                    every contender are not covered -- a step keeps no per-voxel vote counts --, so this is a
                                    statistic beside premise_ok, not a proof; the proof, with counted votes, is
                                    dsi_mapper_prove_near_ties below.) */
} dsi_resolve_info_t;
DSI_API int dsi_mapper_resolve_near_ties(dsi_mapper_t *out, dsi_mapper_t *const *mappers,
                                         const dsi_batch_t *const *batches, int n, int op, dsi_resolve_info_t *info);

/* The resolver's premise as a PROOF, column by column (ABI 10) -- a verification pass, not part of a step.
 * dsi_mapper_resolve_near_ties re-sums the planes within rel_gap of a column's maximum in the reference's order and trusts
 * that no plane outside that gap can win under the reference's arithmetic; it checks this on the voxels it re-sums
 * (premise_ok), not on the others.  This call closes the gap: it COUNTS the votes of every voxel of every camera (the
 * transfer of mapper_emvs_stereo.cpp:177-195 with the IEEE divide and the accept test of cartesian3dgrid.h:255-259, one
 * global atomic per vote on a dimZ x dimY x dimX volume of 32-bit counters per camera), and then bounds, per voxel, the
 * value the reference holds there: its n non-negative weights added one by one in fp32 stay within
 * (n - 1) u / (1 - (n - 1) u), u = 2^-24, of their real sum (recursive summation), the engine's value is that sum with
 * every weight truncated to the 2^-31 grid and one rounding to fp32 (the mappers' DSIs must be such exact sums:
 * DSI_VOTE_LDS_BANDS, not the paired lane mapping 8 -- DSI_ERR_INVALID otherwise), and the camera fusion
 * (cartesian3dgrid.h:108-190) is monotone with at most five roundings.  A column is PROVEN when every plane below best - rel_gap * best has an upper bound
 * strictly below the lower bound of the maximum's plane: then the reference's first maximum (cartesian3dgrid.cpp:132-134)
 * is among the planes the resolver re-sums exactly, and the resolved index is the reference's.
 *   mappers / batches / n / op: as for dsi_mapper_resolve_near_ties (the cameras' DSIs voted from these batches);
 *   out: any mapper of their shape and context (its scratch holds the counters; its depth map is not touched).
 * gap_needed: the smallest rel_gap that would have taken every offending plane into the re-summed set (0 when all columns
 * are proven); resolving again with a gap a little above it and proving again then proves every column. */
typedef struct {
    float rel_gap;              /* in: the gap the resolver ran with (0: its default, 2.5e-4) */
    long long columns;          /* pixels examined: all of them */
    long long columns_proven;
    long long columns_unproven;
    double gap_needed;
    long long max_votes;        /* most votes in one voxel of one camera */
    float elapsed_ms;
    long long columns_resolved_fully; /* 0 from this call; the proven-mode helpers (process_1_exact_depth_map, process.py) count
                                         here the unproven columns they then re-summed on ALL planes (dsi_mapper_exact_voxels +
                                         dsi_reference_fuse2 + dsi_mapper_patch_depth_map): exact by construction */
} dsi_prove_info_t;
DSI_API int dsi_mapper_prove_near_ties(dsi_mapper_t *out, dsi_mapper_t *const *mappers,
                                       const dsi_batch_t *const *batches, int n, int op, dsi_prove_info_t *info);
/* The same proof for n <= 8 cameras fused by an n-ary mode (BASELINE configs[4]'s four-camera rig): fused = the grid that
 * holds dsi_grid_fuse_n(..., mode) of the mappers' DSIs -- the grid dsi_grid_near_tie_voxels took the near-tie columns from
 * (process.exact_depth_map_nary / the building blocks re-sum them); mode = DSI_ACC_GM_TREE (n = 2, 4, 8), DSI_ACC_MIN,
 * DSI_ACC_MAX or DSI_ACC_SUM (the arithmetic mean).  info->rel_gap: the gap those columns were taken with (0: 2.5e-4).
 * The oracle can only cover a strip of a 1024 x 1024 x 256 volume in reasonable time; this covers every column. */
DSI_API int dsi_mapper_prove_near_ties_n(dsi_mapper_t *out, dsi_grid_t *fused, dsi_mapper_t *const *mappers,
                                         const dsi_batch_t *const *batches, int n, int mode, dsi_prove_info_t *info);
/* The proof's pieces for ANY fusion topology (Alg. 2's camera-then-time fusion, process2.cpp:98-249; compositions of your own):
 * INTERVAL GRIDS.  lo / hi are two grids that enclose, voxel by voxel, the value the reference holds.
 *  - dsi_mapper_reference_interval: lo, hi <- the bounds of the DSI `m` built from `batch` (its votes counted as in
 *    dsi_mapper_prove_near_ties; scratch: any mapper of that shape, e.g. the output mapper);
 *  - carry them through the SAME grid ops the values went through (dsi_grid_fuse2, dsi_grid_accumulate, dsi_grid_finalize,
 *    dsi_grid_fuse_n ... on lo and on hi separately): the reference's voxel-wise ops are monotone non-decreasing in their
 *    operands -- except the 1 / (0.01 + g) inside the harmonic accumulation, which the final n / sum turns around, so for
 *    DSI_ACC_INV_SUM the lower bounds accumulate into the lower result as they are;
 *  - dsi_grid_widen_interval after every such step with the number of fp32 roundings the step performs per voxel (fuse2: 5;
 *    accumulate: 3; finalize: 2; an n-ary tree: 2 per level): lo <- lo (1 - k u) rounded down, hi <- hi (1 + k u) rounded up;
 *  - dsi_grid_prove_columns: `fused` holds the engine's values (the near-tie columns and the threshold come from them);
 *    a column is proven when every plane below best - rel_gap * best has hi strictly below lo of the maximum's plane.
 *    info as for dsi_mapper_prove_near_ties (max_votes: from the dsi_mapper_reference_interval calls on `scratch` since its
 *    last proof); dsi_mapper_proof_unproven lists the columns that are not.
 * process.exact_depth_map_process_2_proven is Alg. 2 done that way. */
DSI_API int dsi_mapper_reference_interval(dsi_mapper_t *scratch, dsi_mapper_t *m, const dsi_batch_t *batch, dsi_grid_t *lo,
                                          dsi_grid_t *hi);
DSI_API int dsi_grid_widen_interval(dsi_grid_t *lo, dsi_grid_t *hi, int roundings);
DSI_API int dsi_grid_prove_columns(dsi_mapper_t *scratch, dsi_grid_t *fused, dsi_grid_t *lo, dsi_grid_t *hi, dsi_prove_info_t *info);
/* votes[i] <- the number of votes voxel voxels[i] (z * dimY * dimX + y * dimX + x) of camera `camera` (0 .. 7) received
 * according to the counters the LAST dsi_mapper_prove_near_ties on `out` made (what its bounds were computed from; the
 * same number dsi_mapper_exact_voxels reports from the resolver's own event pass). */
DSI_API int dsi_mapper_proof_votes(dsi_mapper_t *out, int camera, const uint32_t *voxels, size_t n, uint32_t *votes);
/* The columns the LAST dsi_mapper_prove_near_ties on `out` could not prove: pixels[i] = y * dimX + x, gaps[i] (optional) = the
 * rel_gap that column alone would need (1 = down to its all-but-zero planes: a column whose maximum is a handful of tiny
 * weights, where the engine's 2^-31 weight grid is as coarse as the values).  *n may exceed capacity (nothing is written
 * beyond it).  Few and hard columns are cheaper to re-sum on ALL their planes (dsi_mapper_exact_voxels) than to widen the
 * gap of every column for. */
DSI_API int dsi_mapper_proof_unproven(dsi_mapper_t *out, uint32_t *pixels, float *gaps, size_t capacity, size_t *n);

/* The resolver's building blocks, for fusion topologies it does not cover itself (Alg. 2's camera-then-time fusion,
 * process2.cpp:98-249; n cameras): find the near-tie columns of ANY grid, get the reference-order value of ANY list of
 * voxels of the DSI a mapper builds from a batch, recombine them on the host with the reference's scalar ops, patch
 * the depth map.  dvs_mcemvs_amd/process.py::exact_depth_map_process_2 is Alg. 2 done that way.
 *  - dsi_grid_near_tie_voxels: the voxels (z * dimY * dimX + y * dimX + x) of g within rel_gap of their column's
 *    maximum, for the columns that have >= 2 of them; a column's run contiguous, planes ascending.  *n_voxels may
 *    exceed capacity (then nothing beyond capacity was written: call again with more room).  scratch: any mapper of
 *    g's context and shape (its resolver scratch is used).  dimZ <= 256 (main.cpp:156), else DSI_ERR_SHAPE.
 *  - dsi_mapper_exact_voxels: values[i] <- the value voxel voxels[i] of the DSI of (m, batch) has when its votes are
 *    added in fp32 in event order (resetGrid, then += per vote: mapper_emvs_stereo.cpp:145, :197-201,
 *    cartesian3dgrid.h:261-270); votes[i] (optional) <- their number.  m's grid is not touched.  voxels: any order,
 *    duplicates allowed.
 *  - dsi_reference_fuse2 / _accumulate / _finalize: the reference's voxel-wise ops on host arrays (op = dsi_fuse_op_t;
 *    mode = DSI_ACC_SUM or DSI_ACC_INV_SUM), bit for bit what the device kernels compute.
 *  - dsi_mapper_patch_depth_map: overwrite n pixels (y * dimX + x) of the raw depth map m holds: index, confidence,
 *    depth = plane of the index. */
DSI_API int dsi_grid_near_tie_voxels(dsi_mapper_t *scratch, dsi_grid_t *g, float rel_gap, uint32_t *voxels, size_t capacity,
                                     size_t *n_voxels, size_t *n_columns);
DSI_API int dsi_mapper_exact_voxels(dsi_mapper_t *m, const dsi_batch_t *batch, const uint32_t *voxels, size_t n,
                                    float *values, uint32_t *votes);
DSI_API int dsi_reference_fuse2(int op, const float *a, const float *g, size_t n, float *out);
DSI_API int dsi_reference_accumulate(int mode, float *acc, const float *g, size_t n);
DSI_API int dsi_reference_finalize(int mode, float *acc, size_t n, int n_maps);
DSI_API int dsi_mapper_patch_depth_map(dsi_mapper_t *m, const uint32_t *pixels, const uint8_t *idx, const float *conf,
                                       size_t n);

/* OptionsDepthMap (mapper_emvs_stereo.hpp:68-82), the fields the depth-map extraction reads */
typedef struct {
    int adaptive_threshold_kernel_size; /* --adaptive_threshold_kernel_size, default 5 (main.cpp:73) */
    double adaptive_threshold_c;        /* --adaptive_threshold_c, default 5 (main.cpp:74) */
    int median_filter_size;             /* --median_filter_size, default 5 (main.cpp:75) */
    double max_confidence;              /* --max_confidence (main.cpp:97); written to conf(0,0) */
} dsi_depthmap_options_t;

/* MapperEMVS::getDepthMapFromDSI(depth_map, confidence_map, mask, options)
 * (mapper_emvs_stereo.cpp:339-437) for grid g (NULL = the mapper's own DSI), entirely on the
 * device: collapseMaxZSlice (:368), conf(0,0) = max_confidence + cv::normalize to 8 bit
 * (:393-397), Gaussian adaptive threshold (:403-409), masked Huang median of the depth indices
 * (:420-423, median_filtering.cpp), removeMaskBoundary (:426-427) and
 * convertDepthIndicesToValues of the filtered indices (:435).  The Telea inpainting of
 * depth_map_dense (:430-436) is not reproduced.  Host outputs (any may be NULL): depth f32,
 * confidence f32 (element (0,0) overwritten like the reference does), mask u8 in {0,1},
 * filtered indices u8.  Synchronises. */
DSI_API int dsi_mapper_get_depth_map_from_dsi(dsi_mapper_t *m, dsi_grid_t *g, const dsi_depthmap_options_t *opts,
                                      float *depth_host, float *conf_host, uint8_t *mask_host,
                                      uint8_t *idx_filtered_host);

/* The part of getDepthMapFromDSI after collapseMaxZSlice (mapper_emvs_stereo.cpp:390-437), applied to
 * the raw depth map this mapper holds on the device -- the result of the last
 * dsi_mapper_depth_map_of / _of_fusion / _of_fusion_n / _of_events call.  This is how a window loop
 * that never materialises a DSI (dsi_mapper_depth_map_of_events, mode DSI_VOTE_FUSED_ARGMAX) obtains
 * the reference's filtered per-window outputs (main.cpp:177-302 calls getDepthMapFromDSI on the fused
 * DSI).  Same outputs and bits as dsi_mapper_get_depth_map_from_dsi on the same arg-max.  The raw map
 * is consumed (confidence normalised in place): DSI_ERR_INVALID if there is none, or on a second
 * call.  Synchronises. */
DSI_API int dsi_mapper_filter_depth_map(dsi_mapper_t *m, const dsi_depthmap_options_t *opts, float *depth_host,
                                        float *conf_host, uint8_t *mask_host, uint8_t *idx_filtered_host);

/* OptionsPointCloud (mapper_emvs_stereo.hpp:84-89; main.cpp:80-81) */
typedef struct {
    float radius_search;   /* --radius_search, default 0.05: must be finite and > 0 */
    int min_num_neighbors; /* --min_num_neighbors, default 3: must be >= 0 */
} dsi_pointcloud_options_t;

/* MapperEMVS::getPointcloud(depth_map, mask, options_pc, pc) (mapper_emvs_stereo.cpp:440-480) on the device:
 * every pixel with mask > 0 back-projected through the virtual camera in double (projectPixelTo3dRay, normalize(),
 * b / b[2] * depth; intensity = 1 / z), in row-major pixel order, then PCL's RadiusOutlierRemoval as the count rule
 * of dsi_radius_outlier_removal below.  depth_host (f32) / mask_host (u8) are ny x nx maps; both NULL = the filtered
 * depth map and mask that the last dsi_mapper_filter_depth_map / dsi_mapper_get_depth_map_from_dsi left on the device
 * (no upload; DSI_ERR_INVALID if there is none, i.e. none since the last call that wrote a new depth map).  Output:
 * *n_points points of 4 floats (x, y, z, intensity) into xyzi_host; when capacity < *n_points nothing is written,
 * *n_points is the size needed and the call returns DSI_ERR_INVALID (nx * ny is always enough).  n_unfiltered
 * (may be NULL): the point count before the filter.  Refused on plane-sharded mappers and for a non-finite depth
 * at a masked pixel.  Synchronises. */
DSI_API int dsi_mapper_get_pointcloud(dsi_mapper_t *m, const float *depth_host, const uint8_t *mask_host,
                                      const dsi_pointcloud_options_t *opts, float *xyzi_host, size_t capacity,
                                      size_t *n_points, size_t *n_unfiltered);

/* ---- the run's pictures: accumulateEvents and the two images of saveDepthMaps (definitions: DESIGN.md 7e) ---- */
/* accumulateEvents(events, use_polarity, img) (utils.cpp:184-216) on the device: the 8-bit height x width event image of
 * n events with pixel coordinates x, y (host arrays) and polarity bytes (non-zero = positive; NULL is legal only when
 * use_polarity == 0 or n == 0 -- an empty event list gives 128 everywhere, or 0 without polarity).  n <= 2^31 - 1.  width x height is the SENSOR's size (cam.fullResolution()), not the DSI's.
 *   use_polarity != 0: c = (#positive - #negative) per pixel, an integer -- equal to the reference's fp32 += +-1 while no
 *     pixel holds more than 2^24 events; the counters are int32, which n <= 2^31 - 1 cannot overflow.  half = max(|min c|, |max c|); half == 0 (no events
 *     included): 128 everywhere; else a = (float)(128.0 / half), v = (float)c * a + 128.f in fp32 without FMA, rounded to
 *     nearest (ties to even) and clamped to 0..255: +half gives 255, -half gives 0.
 *   use_polarity == 0: the count modulo 256 (the reference's uchar += 1 wraps), then cv::normalize(NORM_MINMAX, 0, 255):
 *     scale = 255 * (range > DBL_EPSILON ? 1 / range : 0), shift = -min * scale in double, applied as floats, rounded alike.
 * An event with x >= width or y >= height is dropped (the reference would write out of bounds); *n_dropped (may be NULL)
 * is their number.  DSI_ERR_INVALID: width or height < 1, use_polarity without polarity (n > 0), n > 2^31 - 1.  Host output;
 * synchronises. */
DSI_API int dsi_event_image(dsi_context_t *ctx, const uint16_t *x, const uint16_t *y, const uint8_t *polarity, size_t n,
                            int width, int height, int use_polarity, uint8_t *out_u8_host, size_t *n_dropped);
/* same, device output (4-byte aligned, else DSI_ERR_INVALID) and device count (one uint32, may be NULL); asynchronous.
 * Host arrays in page-locked memory must stay unchanged until the context's stream has run. */
DSI_API int dsi_event_image_dev(dsi_context_t *ctx, const uint16_t *x, const uint16_t *y, const uint8_t *polarity, size_t n,
                                int width, int height, int use_polarity, uint8_t *out_u8_dev, uint32_t *n_dropped_dev);
/* The same image of the events a batch already holds on the device: only the polarity bytes travel (the batch's n_events
 * of them, host array; NULL only when use_polarity == 0 or the batch holds no events).  Runs on the batch's context. */
DSI_API int dsi_batch_event_image(const dsi_batch_t *batch, const uint8_t *polarity_host, int width, int height,
                                  int use_polarity, uint8_t *out_u8_host, size_t *n_dropped);
DSI_API int dsi_batch_event_image_dev(const dsi_batch_t *batch, const uint8_t *polarity_host, int width, int height,
                                      int use_polarity, uint8_t *out_u8_dev, uint32_t *n_dropped_dev);
/* The two images saveDepthMaps writes (utils.cpp:55-58 and :82-93) of rows x cols host maps: depth f32, confidence f32
 * exactly as getDepthMapFromDSI returns it (element (0,0) = max_confidence), mask u8.  Either output may be NULL.
 *   conf_negated_host (rows * cols bytes): n = conf * a + b with cv::normalize(NORM_MINMAX, 0, 255)'s a, b of the map's
 *     extremes (scale and shift in double, applied as floats), v = 255.f - n, rounded to nearest (ties to even), clamped.
 *     A constant map gives 255 everywhere.  A map holding NaN gives an unspecified image.
 *   inv_depth_bgr_host (rows * cols * 3 bytes, B G R): i = round_clamp((1.f / depth) * a + b) -- NaN gives 0 -- with
 *     s1 = 1 / max_depth, k = 1 / (1 / min_depth - s1), a = (float)(k * 255), b = (float)((-s1 * k) * 255) (doubles);
 *     colour lut_bgr[i] where mask > 0, black elsewhere; then dilated by the 3 x 3 cross (MORPH_ELLIPSE, Size(3,3)),
 *     the maximum per channel, neighbours outside the image not contributing.
 * lut_bgr: 256 x 3 bytes, B G R; NULL selects the engine's default table (dsi_default_jet_lut), a piecewise-linear jet
 * that is NOT OpenCV's COLORMAP_JET table -- a caller with OpenCV passes cv::applyColorMap of a 0..255 ramp.
 * DSI_ERR_INVALID: rows or cols < 1, an output without its input maps, and -- for the colour image -- min_depth or
 * max_depth not finite, not > 0, or equal.  Synchronises. */
DSI_API int dsi_depth_images(dsi_context_t *ctx, const float *depth_host, const float *conf_host, const uint8_t *mask_host,
                             int rows, int cols, float min_depth, float max_depth, const uint8_t *lut_bgr,
                             uint8_t *conf_negated_host, uint8_t *inv_depth_bgr_host);
/* same, of the filtered depth map, confidence map and mask that the last dsi_mapper_filter_depth_map /
 * dsi_mapper_get_depth_map_from_dsi left on the device (ny x nx; no upload): the bytes dsi_depth_images gives for what
 * that call returned.  DSI_ERR_INVALID if there are none (dsi_mapper_get_pointcloud's rule). */
DSI_API int dsi_mapper_depth_images(dsi_mapper_t *m, float min_depth, float max_depth, const uint8_t *lut_bgr,
                                    uint8_t *conf_negated_host, uint8_t *inv_depth_bgr_host);
/* the default colour table, 256 x 3 bytes B G R: with t = i / 255, r = clamp01(1.5 - |4t - 3|), g = clamp01(1.5 - |4t - 2|),
 * b = clamp01(1.5 - |4t - 1|), each x 255 in double, rounded to nearest (ties to even) */
DSI_API int dsi_default_jet_lut(uint8_t *lut_bgr);

/* ---- scoring depth maps against ground-truth depth (scripts/depth_metrics.py:4-37, precision_completeness.py:43-92,
 * evaluate_mcemvs_dsec.py:127-141; definitions: DESIGN.md 7f) ----
 * A score object lives on the device of its context.  Maps are added one window at a time; the metrics and the error
 * histogram are those of the reference's scripts over the consolidated (windows x H x W) stack.  Per pixel, with estimate d,
 * ground truth g (float32, taken to float64 exactly; all arithmetic in float64 without contraction):
 *   est_valid = mask != 0 && isfinite(d) && d > 0;   gt_valid = isfinite(g) && g >= gt_min;   joint = both.
 * Counts (exact): n_est, n_gt, n_joint, n_delta[k] = #joint with max(d/g, g/d) < 1.25, 1.5625, 1.953125, n_bad = #joint with
 * e > 5 && r > 0.05, e = fabs(1/d - 1/g) * baseline * focal, r = e * g / baseline / focal (left to right).
 * Sums over the joint pixels: di = log(g) - log(d): sum_di, sum_di2; sum_are = sum fabs(d - g) / d; sum_abs = sum fabs(g - d);
 * max_gt over the gt_valid pixels.  The sums are reduced in a fixed order (no floating-point atomics): the same adds in the
 * same order give the same bits.  Each joint pixel's fabs(g - d) is also stored (8 bytes; capacity_points of them), which the
 * median and the histogram read; what does not fit is dropped, never written out of bounds, and `overflow` is set. */
typedef struct dsi_score dsi_score_t;
typedef struct dsi_score_metrics {
    uint64_t n_est, n_gt, n_joint, n_delta[3], n_bad;
    uint64_t n_stored;  /* errors held in the buffer: min(n_joint, capacity_points) */
    int32_t overflow;   /* non-zero: n_joint > capacity_points; median_abs is NaN and dsi_score_median / _histogram refuse */
    int32_t guard_intact; /* the 64 words the object keeps behind its buffer still hold their pattern (always 1) */
    double sum_di, sum_di2, sum_are, sum_abs, max_gt;
    /* derived as the scripts write them, n = n_joint: delta[k] = n_delta[k] / n; silog = 1/n * sum_di2 - 1/(n*n) * sum_di^2;
     * are = 1/n * sum_are; lrmse = sqrt(1/n * sum_di2); badp = n_bad / n; mean_abs = sum_abs / n; median_abs = np.ma.median:
     * the middle stored error, or (lower + upper) / 2 of the two middle ones when n is even.  n == 0: all NaN
     * (max_gt: NaN when n_gt == 0). */
    double delta[3], silog, are, lrmse, badp, mean_abs, median_abs;
} dsi_score_metrics_t;
/* capacity_points >= 1 (8 bytes each), baseline > 0, focal > 0 (the b and f of depth_metrics.py:26-27), gt_min > 0 (the script's
 * 0.05, evaluate_mcemvs_dsec.py:122), all finite, else DSI_ERR_INVALID.  The context refuses to be destroyed before its scores. */
DSI_API int dsi_score_create(dsi_context_t *ctx, size_t capacity_points, double baseline, double focal, double gt_min,
                             dsi_score_t **out);
DSI_API int dsi_score_destroy(dsi_score_t *s);
/* forgets every map added (the buffer's contents included); ordered on the context's stream */
DSI_API int dsi_score_reset(dsi_score_t *s);
/* adds one map of n_pixels >= 1 pixels from host arrays (depth f32, mask u8, ground truth f32): uploaded and scored on the
 * context's stream, without a synchronise -- arrays in page-locked memory must stay unchanged until the stream has run */
DSI_API int dsi_score_add(dsi_score_t *s, const float *depth_host, const uint8_t *mask_host, const float *gt_host,
                          size_t n_pixels);
/* same, the three arrays on the score's device; ordered on the context's stream */
DSI_API int dsi_score_add_dev(dsi_score_t *s, const float *depth_dev, const uint8_t *mask_dev, const float *gt_dev,
                              size_t n_pixels);
/* same, of the filtered depth map and mask that the last dsi_mapper_filter_depth_map / dsi_mapper_get_depth_map_from_dsi
 * left on the device (what dsi_mapper_depth_images reads; DSI_ERR_INVALID if there are none) against gt_host[ny * nx]: only
 * the ground truth travels.  The mapper must belong to the score's context, else DSI_ERR_CONTEXT. */
DSI_API int dsi_score_add_mapper(dsi_score_t *s, dsi_mapper_t *m, const float *gt_host);
/* everything above; after an overflow all but median_abs (NaN) stays valid.  Synchronises. */
DSI_API int dsi_score_metrics(dsi_score_t *s, dsi_score_metrics_t *out);
/* median_abs alone (a 64-bit radix select on the bit patterns of the stored errors): NaN when n_joint == 0;
 * DSI_ERR_INVALID after an overflow.  Synchronises. */
DSI_API int dsi_score_median(dsi_score_t *s, double *median_abs);
/* np.histogram(err, bins = int(max(err) / binwidth)) of the stored errors, bin for bin: *n_bins uniform bins over
 * [*first_edge, *last_edge] = [min(err), max(err)] (widened by -+0.5 when equal), numpy's index arithmetic with its edge
 * correction against np.linspace's edges, the last bin closed on the right.  counts == NULL: only *n_bins and the edges
 * are returned (ask, allocate, call again); otherwise cap >= *n_bins counts are written, and cap < *n_bins is
 * DSI_ERR_INVALID with *n_bins set.  Zero bins (no joint pixel, or max(err) < binwidth: numpy raises there) is DSI_OK with
 * *n_bins = 0.  DSI_ERR_INVALID: binwidth not finite or <= 0, more than 2^24 bins, or after an overflow.  Synchronises. */
DSI_API int dsi_score_histogram(dsi_score_t *s, double binwidth, uint64_t *counts, size_t cap, size_t *n_bins,
                                double *first_edge, double *last_edge);

/* ---- ground-truth depth from DSEC disparity images (scripts/evaluate_mcemvs_dsec.py:75-79, 108-122; definitions:
 * DESIGN.md 7g) ----
 * A projector lives on the device of its context and holds the calibration, a winner table and the output map.  For the
 * float32 disparity image d[height][width] (the script's disp.astype(np.float32) * 256) and source pixel (x, y), all in
 * float64 on the exact values, sums left to right, no contraction:
 *   h_i = ((Q[i][0] x + Q[i][1] y) + Q[i][2] d) + Q[i][3];  (X, Y, Z) = (h_0, h_1, h_2) / h_3, each rounded to float32
 *   kept iff Z < +inf as float32 (NaN, +inf dropped; -inf and negatives kept);
 *   P_i = ((T[i][0] X + T[i][1] Y) + T[i][2] Z) + T[i][3];  p_i = ((K[i][0] P_0 + K[i][1] P_1) + K[i][2] P_2) + K[i][3] P_3;
 *   iu = trunc(p_0 / p_2), iv = trunc(p_1 / p_2);  OUTSIDE: u or v not finite, or not -W <= iu < W, or not -H <= iv < H;
 *   out[iv][iu] = float32(P_2), negative indices wrapping as numpy's; of several points on one pixel the one with the
 *   largest row-major source index wins; untouched pixels are 0.
 * DSI_GT_AS_SCRIPT: one outside point leaves the whole map zero (the script's except branch).  DSI_GT_DROP_OUTSIDE: outside
 * points and points with a negative index are dropped one by one, the rest is written.  n_points = kept points, n_outside =
 * kept points that are outside, in both modes.  No floating-point atomics: the map is a function of the inputs alone. */
typedef struct dsi_gt dsi_gt_t;
#define DSI_GT_AS_SCRIPT 0
#define DSI_GT_DROP_OUTSIDE 1
/* Q[16], T[16] (the matrix that is applied: the script's inv(T_rect0_0)), K[12] (3 x 4, the script's K_0): row-major doubles.
 * DSI_ERR_INVALID: width or height < 1, width * height >= 2^32 - 1, a non-finite entry, an unknown mode.  The context
 * refuses to be destroyed before its projectors. */
DSI_API int dsi_gt_create(dsi_context_t *ctx, int width, int height, const double *Q, const double *T, const double *K,
                          int mode, dsi_gt_t **out);
DSI_API int dsi_gt_destroy(dsi_gt_t *gt);
/* uploads disp_f32_host[height * width] and projects it on the context's stream, without a synchronise (an array in
 * page-locked memory must stay unchanged until the stream has run); the map stays on the device */
DSI_API int dsi_gt_project(dsi_gt_t *gt, const float *disp_f32_host);
/* same, from the 16-bit samples of the disparity PNG: d = (float32(raw) / 65535f) * 256f on the device (matplotlib's 16-bit
 * rule, then the script's * 256); 2 bytes per pixel travel */
DSI_API int dsi_gt_project_u16(dsi_gt_t *gt, const uint16_t *raw_u16_host);
/* synchronises; the last projection's map (depth_host[height * width], may be NULL) and counts (each may be NULL);
 * before the first projection: zeros */
DSI_API int dsi_gt_fetch(dsi_gt_t *gt, float *depth_host, uint64_t *n_points, uint64_t *n_outside);
/* the map on the device (float32 [height][width]); NULL for a NULL projector */
DSI_API float *dsi_gt_device_ptr(dsi_gt_t *gt);
/* dsi_score_add against the projector's map on the device: no ground truth travels.  DSI_ERR_CONTEXT unless both belong to
 * one context; DSI_ERR_INVALID unless n_pixels == width * height */
DSI_API int dsi_score_add_gt(dsi_score_t *s, const float *depth_host, const uint8_t *mask_host, size_t n_pixels, dsi_gt_t *gt);
/* dsi_score_add_mapper against the projector's map: nothing travels.  Same context and pixel-count rules. */
DSI_API int dsi_score_add_mapper_gt(dsi_score_t *s, dsi_mapper_t *m, dsi_gt_t *gt);
/* the script's thicken_edges (:75-79): v = mask ? depth : no_estimate (the script's 255); e = min of v over the 3 x 3 cross
 * (MORPH_ELLIPSE, Size(3, 3)), neighbours outside the image not contributing; out_depth = e, out_mask = (e != no_estimate).
 * NaN inputs give unspecified output.  Synchronises.  rows, cols >= 1, at most 2^29 pixels, else DSI_ERR_INVALID. */
DSI_API int dsi_depth_erode(dsi_context_t *ctx, const float *depth_host, const uint8_t *mask_host, int rows, int cols,
                            float no_estimate, float *out_depth_host, uint8_t *out_mask_host);

/* ---- lens rectification: the table of MapperEMVS::precomputeRectifiedPoints (mapper_emvs_stereo.cpp:256-299) made on the
 * device from the calibration numbers.  Entry y*W+x of the table is float32 of the rectified position of the
 * raw pixel (x, y): plumb_bob as image_geometry::PinholeCameraModel::rectifyPoint = cv::undistortPoints(K, D, R, P) iterates it
 * (5 fixed rounds; D = k1 k2 p1 p2 [k3 [k4 k5 k6]], no thin-prism or tilt terms), fisheye as cv::fisheye::undistortPoints(K, D,
 * R, P) does (Kannala-Brandt, k1..k4, at most 10 Newton rounds, -1000000 where it does not converge).  All in float64; DESIGN.md
 * 7h states the arithmetic operation by operation -- that statement is the contract, parity with an OpenCV binary is unpinned.
 * Reading calibration FILES stays with the caller. */
typedef enum { DSI_LENS_PLUMB_BOB = 0, DSI_LENS_FISHEYE = 1 } dsi_lens_model_t;
typedef struct {
    int model;        /* dsi_lens_model_t */
    int n_dist;       /* coefficients in D: plumb_bob 0, 4, 5 or 8 (missing ones are 0); fisheye 4 */
    double K[9], D[8], R[9], P[12];   /* row-major, as in sensor_msgs::CameraInfo; P's fourth column is not read */
} dsi_lens_t;
/* Host only, needs no GPU.  DSI_ERR_INVALID for an unknown model, a coefficient count the model does not have, a value of K,
 * R, P or of the first n_dist of D that is not finite, fx = K[0] or fy = K[4] equal to 0. */
DSI_API int dsi_lens_check(const dsi_lens_t *lens);
/* Host only: RR = P[:, 0:3] * R (row-major 3 x 3), entry (i, j) = ((0 + p_i0 r_0j) + p_i1 r_1j) + p_i2 r_2j -- the matrix
 * the kernel applies to the undistorted point */
DSI_API int dsi_lens_rr(const dsi_lens_t *lens, double RR[9]);
/* the table, made on the device on the context's stream and copied to lut_host (2 * width * height floats); synchronises.
 * width, height in 1..65536 (event coordinates are u16), else DSI_ERR_INVALID */
DSI_API int dsi_rectify_lut(dsi_context_t *ctx, const dsi_lens_t *lens, int width, int height, float *lut_host);
/* the same into device memory of the caller's (2 * width * height floats, 8-byte aligned), queued on the context's stream,
 * without a synchronise */
DSI_API int dsi_rectify_lut_dev(dsi_context_t *ctx, const dsi_lens_t *lens, int width, int height, float *lut_dev);
/* dsi_mapper_create whose table is made on the device straight into the mapper's own buffer: no host round trip.  cfg->lut must
 * be NULL (DSI_ERR_INVALID otherwise); the table's size is cfg->sensor_width x cfg->sensor_height.  cfg->K stays the caller's:
 * fx, fy, cx, cy of P, as for dsi_mapper_create. */
DSI_API int dsi_mapper_create_with_lens(dsi_context_t *ctx, const dsi_mapper_config_t *cfg, const dsi_lens_t *lens,
                                        dsi_mapper_t **out);

/* pcl::RadiusOutlierRemoval (radius_outlier_removal.hpp, dense cloud) on its own: point i of the n points xyz_host
 * (stride_floats = 3 or 4 floats per point; x, y, z first) is kept (keep_host[i] = 1) iff at least min_neighbors + 1
 * points j -- j = i and duplicates included -- satisfy (double) d2(i, j) <= (double) radius * (double) radius, with
 * d2 = ((dx*dx) + dy*dy) + dz*dz in fp32 without FMA (FLANN's L2_Simple<float>).  n = 0 and n < min_neighbors + 1 are
 * legal (everything is removed).  radius must be finite and > 0, min_neighbors >= 0.  Synchronises. */
DSI_API int dsi_radius_outlier_removal(dsi_context_t *ctx, const float *xyz_host, size_t stride_floats, size_t n,
                                       float radius, int min_neighbors, uint8_t *keep_host);

/* ---- the world map: per-window point clouds fused in a voxel hash on the device (definitions: DESIGN.md 7j) ----
 * A map lives on the device of its context and persists across windows.  Every integrate call moves a cloud from its
 * reference view to the world frame and merges it into cubic cells of edge `leaf`: a centroid per cell (what PCL's
 * VoxelGrid gives), the number of points and the number of CALLS (windows) that reached the cell.
 * THE ARITHMETIC (double, every product and sum rounded on its own, no FMA).  A point is float32 (x, y, z); the pose
 * T_w_rv is 12 doubles, row-major [R | t]:
 *   1. X = ((r00 x + r01 y) + r02 z) + t0, Y and Z alike with rows 1 and 2;
 *   2. per axis q = X / leaf, c = floor(q), f = q - c, F = (uint64) floor(f * 2^32).  f is exact and in [0, 1) except for
 *      -2^-54 < q < 0, where q + 1 rounds to 1 and F = 2^32: the cell's upper face;
 *   3. a point is REJECTED (counted, nothing else changes) when X, Y or Z is not finite or some |c| > 2^20 - 2;
 *   4. per cell: n (u32) accepted points, S[3] (u64) the sums of F, windows (u32) the integrate calls that put at least
 *      one accepted point into the cell;
 *   5. on extraction, per axis Q = S / n (integer division), m = ((double) c + (double) Q * 2^-32) * leaf -- the bracket is
 *      exact -- and the output is (float) m;
 *   6. the cell key is (cx + 2^20 - 1) | (cy + 2^20 - 1) << 21 | (cz + 2^20 - 1) << 42.
 * All of a cell's state is integer sums: the map's bits depend neither on the order of the points, nor on how they are
 * split into calls (windows does, by its definition), nor on the table's size.  The table grows by itself (doubling,
 * while occupied cells + points of the call > 3/4 of the slots) up to 2^27 slots; a call that would need more returns
 * DSI_ERR_INVALID and leaves the map as it was.  Nothing is ever dropped silently.  All calls run on the context's stream. */
typedef struct dsi_map dsi_map_t;
typedef struct dsi_map_info {
    double leaf;
    uint64_t capacity;   /* slots of the table now */
    uint64_t occupied;   /* cells */
    uint64_t calls;      /* integrate calls since creation / reset (empty ones included) */
    uint64_t accepted;   /* points merged */
    uint64_t rejected;   /* points rejected by rule 3 */
    uint64_t growths;    /* doublings of the table since creation / reset */
} dsi_map_info_t;
/* Host only: the inverse of a rigid pose of 12 doubles, row-major [R | t]: R' = R^T, t'_i = -((r0i t0 + r1i t1) + r2i t2)
 * (doubles, no FMA) -- T_rv_w to the T_w_rv the integrate calls take.  out may be T itself. */
DSI_API int dsi_invert_pose(const double T[12], double out[12]);
/* leaf: finite and > 0; capacity_log2: the initial table, 2^8 .. 2^27 slots of 44 bytes.  DSI_ERR_INVALID otherwise. */
DSI_API int dsi_map_create(dsi_context_t *ctx, double leaf, int capacity_log2, dsi_map_t **out);
DSI_API int dsi_map_destroy(dsi_map_t *map);
/* an empty map again: no cells, every count of dsi_map_info zero; the table keeps its present size */
DSI_API int dsi_map_reset(dsi_map_t *map);
/* One call (window) of n host points, stride_floats = 3 or 4 floats per point (x, y, z first), by rules 1-4 above.
 * n = 0 is legal (xyz_host may then be NULL) and still counts as a call.  *n_rejected (may be NULL): the points of this
 * call rejected by rule 3.  Synchronises. */
DSI_API int dsi_map_integrate(dsi_map_t *map, const float *xyz_host, size_t stride_floats, size_t n,
                              const double T_w_rv[12], size_t *n_rejected);
/* One call of the mapper's own cloud: the points dsi_mapper_get_pointcloud(m, NULL, NULL, opts_pc, ...) returns -- made by
 * the same routine from the filtered maps left on the device, with the same refusals -- integrated where they lie, by
 * rules 1-4; only the counts travel.  *n_points / *n_rejected may be NULL.  DSI_ERR_CONTEXT when the map and the mapper
 * were created from different contexts.  Synchronises. */
DSI_API int dsi_map_integrate_mapper(dsi_map_t *map, dsi_mapper_t *m, const dsi_pointcloud_options_t *opts_pc,
                                     const double T_w_rv[12], size_t *n_points, size_t *n_rejected);
DSI_API int dsi_map_info(dsi_map_t *map, dsi_map_info_t *info);
/* the number of cells with n >= min_points and windows >= min_windows (rule 4's counts).  Synchronises. */
DSI_API int dsi_map_count(dsi_map_t *map, uint32_t min_points, uint32_t min_windows, size_t *n);
/* Those cells: centroid by rule 5 (xyz_host, 3 floats per cell), n, windows and key (rule 6); any output may be NULL.
 * The order is the table's -- unspecified, but the same for every call while the map is unchanged; sort by key for a
 * reproducible one.  When capacity < *n nothing is written, *n is the size needed and the call returns DSI_ERR_INVALID
 * (dsi_mapper_get_pointcloud's protocol).  Synchronises. */
DSI_API int dsi_map_extract(dsi_map_t *map, uint32_t min_points, uint32_t min_windows, float *xyz_host,
                            uint32_t *n_points_host, uint32_t *n_windows_host, uint64_t *keys_host, size_t capacity,
                            size_t *n);

/* ---- the map rendered into a camera view: a z-buffered depth image on the device (DESIGN.md 7j "Rendering") ----
 * The depth image the map presents to a pinhole camera at an arbitrary pose: every cell projected, the nearest kept per
 * pixel.  THE ARITHMETIC (double, every product and sum rounded on its own, no FMA), for every cell with
 * n >= min_points && windows >= min_windows:
 *   1. the point (x, y, z) is the cell's centroid exactly as dsi_map_extract returns it -- rule 5 above, rounded to float32 --
 *      widened to double: rendering the map and rendering its extracted cloud are the same thing;
 *   2. X = ((r00 x + r01 y) + r02 z) + t0, Y and Z alike with rows 1 and 2 of T_v_w;
 *   3. the cell is CLIPPED (counted, nothing else changes) when X, Y or Z is not finite or when
 *      Z >= min_depth && Z <= max_depth does not hold (NaN fails);
 *   4. u = (fx * (X / Z)) + cx, v = (fy * (Y / Z)) + cy, iu = floor(u + 0.5), iv = floor(v + 0.5): integer pixel coordinates
 *      are pixel centres (dsi_mapper_get_pointcloud's back-projection convention).  The footprint is the pixels
 *      (iu + dx, iv + dy), |dx|, |dy| <= splat, each tested on its own against 0 <= . < width, 0 <= . < height -- in double,
 *      before anything becomes an integer: huge, infinite and NaN coordinates are dropped, never saturated.  A cell none of
 *      whose footprint pixels lies inside the image is OUTSIDE (counted);
 *   5. a DRAWN cell does, per footprint pixel, hits += 1 (u32) and zkey = min(zkey, key) with
 *      key = (uint64) bits((float) Z) << 32 | (0xFFFFFFFF - windows): Z > 0, so the float's bits order as its value, and
 *      among cells whose float32 depths tie exactly the one seen by the most windows wins.  An empty pixel holds all ones,
 *      which no key equals (its upper half would be a NaN);
 *   6. the images, height x width, row-major: depth (f32) = (float) Z of the winner and 0 where hits == 0, windows (u32) the
 *      winner's count and 0 where empty, hits (u32), mask (u8) = hits > 0.
 * Every effect of a cell is an integer atomic on initialised memory: the images depend neither on the order of the threads,
 * nor on the table's size, nor on where probing put a cell -- they are a function of the map (and the view) alone.
 * tests/world_map_render_reference.py restates this in numpy. */
typedef struct dsi_map_view {
    int32_t width, height;        /* >= 1, width * height <= 2^26 */
    int32_t splat;                /* 0..4: a cell is drawn on the (2 splat + 1)^2 pixels around its pixel */
    uint32_t min_points, min_windows;   /* dsi_map_extract's filter */
    double fx, fy, cx, cy;        /* finite, fx and fy != 0 */
    double min_depth, max_depth;  /* finite, FLT_MIN <= min_depth < max_depth <= FLT_MAX */
    double T_v_w[12];             /* world -> view, row-major [R | t]; dsi_invert_pose makes it from T_w_v */
} dsi_map_view_t;
typedef struct dsi_map_render_info {
    int32_t width, height;
    uint64_t n_cells;     /* passed the filter; = n_clipped + n_outside + n_drawn */
    uint64_t n_clipped;   /* rule 3 */
    uint64_t n_outside;   /* rule 4 */
    uint64_t n_drawn;
    uint64_t n_pixels;    /* pixels with hits > 0 */
} dsi_map_render_info_t;
/* Renders and leaves the four images on the device, in buffers that belong to the map (21 bytes per pixel, allocated on
 * first use, reallocated when width * height changes, freed by dsi_map_destroy).  info may be NULL.  DSI_ERR_INVALID for a
 * NULL map or view or a violated bound of dsi_map_view_t, decided before the GPU is touched.  An empty map renders an empty
 * image.  Synchronises. */
DSI_API int dsi_map_render(dsi_map_t *map, const dsi_map_view_t *view, dsi_map_render_info_t *info);
/* The last render's images to the host (height * width elements each; any may be NULL).  DSI_ERR_INVALID when there is
 * none: before the first render and after dsi_map_reset or any integrate call -- a changed map invalidates its render.
 * Synchronises. */
DSI_API int dsi_map_render_fetch(dsi_map_t *map, float *depth_host, uint32_t *windows_host, uint32_t *hits_host,
                                 uint8_t *mask_host);
/* dsi_score_add_dev of the last render's depth and mask, where they lie, against gt_host[height * width]: only the ground
 * truth travels.  DSI_ERR_CONTEXT when score and map were created from different contexts, DSI_ERR_INVALID without a
 * valid render.  Queued on the context's stream. */
DSI_API int dsi_score_add_map_render(dsi_score_t *score, dsi_map_t *map, const float *gt_host);
/* The same against the depth map the projector last made: nothing travels.  DSI_ERR_INVALID unless the render's
 * width * height equals the projector's. */
DSI_API int dsi_score_add_map_render_gt(dsi_score_t *score, dsi_map_t *map, dsi_gt_t *gt);

/* HIP-event stopwatch around the voting kernel (the replacement of fillVoxelGrid's hot
 * loop, mapper_emvs_stereo.cpp:168-203) on the context's stream: enable, run any number of
 * evaluate/fill calls, then read the summed kernel time and launch count (synchronises and
 * clears).  bench.py derives the roofline figure of the dominant kernel from this. */
DSI_API int dsi_mapper_set_kernel_timing(dsi_mapper_t *m, int enable);
DSI_API int dsi_mapper_vote_kernel_time(dsi_mapper_t *m, float *total_ms, int *launches);

/* Work the voting kernel does on one batch (bench.py's roofline): accepted_event_planes = events x planes that passed
 * the accept test of Grid3D::accumulateGridValueAt (cartesian3dgrid.h:255-259) = the sum of the DSI (the four
 * bilinear weights of a vote sum to 1); accepted_records = the same count after the packet sort has merged the
 * events of a packet that share a pixel into one record = a quarter of the LDS atomics actually issued.  Votes the
 * batch twice and leaves the mapper's DSI as dsi_mapper_evaluate_batch does.  Synchronises. */
DSI_API int dsi_mapper_vote_statistics(dsi_mapper_t *m, const dsi_batch_t *batch, double *accepted_event_planes,
                                       double *accepted_records);

/* diagnostics of the last evaluate/fill call: which kernel ran, bands, chunks */
typedef struct {
    int algo;          /* dsi_vote_algo_t actually used */
    int bands;         /* row bands per plane (LDS algo) */
    int band_rows;     /* owned rows per band */
    int chunks;        /* packet chunks (partial DSIs) */
    int block_threads;
    size_t lds_bytes;
    size_t n_packets;
    int packed;        /* lane mapping that ran (see dsi_mapper_set_packed_lanes) */
    int group_packets; /* packets sorted together by mapping 2 */
} dsi_vote_info_t;
DSI_API int dsi_mapper_last_vote_info(const dsi_mapper_t *m, dsi_vote_info_t *info);

#ifdef __cplusplus
}
#endif
#endif /* DSI_ENGINE_H */
