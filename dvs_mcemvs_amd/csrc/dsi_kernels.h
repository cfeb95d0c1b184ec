// dsi_kernels.h -- internal launch interface between the C-ABI host layer
// (dsi_engine.cpp) and the gfx950 kernels (dsi_kernels.hip).  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dsi {

constexpr int kPacket = 1024;  // mapper_emvs_stereo.hpp:152

// Per (packet, plane) transfer coefficients of mapper_emvs_stereo.cpp:177-182,
// plus what the banded kernel needs to divide quickly.  32 bytes so that one
// s_load_dwordx8 fetches it.
struct PlaneCoef {
    float a, bx, by, d;
    float r;         // RN(1/d) for the residual-corrected division
    uint32_t flags;  // kCoefSkip / kCoefSlow / kCoefInvertible; bits 16-31: the inline cuts' widening in 1/256 rows
    float d_a, by_a;  // the inverse of the row transfer, y0 = Y * d_a - by_a (d / a, by / a): a band's rows -> the packet's
                      // z0 rows -> its run of records.  k_plane_coef turns them into the cut table; with
                      // BandPlan::cuts_inline the vector-fill stream does, per pass, from the transposed row table
};
constexpr uint32_t kCoefSkip = 1u;  // no event of this (packet, plane) can be accepted
constexpr uint32_t kCoefSlow = 2u;  // use the IEEE divide and the whole packet
constexpr uint32_t kCoefInvertible = 4u;  // d_a / by_a are usable by the inline cuts (else the run is the whole packet)

// One entry of a grouped packet: an event's z0 location and how many events of the packet
// share exactly that location (identical raw pixel in one 1024-event packet: hot pixels,
// bursts).  Voting m identical events = one vote of m times the fixed-point weight, exactly.
struct EvRec {
    float x, y;
    uint32_t m;
};

struct Geom {
    int nx, ny, nz;
    float vfx, vfy, vcx, vcy;  // virtual camera (geometry_utils.hpp:30-47)
    float kfx, kfy, kcx, kcy;  // sensor projection intrinsics K_ (mapper_emvs_stereo.cpp:46-48)
    float z0;                  // raw_depths_vec_[0]
};

// lane mappings 5 / 6: 64-bit words of LDS scratch per wave (64 tail-bit words, reused as the run table
// of the hand-scheduled loop, whose entry 64 serves the slots beyond a pass)
constexpr int kVfillScratchWords = 65;

struct BandPlan {
    int bands;          // row bands per plane
    int band_rows;      // owned rows per band (last band may own fewer)
    int chunks;         // packet chunks; each writes its own partial DSI when > 1
    int block_threads;  // 256 / 512 / 1024
    int packed;         // lane mapping: 0 k_vote_bands, 1 k_vote_bands_packed (asm), 2 k_vote_groups,
                        // 3 k_vote_bands_packed (compiled loop), 4 k_vote_groups (asm),
                        // 5 k_vote_bands_packed with the vector fill (wide grids), 6 the same all compiled,
                        // 7 mapping 1 with dealt passes, 8 mapping 7 on PAIRED 32-bit Q.19 cells (opt-in: not the exact sums)
    int group_packets;  // mapping 2: packets sorted together (power of two <= 32)
    int row_pad;        // z0 rows binned over [-row_pad, ny + row_pad) by k_sort_packets
    int pass_lg;        // packed mappings: log2(packets a wave takes per pass); 0 = automatic
    size_t lds_bytes;   // (band_rows + 1) * nx * 8 (u64 fixed-point accumulators; +1 = the carry row)
                        // + mappings 5 / 6: kVfillScratchWords * 8 B per wave (tail-bit words / run table)
    int scratch_offset; // mapping 5: byte offset of that area behind the band
    int persistent;     // packed mappings: workgroups pull work items from per-XCD counters
    int raw_out;        // the voting kernel's `out` is 1: the chunks' partial volumes of raw 64-bit sums (unsigned long long
                        // [chunks][partial_stride]), summed exactly by k_reduce_partials; 0: the fp32 DSI itself (one chunk)
    int halo;           // 1: a band also takes the events of the row above its first owned row and keeps a halo row
                        // on either side in LDS ((band_rows + 2) rows; k_vote_fuse_argmax), 0: carry row ((band_rows + 1))
    int experiment;     // DSI_EXPERIMENT (timing experiments only, results are wrong): 1 no votes, 2 no flush
    int interleave;     // k_vote_fuse_argmax: 1 an XCD's workgroups take the pairs of its stretch in turn, 2 they DRAW them from
                        // the XCD's counter behind the keys (and from the other XCDs' once theirs is dry); see the kernel
    int cuts_inline;    // mappings 5 / 6 with many packets: NO cut table (bands x planes x packets words: 6.1 GB per camera at
                        // 1024 x 1024 x 256 with 100 M events, 3.9 ms to write); the voting kernel's `cuts` argument is then the
                        // TRANSPOSED row table u16 [ny + 2 row_pad + 3][rs_stride] (k_transpose_rowstart) and every pass
                        // derives its packets' runs from it and from PlaneCoef::d_a / by_a
    int rs_stride;      // cuts_inline: packets per row of the transposed table (a multiple of 64)
};

// lane mapping 8: 8-byte words per band row of paired 32-bit cells (dsi_vote_asm.h)
inline int paired_row_words_host(int nx) { return 2 * ((nx >> 1) + 1); }

// distance in voxels between the partial volumes of consecutive packet chunks: the volume size
// rounded up to 4 voxels, so that every partial volume starts 16-byte aligned
__host__ __device__ inline size_t partial_stride(size_t n_voxels) { return (n_voxels + 3) & ~(size_t)3; }

// ---- stage A ---------------------------------------------------------------
hipError_t launch_packet_geometry(hipStream_t s, const float* Rt, int np, const Geom& g,
                                  float* centers, float* H);
hipError_t launch_warp_z0(hipStream_t s, const uint16_t* ex, const uint16_t* ey,
                          const uint32_t* packet_first, int np, const float* H,
                          const float2* lut, int sensor_w, int sensor_h, float2* xy);
// ---- stage B, global-atomic form ------------------------------------------
hipError_t launch_vote_global(hipStream_t s, const float2* xy, const float* centers, int np,
                              const float* planes, const Geom& g, float* dsi);
// ---- stage B, LDS row-band form -------------------------------------------
// the same with stage A (per-packet geometry + z0 warp) fused in: raw events in, centers out
hipError_t launch_sort_packets_raw(hipStream_t s, const float* Rt, const uint16_t* ex, const uint16_t* ey,
                                   const uint32_t* packet_first, const float2* lut, int sensor_w, int sensor_h, const Geom& g,
                                   float* centers, int np, int pad, EvRec* sxy, uint32_t* nvalid,
                                   uint16_t* rowstart, int unit_multiplicity = 0);
hipError_t launch_sort_packets(hipStream_t s, const float2* xy, int np, int ny, int nz, int pad,
                               EvRec* sxy, uint32_t* nvalid, uint16_t* rowstart);
hipError_t launch_plane_coef(hipStream_t s, const float* centers, const float* planes,
                             const uint16_t* rowstart, uint32_t* nvalid, int np,
                             const Geom& g, const BandPlan& bp, PlaneCoef* coef, uint32_t* cuts);
hipError_t launch_vote_bands(hipStream_t s, const EvRec* sxy, const PlaneCoef* coef,
                             const uint32_t* cuts, const uint32_t* slow_any, int np, const Geom& g,
                             const BandPlan& bp, void* out, unsigned long long* seam);
// seam rows (first row of every band but the first, of every plane of every chunk volume in `out`) =
// fl((head + carry) * 2^-31) from the voting kernel's 64-bit sums seam[chunks][nz][bands][2][nx]
hipError_t launch_seam_rows(hipStream_t s, const unsigned long long* seam, int chunks, const Geom& g,
                            const BandPlan& bp, void* out);
hipError_t launch_sort_groups(hipStream_t s, const float2* xy, int np, int S, int ny, int nz, int pad,
                              EvRec* sxy, uint8_t* spk, uint32_t* nvalid, uint16_t* rowstart);
hipError_t launch_group_cuts(hipStream_t s, const uint32_t* prow, const uint16_t* rowstart, int np,
                             int S, const Geom& g, const BandPlan& bp, uint32_t* gcuts);
hipError_t launch_vote_groups(hipStream_t s, const EvRec* sxy, const uint8_t* spk,
                              const PlaneCoef* coef, const uint32_t* gcuts, const uint32_t* slow_any,
                              int np, int S, const Geom& g, const BandPlan& bp, void* out, unsigned long long* seam);
// dsi (+)= fl(sum of the chunks' raw partial volumes).  seam != nullptr (with g, bp; needs an even nx and < 2^32 voxels:
// reduce_can_fold_seams): the seam rows are read from the bands' head / carry sums instead, i.e. launch_seam_rows is
// folded in and must NOT be run on the partial volumes first
hipError_t launch_reduce_partials(hipStream_t s, const unsigned long long* partials, int chunks, size_t n,
                                  float* dsi, int accumulate, const unsigned long long* seam = nullptr,
                                  const Geom* g = nullptr, const BandPlan* bp = nullptr);
inline bool reduce_can_fold_seams(const Geom& g, size_t n) { return (g.nx & 1) == 0 && n <= 0xffffffffull; }
// ---- stage B fused with the camera fusion and the arg-max (no DSI leaves the CU) ----
// the per-camera tables of the banded vote (k_sort_packets / k_plane_coef outputs, built with bp.halo = 1)
struct FusedCamera {
    const EvRec* sxy;
    const PlaneCoef* coef;
    const uint32_t* cuts;
    const uint32_t* slow_any;
    int np;
};
constexpr int kFusedMaxCameras = 4;
struct FusedCameras {
    FusedCamera cam[kFusedMaxCameras];
    int n;  // 1 (vote -> arg-max), 2 (vote x 2 -> op -> arg-max), 3 (process1.cpp:169-191: the trinocular rig --
            // op 1 min, 2 harmonicMeanTwoGrids(g, 3), 6 max of the two-camera result and camera 2) or 4 (round 6: the
            // balanced tree of the reference's 2-ary geometric mean, cartesian3dgrid.h:150-156 -- DSI_ACC_GM_TREE)
};
// LAYOUT LOCK: k_vote_fuse_argmax reads cam[c] with scalar loads straight from the kernel-argument segment
// (__builtin_amdgcn_kernarg_segment_ptr), which holds because (i) `cams` is the kernel's FIRST parameter, so cam[0]
// sits at offset 0 of the segment, and (ii) a by-value struct parameter keeps its host layout there (code object v5:
// by-value aggregates are copied verbatim, aligned to their natural alignment).  Reordering the kernel's parameters or
// these fields breaks (i) / (ii); the asserts below and the one in the kernel catch the second kind at compile time.
static_assert(sizeof(FusedCamera) == 40 && alignof(FusedCamera) == 8, "FusedCamera: 4 pointers + int, 8-byte aligned");
static_assert(offsetof(FusedCamera, sxy) == 0 && offsetof(FusedCamera, coef) == 8 && offsetof(FusedCamera, cuts) == 16 &&
                  offsetof(FusedCamera, slow_any) == 24 && offsetof(FusedCamera, np) == 32,
              "FusedCamera field offsets are read from the kernarg segment");
static_assert(offsetof(FusedCameras, cam) == 0 && sizeof(FusedCameras) == kFusedMaxCameras * sizeof(FusedCamera) + 8,
              "FusedCameras: the camera table starts the struct (and so the kernel-argument segment)");
// Alg. 2 without a DSI (k_vote_fuse_argmax_alg2, dsi_mapper_depth_map_of_events_alg2): the tables of 2 N event batches, k-major --
// b[2 k] camera 0's and b[2 k + 1] camera 1's share of sub-interval k -- for N <= kAlg2MaxSub sub-intervals.  Read like
// FusedCameras: `bt` is the kernel's FIRST parameter and b[] starts the struct, so b[i] lies at 40 i bytes of the
// kernel-argument segment (LAYOUT LOCK, the same two conditions as FusedCameras'; FusedCamera's own asserts above).
constexpr int kAlg2MaxSub = 8;
struct Alg2Batches {
    FusedCamera b[2 * kAlg2MaxSub];
    int n_sub;  // N, 1 .. kAlg2MaxSub
};
static_assert(offsetof(Alg2Batches, b) == 0 && sizeof(Alg2Batches) == 2 * kAlg2MaxSub * sizeof(FusedCamera) + 8,
              "Alg2Batches: the batch table starts the struct (and so the kernel-argument segment)");
static_assert(sizeof(Alg2Batches) <= 1024, "Alg2Batches travels in the kernel-argument segment");
// cells per thread of k_vote_fuse_argmax_alg2 ((band_rows + 2) * nx <= 1024 x this): camera_time keeps four fp32 arrays per
// thread (c0, A_tc, A_l, A_r) beside two running maxima, time_camera alone two
size_t alg2_max_cells(int mapping, bool camera_time);
// keys_tc / keys_ct (nullptr: camera_time not computed) as launch_vote_fuse_argmax's keys; sf 1..6, tf 2 or 4
hipError_t launch_vote_alg2_argmax(hipStream_t s, const Alg2Batches& bt, const Geom& g, const BandPlan& bp, int sf, int tf,
                                   unsigned long long* keys_tc, unsigned long long* keys_ct);
// The preparation of up to three cameras in two launches instead of two per camera (stage A + packet sort; coefficient /
// cut tables), optionally counting the records per (band, plane) pair for launch_fused_splits.
struct PrepCameraArgs {
    const float* Rt;
    const uint16_t *ex, *ey;
    const uint32_t* packet_first;
    const float2* lut;
    int sensor_w, sensor_h;
    float* centers;
    int np;
    EvRec* sxy;
    uint32_t* nvalid;
    uint16_t* rowstart;
    const float* planes;
    PlaneCoef* coef;
    uint32_t* cuts;
    uint32_t* pair_work;  // [bands * nz] or nullptr
    Geom g;               // this camera's own intrinsics, virtual camera and z0 (process1.cpp:73-110: one mapper
                          // per camera, each built from its own calibration); nx, ny, nz equal for all cameras
};
hipError_t launch_prepare_cameras(hipStream_t s, const PrepCameraArgs* cams, int n, const Geom& g, const BandPlan& bp);
// splits[fused_grid_blocks() + 1] <- cuts of the pair list into stretches of equal cost (records + fixed_per_pair
// each); prefix: n_pairs words of scratch.  n_pairs <= fused_max_pairs()
hipError_t launch_fused_splits(hipStream_t s, const uint32_t* work0, const uint32_t* work1, int n_pairs, uint32_t fixed_per_pair,
                               unsigned long long* prefix, uint32_t* splits);
int fused_max_pairs();
// keys[ny * nx] (zeroed by the caller) receive max over planes of conf_bits << 8 | 255 - plane: feed
// launch_unpack_argmax.  splits: optional balanced partition of the (band-major) pair list, one entry
// per workgroup + 1 (fused_grid_blocks() workgroups)
int fused_grid_blocks();
#ifdef DSI_TIMING_EXPERIMENTS
// test hook (experiments flavour only): every later fused_grid_blocks() returns `blocks` (a multiple of 8, >= 8); 0 = the device's
bool fused_grid_blocks_force(int blocks);
// test hook (experiments flavour only): the last launch of a DSI-less kernel -- its grid size, bp.interleave, the kernel
// (1 k_vote_fuse_argmax, 2 its two-per-CU sibling, 3 the instantiation that defers camera 1's arg-max, 4 four cameras,
// 5 k_vote_fuse_argmax_alg2) and whether it read a balanced partition
void fused_last_launch(int* blocks, int* interleave, int* kernel, int* splits);
#endif
size_t fused_max_cells(int mapping, int n_cameras = 2);  // (band_rows + 2) * nx may not exceed this (four cameras: 16 cells per thread)
hipError_t launch_vote_fuse_argmax(hipStream_t s, const FusedCameras& cams, const Geom& g, const BandPlan& bp, int op,
                                   const uint32_t* splits, unsigned long long* keys, unsigned long long* trace = nullptr);
size_t fused_trace_words();  // trace: [workgroup][64 phases][16 waves][4 stamps] of 100 MHz ticks, or nullptr
// ---- Grid3D ops ------------------------------------------------------------
hipError_t launch_fuse2(hipStream_t s, float* a, const float* g, size_t n, int op);
hipError_t launch_fuse2_into(hipStream_t s, float* dst, const float* a, const float* g, size_t n,
                             int op);
hipError_t launch_fuse_hm_n(hipStream_t s, float* a, const float* g, size_t n, int n_maps);
hipError_t launch_accumulate(hipStream_t s, float* acc, const float* g, size_t n, int mode);
hipError_t launch_finalize(hipStream_t s, float* acc, size_t n, int mode, int n_maps);
hipError_t launch_fill(hipStream_t s, float* a, size_t n, float v);
// the depth map's arrays stored by a kernel into mapped page-locked host memory (device-side addresses; any may be null)
hipError_t launch_store_depth_map(hipStream_t s, const float* depth, const float* conf, const uint8_t* idx, size_t npix,
                                  float* depth_host_dev, float* conf_host_dev, uint8_t* idx_host_dev);
hipError_t launch_fuse_n(hipStream_t s, float* dst, const float* const* srcs, int n_src, size_t n, int mode);
hipError_t launch_pack_argmax(hipStream_t s, const float* conf, const uint8_t* idx, int n, int plane_begin,
                              unsigned long long* keys, int combine = 0);
// clear != 0: the keys are zeroed as they are read (the fused vote kernel needs them zero before it runs) -- and so are the
// kFusedKeyTail 64-bit words BEHIND the n keys, which such a buffer must have: the fused kernel's pair-dealing counters
constexpr int kFusedKeyTail = 8;
hipError_t launch_unpack_argmax(hipStream_t s, unsigned long long* keys, int n, const float* planes_full,
                                float* conf, uint8_t* idx, float* depth, int clear = 0);
hipError_t launch_collapse_max_z(hipStream_t s, const float* dsi, int nx, int ny, int nz,
                                 float* conf, uint8_t* idx, const float* planes, float* depth);
hipError_t launch_depth_map_filters(hipStream_t s, float* conf, const uint8_t* idx, int nx, int ny,
                                    int ksize, double C, int median_size, double max_confidence,
                                    const float* planes, uint32_t* minmax_scratch, uint8_t* conf8,
                                    uint8_t* mask, uint8_t* idx_filtered, float* depth);
hipError_t launch_collapse_max_z_fused(hipStream_t s, const float* a, const float* b, int nx, int ny, int nz, int op,
                                       float* conf, uint8_t* idx, const float* planes, float* depth);
hipError_t launch_collapse_max_z_fused_n(hipStream_t s, const float* const* srcs, int n_src, int mode, int nx, int ny,
                                         int nz, float* conf, uint8_t* idx, const float* planes, float* depth);
hipError_t launch_mean_square(hipStream_t s, const float* dsi, size_t n, double* accum);

// ---- exact tie resolver (dsi_mapper_resolve_near_ties): see the kernels' comment ----
// cand[<= cap] <- voxel indices (z * npix + p) of every plane whose value is within rel_gap of its column's maximum, for
// the columns that have >= 2 such planes, a column's run contiguous and ascending in z; counters[0] = voxels (may exceed
// cap: nothing beyond cap is written), counters[1] = columns.  b == nullptr: the values of `a`; else op(a, b)
// cols (<= cols_cap entries) <- per near-tie column (first entry of its run in cand, pixel, contenders, 0).  nz <= 256
hipError_t launch_tie_candidates(hipStream_t s, const float* a, const float* b, int op, int npix, int nz, float rel_gap,
                                 unsigned* counters, uint32_t* cand, uint32_t cap, uint4* cols, uint32_t cols_cap);
// desc[c] <- (x | y << 16, z) of voxel vox[c]; plane_bits (optional, 8 zeroed words): bit z <- plane z holds one of them
hipError_t launch_tie_desc(hipStream_t s, const uint32_t* vox, int n, int nx, int npix, uint2* desc, unsigned* plane_bits);
// The resolver's event pass, inverted (see k_tie_hits_binned): every vote of the batch that lands on one of the voxels
// `desc` -> keys[] = (rank_base + index of the voxel) << pos_bits | position of the vote in the reference's loop over events
// (packet * 1024 + slot), wts[] = the bilinear weight the reference adds.  Output in segments of tie_segment_records()
// records, *seg_counter of them handed out so far (it keeps counting beyond cap_segs: flags bit 1, nothing written there;
// flags bit 0: a block overflowed its segment table); unused tails hold sentinel keys sentinel_rank << pos_bits.  Several
// launches (cameras) may append to the same arrays.  *total_hits += the real votes
int tie_segment_records();
int tie_block_capacity_records();  // votes one workgroup of the pass can record
hipError_t launch_tie_hits_binned(hipStream_t s, const uint16_t* ex, const uint16_t* ey, const uint32_t* packet_first, const float* H,
                                  const float2* lut, int sensor_w, int sensor_h, const float* centers, const float* planes, const Geom& g,
                                  int np, const uint2* desc, int nsv, unsigned rank_base, unsigned pos_bits, unsigned sentinel_rank,
                                  unsigned* seg_counter, unsigned cap_segs, unsigned* flags, unsigned long long* total_hits,
                                  unsigned long long* keys, float* wts);
// per near-tie column: op(exact camera 0, exact camera 1) (op 0: one camera), first maximum, patch; stats[0] = max float bits
// of diff, [1] = max count, [2] += changed pixels, [3] += columns whose gap covers their own contenders' worst-case bound
hipError_t launch_tie_pick(hipStream_t s, int op, const uint4* cols, int n_cols, const uint32_t* vox, int nsv, int npix,
                           const float* exact, const uint32_t* count, const float* diff, const float* planes, float* conf,
                           uint8_t* idx, float* depth, unsigned* stats, float rel_gap);
// round 6, instead of a device-wide sort: the recorded votes partitioned by rank (camera * nsv + voxel) into runs[], each run
// ordered by event position in LDS and added one by one in fp32.  counts / cursor: n_cams * nsv words, starts: one more (scratch);
// runs: n_rec words; wts is consumed (it receives the weights in event order).  exact[cam * nsv + c], count[...] <- sequential fp32
// sum / number of the votes of voxel c of camera cam; diff[...] (optional; needs grid0 (and grid1 for two cameras)) <-
// |grid_cam[vox[c]] - exact| / max(1, |exact|).  No library call.
// the resolver's premise as a per-column proof (dsi_mapper_prove_near_ties): H (nz * ny * nx zeroed words) <- the reference's
// votes per INTEGER location (a voxel's votes: the four locations whose 2 x 2 footprint holds it); then, per column, every plane
// below best - rel_gap * best against the maximum's plane with rigorous bounds of both reference values.  stats5 (zeroed):
// columns proven, columns not, float bits of the rel_gap that would take the offending planes in, most votes in a voxel,
// entries of unproven[] (pixel, float bits of the gap that column needs)
hipError_t launch_count_votes(hipStream_t s, const uint16_t* ex, const uint16_t* ey, const uint32_t* packet_first, const float* H9,
                              const float2* lut, int sensor_w, int sensor_h, const float* centers, const float* planes, const Geom& g,
                              int np, uint32_t* H);
// the proof's pieces for any fusion topology: interval grids (lo / hi enclose the reference's value voxel by voxel)
hipError_t launch_interval_of_counts(hipStream_t s, const float* dsi, const uint32_t* H, int nx, int ny, int nz, float* lo, float* hi,
                                     unsigned* most /* atomicMax: most votes in a voxel */);
hipError_t launch_interval_widen(hipStream_t s, float* lo, float* hi, size_t n, int roundings);
hipError_t launch_prove_columns(hipStream_t s, const float* fused, const float* lo, const float* hi, int npix, int nz, float rel_gap,
                                unsigned* stats5, uint2* unproven);
// ... and for n <= 8 cameras fused by an n-ary mode (DSI_ACC_GM_TREE 6 with n = 2, 4, 8; DSI_ACC_MIN 4, DSI_ACC_MAX 5, DSI_ACC_SUM 0):
// `fused` = the engine's fused grid, whose values decide the near-tie columns and the threshold
hipError_t launch_tie_prove_n(hipStream_t s, const float* fused, const float* const* e, const uint32_t* const* h, int n, int mode, int nx,
                              int ny, int nz, float rel_gap, unsigned* stats5, uint2* unproven);
hipError_t launch_tie_votes_of(hipStream_t s, const uint32_t* H, const uint32_t* vox, int n, int nx, int ny, uint32_t* votes);
hipError_t launch_tie_prove(hipStream_t s, const float* a, const float* b, const uint32_t* Ha, const uint32_t* Hb, int op, int nx,
                            int ny, int nz, float rel_gap, unsigned* stats5, uint2* unproven /* nx * ny entries, or nullptr */);
// cursor: tie_partition_cursor_words(n_ranks) words (the per-stretch table of the LDS path, or one cursor per rank)
size_t tie_partition_cursor_words(size_t n_ranks);
hipError_t launch_tie_partition_sums(hipStream_t s, const unsigned long long* keys, const float* wts, unsigned long long n_rec,
                                     unsigned pos_bits, uint32_t* counts, uint32_t* starts, uint32_t* cursor, unsigned long long* runs,
                                     const uint32_t* vox, int nsv, int n_cams, const float* grid0, const float* grid1, float* exact,
                                     uint32_t* count, float* diff);
hipError_t launch_tie_patch(hipStream_t s, const uint32_t* pix, const uint8_t* new_idx, const float* new_conf, int n,
                            const float* planes, float* conf, uint8_t* idx, float* depth);

// test hook: q[i] = residual-corrected division, ref[i] = n[i] / d[i]
hipError_t launch_div_probe(hipStream_t s, const float* n, const float* d, size_t count,
                            float* q, float* ref);

size_t max_dynamic_lds();

// ---- point cloud (MapperEMVS::getPointcloud): back-projection, radius outlier removal, compaction ----
// The radius filter's scratch, for up to n_max points: spts / key / skey / slot [n_max], bstart [pc_buckets(n_max) + 1],
// tiles [pc_scan_tile_words(max(pc_buckets(n_max), pc_block_words(n_max)))].
struct PcScratch {
    float4* spts;
    unsigned long long *key, *skey;
    uint32_t *slot, *bstart, *tiles;
};
size_t pc_block_words(size_t n);       // per-workgroup counts of a compaction of n items, + the total
size_t pc_scan_tile_words(size_t len);  // scan scratch for `len` values
uint32_t pc_buckets(size_t n);          // hash buckets for n points: a power of two >= 2 n (n <= 2^30)
// the masked pixels of depth / mask (nx x ny, row-major) as points (x, y, z, 1/z) in pixel order; the count lands in
// blk[pc_block_words(nx * ny) - 1] (blk: pc_block_words(nx * ny) words)
hipError_t launch_pc_backproject(hipStream_t s, const float* depth, const uint8_t* mask, int nx, int ny, float fx, float fy,
                                 float cx, float cy, uint32_t* blk, uint32_t* tiles, float4* pts);
// keep[i] (i < n_max) = 1 iff point i of the first *n_dev has >= need points j (itself included) with
// (double) d2_f32(i, j) <= (double) radius^2; 0 from *n_dev on
hipError_t launch_pc_radius_filter(hipStream_t s, const float4* pts, const uint32_t* n_dev, uint32_t n_max, float radius,
                                   uint32_t need, const PcScratch& w, uint8_t* keep);
// out = the points with keep > 0 in input order; their count lands in blk[pc_block_words(n_max) - 1]
hipError_t launch_pc_compact(hipStream_t s, const float4* pts, const uint8_t* keep, uint32_t n_max, uint32_t* blk, uint32_t* tiles,
                             float4* out);

// ---- the world map (dsi_map_*): a voxel hash of 2^cap_log2 slots in one device block ----
// keys [cap] (0 = empty), sums [3 * cap] (u64 sums of the 32-bit cell fractions, x y z per slot), n / windows / stamp [cap]
struct MapTable {
    unsigned long long *keys, *sums;
    uint32_t *n, *windows, *stamp;
    uint32_t cap_log2;
};
size_t map_table_bytes(uint32_t cap_log2);
MapTable map_table_at(void* block, uint32_t cap_log2);  // the arrays inside a block of map_table_bytes (8-byte aligned)
// n points (stride floats each, x y z first) through T_w_rv (row-major [R | t]) into the table as call number `serial` (> 0).
// ctr: four u64 -- occupied slots, accepted points, rejected points, points that found the table full (must stay 0).
// The caller keeps occupied + n <= 3/4 of the capacity.
hipError_t launch_map_integrate(hipStream_t s, const float* pts, uint32_t stride, uint32_t n, const double T_w_rv[12], double leaf,
                                uint32_t serial, const MapTable& t, unsigned long long* ctr);
// every occupied slot of `from` into `to` (zeroed by the caller, larger than `from`)
hipError_t launch_map_rehash(hipStream_t s, const MapTable& from, const MapTable& to, unsigned long long* ctr);
// the cells with n >= min_points and windows >= min_windows: per-workgroup counts, scanned; the total lands in
// blk[pc_block_words(capacity) - 1] (blk: pc_block_words(capacity) words, tiles: pc_scan_tile_words of that)
hipError_t launch_map_count(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, uint32_t* blk, uint32_t* tiles);
// after launch_map_count with the same filter: the cells in slot order -- centroid (3 floats), n, windows, key
hipError_t launch_map_extract(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, double leaf,
                              const uint32_t* blk, float* xyz, uint32_t* n_out, uint32_t* w_out, unsigned long long* key_out);
// the map rendered into a pinhole view (dsi_map_render; DESIGN.md 7j "Rendering"); the host has checked every bound of v
struct MapView {
    double T[12];  // world -> view, row-major [R | t]
    double fx, fy, cx, cy, min_depth, max_depth;
    int width, height, splat;
    uint32_t min_points, min_windows;
};
// 21 bytes per pixel: zkey / hits are the render's working state, depth / windows / mask what the finish pass unpacks
struct MapImage {
    unsigned long long* zkey;
    uint32_t *hits, *windows;
    float* depth;
    uint8_t* mask;
};
constexpr int kMapRenderCounters = 5;  // cells that passed the filter, clipped, outside, drawn, covered pixels
// clears zkey (all ones), hits and ctr, draws every cell that passes v's filter and unpacks the image; ctr: kMapRenderCounters u64
hipError_t launch_map_render(hipStream_t s, const MapTable& t, const MapView& v, double leaf, const MapImage& img, unsigned long long* ctr);

// ---- the map scored in 3-D (include/dsi_map_eval.h; DESIGN.md 7j "Scoring the map in 3-D") ----
// a depth image (width * height = npix <= 2^26 pixels, row-major) and its pinhole; the host has checked every bound
struct MapDepthImage {
    uint32_t width, npix;
    double fx, fy, cx, cy, min_depth, max_depth;
};
// one integrate call of the image's pixels (device arrays; mask may be NULL), by rules 1-4; ctr and the caller's duty as
// launch_map_integrate's, with the call's point count bounded by npix
hipError_t launch_map_integrate_depth(hipStream_t s, const float* depth, const uint8_t* mask, const MapDepthImage& g,
                                      const double T_w_c[12], double leaf, uint32_t serial, const MapTable& t, unsigned long long* ctr);
constexpr int kMapCompareMaxBins = 4096, kMapCompareMaxReach = 3;
constexpr int kMapCompareCounters = 3;  // matched, unmatched, sum_q
struct MapCompare {
    double leaf_a, leaf_b, radius, bin_width;  // bin_width = radius / n_bins > 0
    uint32_t min_points_a, min_windows_a, min_points_b, min_windows_b;
    int reach, n_bins;                         // 1..kMapCompareMaxReach, 1..kMapCompareMaxBins
};
// clears hist [n_bins] and ctr [kMapCompareCounters], then every filtered cell of a against b; dist: one float per slot of a
// (written for the cells that pass a's filter)
hipError_t launch_map_compare(hipStream_t s, const MapTable& a, const MapTable& b, const MapCompare& o, float* dist,
                              unsigned long long* hist, unsigned long long* ctr);
// after launch_map_count(t, min_points, min_windows): key and dist of the filtered cells in slot order (launch_map_extract's)
hipError_t launch_map_compare_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const float* dist,
                                     const uint32_t* blk, float* dist_out, unsigned long long* key_out);

// ---- pruning the map (include/dsi_map_prune.h; DESIGN.md 7j "Pruning") ----
// the five criteria; the host has checked every bound.  calls: the map's call count (the newest serial)
struct MapPrune {
    double leaf, box_lo[3], box_hi[3];
    long long max_age;  // < 0: off
    uint32_t min_points, min_windows, calls, min_neighbors;
    int use_box, reach;  // reach 0..kMapPruneMaxReach
};
constexpr int kMapPruneMaxReach = 2;
constexpr int kMapPruneCounters = 6;               // kept, removed by criterion 1..5
constexpr uint8_t kMapPruneEmpty = 0xff;           // the reason of a slot that holds no cell
// clears ctr [kMapPruneCounters]; first [cap]: every slot's reason by criteria 1-4 (0: survived them); reason [cap]: the
// final reason, criterion 5 judged on `first` alone.  Reads the table, writes the two arrays.
hipError_t launch_map_prune_classify(hipStream_t s, const MapTable& t, const MapPrune& o, uint8_t* first, uint8_t* reason,
                                     unsigned long long* ctr);
// every slot of `from` with reason 0 into `to` (zeroed by the caller); ctr: the map's four counters, [0] += the cells moved
// (the caller cleared it), [3] += cells that found `to` full
hipError_t launch_map_prune_rehash(hipStream_t s, const MapTable& from, const MapTable& to, const uint8_t* reason,
                                   unsigned long long* ctr);
// after launch_map_count(t, 1, 1): key and reason of every cell in slot order (launch_map_extract's)
hipError_t launch_map_prune_gather(hipStream_t s, const MapTable& t, const uint8_t* reason, const uint32_t* blk, uint8_t* reason_out,
                                   unsigned long long* key_out);

// ---- the map's connected components (include/dsi_map_components.h; DESIGN.md 7j "Components") ----
// the labelling of a table, per slot: parent (after launch_map_components the root's slot for a node, kMapCompNone
// elsewhere) and, meaningful at a root's slot only, the component's label (its smallest key), cells and points
struct MapComponents {
    uint32_t* parent;
    unsigned long long* label;
    uint32_t* cells;
    unsigned long long* points;
};
constexpr uint32_t kMapCompNone = 0xffffffffu;
constexpr int kMapCompMaxKeep = 16;
constexpr int kMapCompCounters = 5;        // nodes, unlabelled cells, components, singletons, the largest's points
constexpr int kMapCompSelectCounters = 6;  // kept, removed by reason 1..4, components kept
constexpr int kMapCompTopWords = 2 * kMapCompMaxKeep;  // per rank: cells, label
// the selection's criteria 2-4; keep 0..kMapCompMaxKeep
struct MapCompSelect {
    unsigned long long min_cells, min_points;
    int keep;
};
// clears ctr [kMapCompCounters] and top [kMapCompTopWords]; labels the nodes of t (the cells that pass the filter) at
// connectivity 6, 18, 26 or 124; top[0], top[1]: the largest component's cells and label (0, ~0 without a node).  A fixed
// number of launches, whatever the table holds.
hipError_t launch_map_components(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, int connectivity,
                                 const MapComponents& c, unsigned long long* top, unsigned long long* ctr);
// clears ctr [kMapCompSelectCounters] and top; reason [cap]: every slot's reason under o (kMapPruneEmpty without a cell):
// two launches per rank of o.keep and one for the reasons
hipError_t launch_map_components_select(hipStream_t s, const MapTable& t, const MapComponents& c, const MapCompSelect& o, uint8_t* reason,
                                        unsigned long long* top, unsigned long long* ctr);
// after launch_map_count(t, min_points, min_windows) with the labelling's filter: key, label and (reason != NULL) reason of
// every node in slot order (launch_map_extract's)
hipError_t launch_map_components_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const MapComponents& c,
                                        const uint8_t* reason, const uint32_t* blk, unsigned long long* key_out,
                                        unsigned long long* label_out, uint8_t* reason_out);
// the roots counted per tile of the table and scanned, as launch_map_count does for cells
hipError_t launch_map_components_count_roots(hipStream_t s, const MapTable& t, const MapComponents& c, uint32_t* blk, uint32_t* tiles);
// after launch_map_components_count_roots: label, cells and points of every component in slot order of the roots
hipError_t launch_map_components_list(hipStream_t s, const MapTable& t, const MapComponents& c, const uint32_t* blk,
                                      unsigned long long* label_out, unsigned long long* cells_out, unsigned long long* points_out);

// ---- the map's k nearest cells (include/dsi_map_knn.h; DESIGN.md 7j "Neighbours and statistical outliers") ----
constexpr int kMapKnnMaxK = 16, kMapKnnMaxReach = 3;
constexpr int kMapKnnCounters = 7;        // queries, unqueried cells, scored, isolated, sum_q, sum q^2's low 32 bits, its rest
constexpr int kMapKnnSelectCounters = 4;  // kept, removed by reason 1..3
// the query; the host has checked every bound (k 1..kMapKnnMaxK, min_found 1..k, reach 1..kMapKnnMaxReach)
struct MapKnn {
    double leaf, radius;
    uint32_t min_points, min_windows;
    int k, min_found, reach;
};
// the self query's result, per slot (written for the cells that pass the filter)
struct MapKnnCells {
    uint8_t* found;
    uint32_t* q;
    float* mean;
};
// the neighbours of n points (stride floats each, x y z first): keys [n][k] (padded with 0), dist [n][k] (padded with
// +inf), found [n]; any of the three may be NULL.  Reads the table.
hipError_t launch_map_knn_points(hipStream_t s, const MapTable& t, const MapKnn& o, const float* pts, uint32_t stride, uint32_t n,
                                 unsigned long long* keys, float* dist, uint8_t* found);
// clears ctr [kMapKnnCounters], then every filtered cell of t against the others: c as above
hipError_t launch_map_knn_self(hipStream_t s, const MapTable& t, const MapKnn& o, const MapKnnCells& c, unsigned long long* ctr);
// clears ctr [kMapKnnSelectCounters]; reason [cap]: every slot's reason (kMapPruneEmpty without a cell) with criterion 3
// judged against T_q when use_threshold
hipError_t launch_map_knn_select(hipStream_t s, const MapTable& t, const MapKnn& o, const MapKnnCells& c, int use_threshold, uint32_t T_q,
                                 uint8_t* reason, unsigned long long* ctr);
// after launch_map_count(t, min_points, min_windows) with the query's filter: key, found, mean, q and (reason != NULL)
// reason of every query in slot order (launch_map_extract's)
hipError_t launch_map_knn_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const MapKnnCells& c,
                                 const uint8_t* reason, const uint32_t* blk, unsigned long long* key_out, uint8_t* found_out,
                                 float* mean_out, uint32_t* q_out, uint8_t* reason_out);

// ---- the map's local shape (include/dsi_map_pca.h; DESIGN.md 7j "Local shape") ----
constexpr int kMapPcaCounters = 9;        // queries, unqueried cells, sparse, label 1..3, normal / tangent determined, sum of members
constexpr int kMapPcaSelectCounters = 4;  // kept, removed by reason 1..3
// the pass; the host has checked every bound.  q is the neighbour search's view: k 0..kMapKnnMaxK (0: the radius search),
// min_found from 2 on, reach 1..kMapKnnMaxReach; quantum = leaf * 2^-10
struct MapPca {
    MapKnn q;
    double quantum, viewpoint[3];
    int orient;
};
// the pass's result, per slot (written for the cells that pass the filter): normal, tangent, eval [3] each; moments [9]
// (s[3], ss[6]) or NULL
struct MapPcaCells {
    float *normal, *tangent, *eval;
    uint16_t* members;
    uint8_t *label, *flags;
    long long* moments;
};
// clears ctr [kMapPcaCounters], then every filtered cell of t: its neighbourhood's moments, their solve, the row into c
hipError_t launch_map_pca(hipStream_t s, const MapTable& t, const MapPca& o, const MapPcaCells& c, unsigned long long* ctr);
// clears ctr [kMapPcaSelectCounters]; reason [cap]: every slot's reason (kMapPruneEmpty without a cell) from the pass's labels
hipError_t launch_map_pca_select(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const uint8_t* label,
                                 uint32_t keep_labels, int remove_sparse, uint8_t* reason, unsigned long long* ctr);
// after launch_map_count(t, min_points, min_windows) with the pass's filter: the rows of every query in slot order
// (launch_map_extract's) into key_out and out (compacted; out.moments NULL: not wanted) and (reason != NULL) reason_out
hipError_t launch_map_pca_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const MapPcaCells& c,
                                 const uint8_t* reason, const uint32_t* blk, unsigned long long* key_out, const MapPcaCells& out,
                                 uint8_t* reason_out);

// ---- the map carved by free space (include/dsi_map_visibility.h; DESIGN.md 7j "Visibility") ----
constexpr int kMapObserveMaxWindow = 3;
constexpr int kMapObserveCounters = 7;           // clipped, outside, unseen, agree, through, behind, the image's valid pixels
constexpr int kMapVisibilitySelectCounters = 2;  // kept, carved
// one observation; the host has checked every bound (window 0..kMapObserveMaxWindow, width * height <= 2^26)
struct MapObserve {
    double T[12];  // world -> view, row-major [R | t]
    double fx, fy, cx, cy, min_depth, max_depth, abs_tol, rel_tol;
    int width, height, window;
};
// the tally, per slot: the views with a verdict, and those that agreed and looked through
struct MapTally {
    uint32_t *seen, *agree, *through;
};
// clears ctr [kMapObserveCounters], then every occupied cell of t against the depth image (device arrays; mask may be NULL):
// its verdict added to the tally
hipError_t launch_map_observe(hipStream_t s, const MapTable& t, const MapObserve& o, double leaf, const float* depth, const uint8_t* mask,
                              const MapTally& c, unsigned long long* ctr);
// clears ctr [kMapVisibilitySelectCounters]; reason [cap]: every slot's reason (kMapPruneEmpty without a cell) from the tally
hipError_t launch_map_visibility_select(hipStream_t s, const MapTable& t, const MapTally& c, uint32_t min_through, uint32_t agree_weight,
                                        uint8_t* reason, unsigned long long* ctr);
// after launch_map_count(t, 1, 1): key, tally and (reason != NULL) reason of every cell in slot order (launch_map_extract's)
hipError_t launch_map_visibility_gather(hipStream_t s, const MapTable& t, const MapTally& c, const uint8_t* reason, const uint32_t* blk,
                                        unsigned long long* key_out, const MapTally& out, uint8_t* reason_out);

// ---- merging maps and moving their state (include/dsi_map_merge.h; DESIGN.md 7j "Merging") ----
constexpr int kMapImportCounters = 8;  // bad key, duplicate, n == 0, bad windows, bad stamp, S too large, table full, sum of n
constexpr int kMapMergeCounters = 2;   // cells new to dst, cells both maps hold
// after launch_map_count(t, 0, 0): the raw state of every cell in slot order (launch_map_extract's); sums_out: 3 per cell
hipError_t launch_map_export(hipStream_t s, const MapTable& t, const uint32_t* blk, unsigned long long* key_out, uint32_t* n_out,
                             unsigned long long* sums_out, uint32_t* w_out, uint32_t* stamp_out);
// clears ctr [kMapImportCounters]; m incoming cells (device arrays) checked against `calls` and built into `to` (zeroed by
// the caller, 4 m <= 3 slots); the state is usable only when ctr[0..6] are all 0
hipError_t launch_map_import_build(hipStream_t s, const unsigned long long* keys, const uint32_t* n, const unsigned long long* sums,
                                   const uint32_t* windows, const uint32_t* stamp, uint32_t m, uint32_t calls, const MapTable& to,
                                   unsigned long long* ctr);
// clears mctr [kMapMergeCounters]; every cell of src appended to dst with its stamp moved by off; ctr: dst's four counters,
// [0] += new cells, [1] += add_accepted, [2] += add_rejected, [3] += cells that found dst full.  The caller keeps dst's
// occupied + src's cells <= 3/4 of dst's capacity and every sum below 2^32.
hipError_t launch_map_merge(hipStream_t s, const MapTable& src, const MapTable& dst, uint32_t off, unsigned long long add_accepted,
                            unsigned long long add_rejected, unsigned long long* ctr, unsigned long long* mctr);

// ---- aligning maps (include/dsi_map_align.h; DESIGN.md 7j "Aligning") ----
constexpr int kMapAlignSums = 25;                     // su[3], sv[3], suv_hi[9], suv_lo[9], e2
constexpr int kMapAlignCounters = 2 + kMapAlignSums;  // matched, unmatched, then the sums
struct MapAlign {
    double T[12];  // a's frame in b's, row-major [R | t]
    double leaf_a, leaf_b, radius, quantum;  // quantum = leaf_b * 2^-10
    uint32_t min_points_a, min_windows_a, min_points_b, min_windows_b;
    int reach;     // 1..kMapCompareMaxReach
};
// clears ctr [kMapAlignCounters], then every filtered cell of a, moved by o.T, against b; key_b and dist: one word per slot
// of a (written for the cells that pass a's filter)
hipError_t launch_map_align_step(hipStream_t s, const MapTable& a, const MapTable& b, const MapAlign& o, unsigned long long* key_b,
                                 float* dist, unsigned long long* ctr);
// after launch_map_count(t, min_points, min_windows): a's key, the correspondence's key and the distance of the filtered
// cells in slot order (launch_map_extract's)
hipError_t launch_map_align_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows,
                                   const unsigned long long* key_b, const float* dist, const uint32_t* blk, unsigned long long* key_a_out,
                                   unsigned long long* key_b_out, float* dist_out);
// one integrate call of src's filtered cells (their extracted centroids at leaf_src) under T into dst as call `serial`; ctr
// and the caller's duty as launch_map_integrate's, with the call's point count bounded by src's cells
hipError_t launch_map_integrate_map(hipStream_t s, const MapTable& src, uint32_t min_points, uint32_t min_windows, double leaf_src,
                                    const double T[12], double leaf, uint32_t serial, const MapTable& dst, unsigned long long* ctr);

// focus-based collapses (Grid3D::collapseZSliceBy*, cartesian3dgrid.cpp:192-414; DESIGN.md "Focus-based collapses"):
// method 0 LocalVar, 1 LocalMeanSquare, 2 GradMag (half_patchsize 0..8), 3 LaplacianMag, 4 DoG.  keys: scratch of
// focus_chunks(nx, ny, nz) * nx * ny words, fully written before it is read.  planes / depth as launch_collapse_max_z.
int focus_chunks(int nx, int ny, int nz);
hipError_t launch_focus_collapse(hipStream_t s, const float* dsi, int nx, int ny, int nz, int method, int half_patchsize,
                                 unsigned long long* keys, float* conf, uint8_t* idx, const float* planes, float* depth);
// Grid3D::computeLocalFocusInPlace (cartesian3dgrid.cpp:417-483) into dst (dst != src): focus_method 1 the local mean
// square, any other value the local standard deviation
hipError_t launch_local_focus(hipStream_t s, const float* src, float* dst, int nx, int ny, int nz, int focus_method);
// Grid3D::collapseMinZSlice (cartesian3dgrid.cpp:139-161)
hipError_t launch_collapse_min_z(hipStream_t s, const float* dsi, int nx, int ny, int nz, float* val, uint8_t* idx);

// ---- Grid3D: binary ops 1..4 (subtract, ratio, quadratic mean, cubic mean; cartesian3dgrid.h:95-109,166-184), getMinMax,
// getSlice, accumulateZSliceAt and the 8-bit slice images of imwriteSlices ----
hipError_t launch_grid_binary(hipStream_t s, float* a, const float* g, size_t n, int op);
// words[0..3): (min, max | min_pos | max_pos) once the stream has run; grid_min_max_words() 64-bit words of scratch in all.
// max_blocks: 0 for the default number of workgroups; the result does not depend on it ((value, position) is a total order).
constexpr int kGridMinMaxBlocks = 1024;
size_t grid_min_max_words();
hipError_t launch_grid_min_max(hipStream_t s, const float* vol, size_t n, unsigned long long* words, int max_blocks);
hipError_t launch_grid_get_slice(hipStream_t s, const float* vol, int nx, int ny, int nz, int slice, int dim, float* out);
hipError_t launch_grid_accumulate_z_slice(hipStream_t s, float* vol, int nx, int ny, int iz, const float* img, int rows, int cols);
// words: grid_min_max_words() + 2 * (slices of the orientation) words of scratch; out: nx * ny * nz bytes, 4-byte aligned
hipError_t launch_grid_slices_u8(hipStream_t s, const float* vol, int nx, int ny, int nz, int dim, int normalize_by_minmax,
                                 unsigned long long* words, uint8_t* out);

// ---- the run's pictures: accumulateEvents (utils.cpp:184-216) and the two images of saveDepthMaps (utils.cpp:55-58, 82-93;
// DESIGN.md 7e) ----
// scratch: event_image_scratch_words(width, height) 32-bit words -- [0] ~key of the minimum, [1] key of the maximum, [2] events
// outside the sensor, then the height x width int32 counts; zeroed by the launch.  x, y: 16-byte aligned, pol: 8-byte aligned
// (NULL when use_polarity == 0), out: height * width bytes, 4-byte aligned.  The signed count equals the reference's fp32
// += +-1 while no pixel holds more than 2^24 events; the callers keep n <= 2^31 - 1, which int32 counters hold.
constexpr size_t kEventImageHeadWords = 4;
size_t event_image_scratch_words(int width, int height);
hipError_t launch_event_image(hipStream_t s, const uint16_t* x, const uint16_t* y, const uint8_t* pol, size_t n, int width,
                              int height, int use_polarity, uint32_t* scratch, uint8_t* out);
// the engine's default colour table (256 x BGR; host): a piecewise-linear jet, NOT OpenCV's COLORMAP_JET table
void default_jet_lut(uint8_t* lut_bgr);
// mm: 2 words of scratch; lut_dev: 768 bytes; conf_negated (rows * cols bytes) / inv_depth_bgr (rows * cols * 3 bytes) may be
// NULL (conf / depth, mask, lut_dev are then not read)
hipError_t launch_depth_images(hipStream_t s, const float* depth, const float* conf, const uint8_t* mask, int rows, int cols,
                               float min_depth, float max_depth, const uint8_t* lut_dev, uint32_t* mm, uint8_t* conf_negated,
                               uint8_t* inv_depth_bgr);

// ---- depth-map scores against ground truth: depth_metrics.py:4-37, precision_completeness.py:43-92 ----
// the accumulators of one score object, on the device; zero = empty
struct ScoreState {
    unsigned long long count[7];    // n_est, n_gt, n_joint, n_delta[0..2], n_bad
    unsigned long long cursor;      // errors appended so far, dropped ones included (stored: min(cursor, capacity))
    unsigned long long overflow;    // non-zero once an error was dropped
    unsigned long long max_gt_key;  // bit pattern of the largest valid ground-truth depth (0: none)
    double sum[4];                  // sum di, sum di^2, sum |d - g| / d, sum |g - d|
};
// np.histogram's uniform bins: delta = last - first, step = delta / nb (step_zero: it underflowed)
struct ScoreBins {
    double first, last, delta, step;
    long long nb;
    int step_zero;
};
constexpr int kScoreMaxBlocks = 512;                    // partials: 4 * kScoreMaxBlocks doubles
constexpr long long kScoreMaxBins = 1ll << 24;
constexpr size_t kScoreSelectWords = 4 + 8 * 2 * 256;   // launch_score_select's work area (64-bit words)
// one map of n >= 1 pixels into st, its joint errors |g - d| appended to buf (capacity doubles; what does not fit is dropped
// and st->overflow set); then st->sum += this map's sums.  The order of every addition depends on n alone.
hipError_t launch_score_accumulate(hipStream_t s, const float* depth, const uint8_t* mask, const float* gt, size_t n, double gt_min,
                                   double baseline, double focal, ScoreState* st, double* buf, size_t capacity, double* partials);
// mm[0] / mm[1] = bit patterns of the smallest / largest of the n stored errors (all ones / zero when n == 0)
hipError_t launch_score_minmax(hipStream_t s, const double* buf, size_t n, unsigned long long* mm);
// counts[0 .. bins.nb) = np.histogram(buf[:n], bins=nb) over [first, last], which must hold every stored error
hipError_t launch_score_histogram(hipStream_t s, const double* buf, size_t n, const ScoreBins& bins, unsigned long long* counts);
// work[0] / work[1] = bit patterns of the elements of rank rank0 / rank1 (0-based, < n) of the n stored errors
hipError_t launch_score_select(hipStream_t s, const double* buf, size_t n, size_t rank0, size_t rank1, unsigned long long* work);

// ---- ground-truth depth from disparity images: scripts/evaluate_mcemvs_dsec.py:75-79, 108-122 ----
constexpr int GT_AS_SCRIPT = 0, GT_DROP_OUTSIDE = 1;  // DSI_GT_AS_SCRIPT, DSI_GT_DROP_OUTSIDE
struct GtCalib {
    double Q[16], T[16], K[12];  // row-major; T is the matrix that is applied
};
// device memory of one projection of width * height pixels: the winner table and the output map (both cleared by the
// launch), two counters (kept points, outside points)
struct GtWork {
    uint32_t* winner;
    unsigned int* counters;
    float* out;
};
// out[height][width] = the depth map of the float32 disparity image disp[height][width]; width * height < 2^32 - 1
hipError_t launch_gt_project(hipStream_t s, const float* disp, const GtCalib& calib, int width, int height, int mode, const GtWork& w);
// same, of the raw 16-bit image: d = (float32(raw) / 65535f) * 256f
hipError_t launch_gt_project_u16(hipStream_t s, const uint16_t* raw, const GtCalib& calib, int width, int height, int mode,
                                 const GtWork& w);
// thicken_edges: e = min over the 3 x 3 cross of (mask ? depth : no_estimate); out_depth = e, out_mask = e != no_estimate
hipError_t launch_depth_erode_cross(hipStream_t s, const float* depth, const uint8_t* mask, int rows, int cols, float no_estimate,
                                    float* out_depth, uint8_t* out_mask);

// ---- lens rectification table: precomputeRectifiedPoints, mapper_emvs_stereo.cpp:256-299 ----
constexpr int LENS_PLUMB_BOB = 0, LENS_FISHEYE = 1;  // DSI_LENS_PLUMB_BOB, DSI_LENS_FISHEYE
// what the kernel reads of a dsi_lens_t, by value in the kernel-argument segment (168 bytes)
struct LensCoef {
    double fx, fy, cx, cy;
    double k[8];   // plumb_bob: k1 k2 p1 p2 k3 k4 k5 k6 (missing ones 0); fisheye: k1..k4
    double RR[9];  // P[:, 0:3] R, row-major
};
// lut[y * width + x] = float32 (u, v) of raw pixel (x, y); width * height < 2^32 - 1
hipError_t launch_rectify_lut(hipStream_t s, int model, const LensCoef& c, int width, int height, float2* lut);

// ---- volume filters: laplacianInPlace / smoothInPlace (cartesian3dgrid_filter.cpp:19-110), smoothInPlaceIIR3D
// (gaussianiir3d.cpp:143-251) and the sums of computeMoranIndexGaussianWeights (cartesian3dgrid_filter.cpp:113-199) ----
// dst = the 7-point Laplacian of src with index-clamped neighbours (diffuse == false), or src + dt * that (one explicit
// Euler step of the heat equation).  dst must not be src.
hipError_t launch_stencil3d(hipStream_t s, const float* src, float* dst, int nx, int ny, int nz, bool diffuse, float dt);
// numsteps >= 1 forward / backward recurrences along every line of one axis (0 x, 1 y, 2 z), in place; with_post: every
// voxel * post afterwards (the same single fp32 multiply wherever it is folded in)
hipError_t launch_iir_axis(hipStream_t s, float* vol, int nx, int ny, int nz, int axis, float nu, float boundaryscale,
                           int numsteps, bool with_post, float post);
// words: volume_sum_words() doubles of scratch; words[0] = mean, words[1] = population deviation (two passes), words[2] =
// the Moran numerator once the stream has run.  The order of every addition depends on n alone.
constexpr int kVolumeSumBlocks = 1024;
size_t volume_sum_words();
hipError_t launch_volume_mean_std(hipStream_t s, const float* vol, size_t n, double* words);
// z = z_copy = float((double(v) - mean) * double(inv_stddev))
hipError_t launch_volume_standardize(hipStream_t s, const float* vol, size_t n, double mean, float inv_stddev, float* z, float* z_copy);
// words[2] = sum of double(float(z * float(smooth - centre * z)))
hipError_t launch_volume_moran_numerator(hipStream_t s, const float* z, const float* smooth, size_t n, float centre, double* words);

}  // namespace dsi
