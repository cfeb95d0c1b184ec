// dsi_engine.cpp -- C ABI (include/dsi_engine.h) over the gfx950 kernels.
// Host-side mirror of the reference objects on the hot path:
//   dsi_grid_t    <-> Grid3D        (cartesian3dgrid.h / cartesian3dgrid.cpp)
//   dsi_mapper_t  <-> MapperEMVS    (mapper_emvs_stereo.hpp / .cpp)
//   dsi_batch_t   <-> the (events, per-packet pose) pairs evaluateDSI iterates over
// There is no CPU implementation behind this ABI: without a gfx950 device every
// constructor fails with DSI_ERR_NO_DEVICE.
// Every object owns its device memory, events and streams through the move-only members of dsi_owned.hpp: `delete obj`
// frees them (in reverse order of declaration), a dsi_*_destroy only checks, synchronises and counts before it.
#include "../../include/dsi_engine.h"
#include "../../include/dsi_map_eval.h"
#include "../../include/dsi_map_components.h"
#include "../../include/dsi_map_knn.h"
#include "../../include/dsi_map_pca.h"
#include "../../include/dsi_map_visibility.h"
#include "../../include/dsi_map_prune.h"
#include "../../include/dsi_map_merge.h"
#include "../../include/dsi_map_align.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: librccl is loaded at run time (load_rccl)

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "dsi_host.hpp"
#include "dsi_kernels.h"
#include "dsi_knn_host.hpp"
#include "dsi_owned.hpp"
#include "dsi_pca_host.hpp"

#pragma clang fp contract(off)

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(DSI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                                 \
    } while (0)

#define REQUIRE(cond, code, ...)                  \
    do {                                          \
        if (!(cond)) return fail(code, __VA_ARGS__); \
    } while (0)

using dsi::DevBuf;
using dsi::Event;
using dsi::HostPinned;
using dsi::Stream;

// device scratch of the point-cloud path (dsi_mapper_get_pointcloud, dsi_radius_outlier_removal): grown, never shrunk
struct PcBuffers {
    DevBuf<float> depth;    // host-supplied maps
    DevBuf<uint8_t> mask;
    DevBuf<float4> pts, spts, out;
    DevBuf<unsigned long long> key, skey;
    DevBuf<uint32_t> slot, bstart, tiles, blk, blk2, n;
    DevBuf<uint8_t> keep;
    hipError_t reserve(size_t n_max)
    {
        const size_t buckets = dsi::pc_buckets(n_max), blocks = dsi::pc_block_words(n_max);
        hipError_t e;
        if ((e = pts.reserve(n_max)) != hipSuccess || (e = spts.reserve(n_max)) != hipSuccess ||
            (e = out.reserve(n_max)) != hipSuccess || (e = key.reserve(n_max)) != hipSuccess ||
            (e = skey.reserve(n_max)) != hipSuccess || (e = slot.reserve(n_max)) != hipSuccess ||
            (e = keep.reserve(n_max)) != hipSuccess || (e = bstart.reserve(buckets + 1)) != hipSuccess ||
            (e = tiles.reserve(dsi::pc_scan_tile_words(std::max(buckets, blocks)))) != hipSuccess ||
            (e = blk.reserve(blocks)) != hipSuccess || (e = blk2.reserve(blocks)) != hipSuccess || (e = n.reserve(1)) != hipSuccess)
            return e;
        return hipSuccess;
    }
    dsi::PcScratch scratch() const { return dsi::PcScratch{spts.p, key.p, skey.p, slot.p, bstart.p, tiles.p}; }
};

}  // namespace

// OWNERSHIP (here and in every object struct below): device memory, events and streams are owning members
// (dsi_owned.hpp), freed by `delete obj`; a destroy function only synchronises before it.  Members go in reverse order
// of declaration, so a stream is declared BEFORE whatever is recorded on it or queued to it: it is destroyed last.
struct dsi_context {
    int device = 0;
    Stream stream;  // first: outlives every event and buffer below
    // device -> host copies of depth maps that must not wait for later work of the compute stream
    // (dsi_mapper_fetch_depth_map[_async]); created on first use
    Stream copy_stream;
    Event t0, t1;
    std::vector<Event> marks;  // dsi_context_timeline_mark
    size_t n_marks = 0;
    Event sync_ev;  // dsi_context_wait_for: "everything queued on this stream so far"
    DevBuf<double> ms_accum;  // device scalar for mean-square
    // Event batches are uploaded on their own stream so that the upload of the next batch (camera,
    // window) overlaps the voting of the current one; "ready" / "freed" events order the two streams.
    // ONE upload stream per device, shared by its contexts (uploads share the PCIe link anyway): the runtime maps
    // streams onto four hardware queues by default, and a pipeline of windows -- one context per window in flight --
    // that gave every context two streams of its own had its uploads queue behind another window's kernel
    // (profiles/r04_cpp_window_stream.txt: 0.41 ms per window waiting for uploads).
    hipStream_t upload_stream = nullptr;  // (not owned: upload_stream_acquire / _release)
    // Released event-batch blocks, reused by the next dsi_batch_create on this context: a stream of
    // windows then costs no hipMalloc / hipFree (hipFree synchronises the device).  A plain value, copied between
    // the pool and a batch: whichever holds it frees it (pool_give's trim and ~dsi_context; dsi_batch_destroy gives it back).
    struct PoolBlock {
        void* p;
        size_t bytes;
        hipEvent_t freed;  // recorded on `stream` when the batch was released: its last reader is done
    };
    std::vector<PoolBlock> batch_pool;
    // grow-only scratch of Grid3D::collapseMaxZSlice's host-output form (no hipMalloc / hipFree --
    // i.e. no device synchronisation -- per call)
    DevBuf<unsigned char> collapse_scratch;
    // focus-based collapses: one arg-max key per pixel and plane range; dsi_grid_local_focus in place: the new volume
    DevBuf<unsigned long long> focus_keys;
    DevBuf<float> focus_volume;
    // Grid3D min/max, slices and slice images: partial extremes and per-slice scales; device side of the host-output forms
    DevBuf<unsigned long long> grid_words;
    DevBuf<uint8_t> grid_bytes;
    // volume filters (dsi_grid_laplacian, _smooth_diffuse, _moran_index): the other volume of the ping-pong / the
    // standardized volume and its smoothed copy; the sums of dsi_grid_mean_std and of Moran's index
    DevBuf<float> filter_a, filter_b;
    DevBuf<double> filter_words;
    // the run's pictures (dsi_event_image*, dsi_depth_images, dsi_mapper_depth_images): counts and extremes; uploaded inputs,
    // the colour table and the device side of the host-output forms
    DevBuf<uint32_t> img_words;
    DevBuf<uint8_t> img_bytes;
    // grids, mappers and batches created from this context and not yet destroyed: each holds a pointer to it, so the
    // context refuses to go while any is alive (destroying it first was a use-after-free in their destroy)
    std::atomic<int> children{0};
    PcBuffers pc;  // dsi_radius_outlier_removal
    ~dsi_context();  // what is not an owning member: the shared upload stream and the pooled blocks
};

// the per-device upload stream (see dsi_context::upload_stream)
struct SharedUpload {
    hipStream_t stream = nullptr;
    int refs = 0;
};
std::mutex g_upload_mu;
std::map<int, SharedUpload> g_upload;

hipError_t upload_stream_acquire(int device, hipStream_t* out)
{
    std::lock_guard<std::mutex> lock(g_upload_mu);
    SharedUpload& u = g_upload[device];
    if (!u.stream)
        if (hipError_t e = hipStreamCreateWithFlags(&u.stream, hipStreamNonBlocking)) return e;
    ++u.refs;
    *out = u.stream;
    return hipSuccess;
}

void upload_stream_release(int device)
{
    std::lock_guard<std::mutex> lock(g_upload_mu);
    auto it = g_upload.find(device);
    if (it == g_upload.end()) return;
    if (--it->second.refs <= 0) {
        if (it->second.stream) {
            (void)hipStreamSynchronize(it->second.stream);
            (void)hipStreamDestroy(it->second.stream);
        }
        g_upload.erase(it);
    }
}

dsi_context::~dsi_context()
{
    if (upload_stream) upload_stream_release(device);
    for (auto& blk : batch_pool) {
        (void)hipFree(blk.p);
        (void)hipEventDestroy(blk.freed);
    }
}

hipError_t copy_stream_of(dsi_context* ctx, hipStream_t* out)
{
    if (!ctx->copy_stream)
        if (hipError_t e = ctx->copy_stream.create(hipStreamNonBlocking)) return e;
    *out = ctx->copy_stream;
    return hipSuccess;
}

bool pool_take(dsi_context* ctx, size_t bytes, dsi_context::PoolBlock* out)
{
    size_t best = (size_t)-1;
    for (size_t i = 0; i < ctx->batch_pool.size(); ++i) {
        const size_t sz = ctx->batch_pool[i].bytes;
        if (sz >= bytes && sz <= 4 * bytes + 65536 && (best == (size_t)-1 || sz < ctx->batch_pool[best].bytes))
            best = i;
    }
    if (best != (size_t)-1) {
        *out = ctx->batch_pool[best];
        ctx->batch_pool.erase(ctx->batch_pool.begin() + (long)best);
        return true;
    }
    out->p = nullptr;
    out->bytes = bytes;
    out->freed = nullptr;
    if (hipMalloc(&out->p, bytes) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&out->freed, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(out->p);
        return false;
    }
    (void)hipEventRecord(out->freed, ctx->stream);
    return true;
}

void pool_give(dsi_context* ctx, const dsi_context::PoolBlock& blk)
{
    if (!blk.p) return;
    (void)hipEventRecord(blk.freed, ctx->stream);  // everything that read the block was queued before
    ctx->batch_pool.push_back(blk);
    // keep a handful -- two windows of Alg. 2's up to 2 x 8 sub-interval batches (dsi_mapper_depth_map_of_events_alg2), so
    // that a stream's batches are reused instead of freed (a free waits for the stream) -- and drop the oldest
    if (ctx->batch_pool.size() > 4 * (size_t)dsi::kAlg2MaxSub) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(ctx->batch_pool.front().p);
        (void)hipEventDestroy(ctx->batch_pool.front().freed);
        ctx->batch_pool.erase(ctx->batch_pool.begin());
    }
}

struct dsi_grid {
    dsi_context* ctx = nullptr;
    int nx = 0, ny = 0, nz = 0;
    size_t n = 0;
    float* data = nullptr;  // the volume: `own.p`, or the caller's memory (dsi_grid_wrap), which is not freed
    DevBuf<float> own;
};

struct dsi_batch {
    dsi_context* ctx = nullptr;
    dsi_context::PoolBlock block{nullptr, 0, nullptr};  // one device allocation holding the four arrays below
    Event ready;  // recorded on the copy stream after the upload
    uint16_t *x = nullptr, *y = nullptr;
    uint32_t* first = nullptr;
    float* Rt = nullptr;
    size_t n_events = 0, n_packets = 0;
};

// grow-only device scratch of the exact tie resolver (dsi_mapper_resolve_near_ties), owned by the output mapper
struct TieScratch {
    DevBuf<uint32_t> cand, count, rank_count, rank_start, rank_cursor;
    DevBuf<uint2> desc;
    DevBuf<uint4> cols;
    // 32-bit words: [0] contending voxels, [1] near-tie columns (k_tie_candidates); [2] output segments handed out,
    // [3] overflow flags (k_tie_hits_binned); [4] max order difference (float bits), [5] max votes of a voxel (k_tie_pick);
    // [6] changed pixels (k_tie_pick); [8..9] one 64-bit word: real votes recorded; [16..23] planes with a contender (k_tie_desc)
    DevBuf<unsigned long long> counters;
    DevBuf<unsigned long long> keys, keys2;
    DevBuf<float> w, exact, diff;
    DevBuf<char> tmp;  // dsi_mapper_patch_depth_map: the new indices
    DevBuf<uint32_t> votes[8];  // dsi_mapper_prove_near_ties(_n): the cameras' vote counters per integer location
    bool votes_valid[8] = {false, false, false, false, false, false, false, false};
    DevBuf<unsigned> interval_most;  // dsi_mapper_reference_interval: most votes in a voxel since the last dsi_grid_prove_columns
    bool interval_most_live = false;
    DevBuf<uint2> unproven;     // ... and the columns it could not prove (pixel, float bits of the gap the column needs)
    size_t n_unproven = 0;
    HostPinned<unsigned> host;  // page-locked copy of the counters: the three reads of a call are plain DMAs
    hipError_t host_counters(unsigned** out)
    {
        if (!host)
            if (hipError_t e = host.alloc(64, hipHostMallocDefault)) return e;
        *out = host;
        return hipSuccess;
    }
};

struct dsi_mapper {
    dsi_context* ctx = nullptr;
    // Opt-in experiment (DSI_PREP_OVERLAP=1): stage A, the packet sort and the coefficient tables of
    // evaluateDSI on a second stream, overlapping whatever the context's stream is still doing
    // (typically the previous camera's voting kernel).  Measured: the voting kernel loses more
    // (1.21 -> 1.38 ms: wave slots, LDS and L2 taken by the preparation kernels) than the overlap
    // hides, 2.80 -> 2.92 ms per step, so it is off by default.
    Stream prep_stream;  // (a stream: before the buffers its kernels use, see dsi_context)
    Event ev_prep, ev_vote_done;
    TieScratch tie;
    int sensor_w = 0, sensor_h = 0;
    dsi::Geom geom{};
    std::vector<float> planes;  // raw_depths_vec_ (of the planes this mapper owns)
    std::vector<float> planes_full;  // the whole depth vector (plane-sharded arg-max: index -> depth)
    DevBuf<float> planes_full_dev;
    DevBuf<unsigned long long> argmax_keys;
    DevBuf<unsigned long long> fused_keys;   // dsi_mapper_depth_map_of_events: one arg-max key per pixel, kept zero between calls
    DevBuf<unsigned long long> fused_trace;  // test hook: time stamps of the fused kernel's phases
    bool fused_trace_on = false;
    int unit_multiplicity = 0;  // set only inside dsi_mapper_vote_statistics
    // fused kernel: records per (band, plane) pair of this camera's tables; the balanced partition; the cost of
    // a phase's set-up, pass switches, barriers and read-back in record units (measured with tools/fused_trace.py at
    // 512 x 512 x 200: a phase without records takes 8.6 us, a full one 18.7 us for ~38 k records)
    DevBuf<uint32_t> pair_work, fused_splits;
    DevBuf<unsigned long long> fused_prefix;
#ifdef DSI_TIMING_EXPERIMENTS
    int fused_solo = -1;  // test hook dsi_test_fused_solo: >= 0 = one workgroup acting as workgroup 0 of that XCD
#endif
    int fused_fixed_cost = -1;  // < 0: equal pair counts per workgroup (default: balancing by records did not pay at
                                // 512 x 512 x 200 -- 446 vs 447 us, the slow workgroups are slow per record, not by count)
    int want_pass_lg = 0;  // test hook: log2(packets per pass) of the packed / vector-fill streams (0 = automatic)
    int plane_begin = 0;        // first owned plane of the full depth vector (plane sharding)
    DevBuf<float> planes_dev;
    DevBuf<float2> lut_dev;
    dsi_grid* grid = nullptr;
    bool vote_recorded = false;
    int prep_overlap = 0;
    int algo = DSI_VOTE_AUTO;
    int want_band_rows = 0, want_chunks = 0, want_block = 0;
    int want_packed = -1;  // -1 automatic, 0 per-packet waves, 1 packed lanes, 2 packet groups
    bool keep_z0 = false;  // tests: materialise event_locations_z0 (stage A as separate kernels)
    dsi_vote_info_t info{};
    // scratch
    DevBuf<float> centers, H, Rt_tmp, conf, depth;
    DevBuf<unsigned long long> partials;  // [chunks][partial_stride]: raw 64-bit sums per chunk (several chunks, or accumulation)
    DevBuf<float2> xy;
    DevBuf<dsi::EvRec> sxy;
    DevBuf<unsigned long long> seam;  // [chunks][nz][bands][2][nx]: 64-bit sums of each band's first row and of the row below it
    DevBuf<uint32_t> nvalid, cuts, gcuts;
    size_t cuts_inline_min_packets = 8192;   // vote_device: from this many packets on the vector fill derives its cuts itself
    bool info_cuts_inline = false;           // the last banded vote did
    DevBuf<uint8_t> spk;
    DevBuf<uint16_t> rowstart;
    DevBuf<dsi::PlaneCoef> coef;
    DevBuf<uint8_t> idx, conf8, mask, idx_filtered;
    DevBuf<uint32_t> minmax;
    bool depth_valid = false;
    // m->depth / m->mask hold the FILTERED map and mask of the last dsi_mapper_filter_depth_map (the device-resident input of
    // dsi_mapper_get_pointcloud); cleared by every call that writes a new depth map (depth_buffers_ready)
    bool filtered_valid = false;
    PcBuffers pc;
    // dsi_mapper_depth_map_of_events_alg2, on its time_camera output mapper: the banded-vote tables of each of the 2 N
    // event batches of a window (what a camera mapper holds for one batch in the fused path)
    struct BatchTables {
        DevBuf<float> centers;
        DevBuf<dsi::EvRec> sxy;
        DevBuf<uint32_t> nvalid, cuts;
        DevBuf<uint16_t> rowstart;
        DevBuf<dsi::PlaneCoef> coef;
    };
    std::vector<BatchTables> alg2_tables;  // (resize relocates the tables: DevBuf moves)
    bool fused_keys_dirty = false;  // the fused kernel may have written keys that no unpack cleared
    // The depth map leaves the device on the context's COPY stream, so that fetching window w's map
    // does not queue behind window w+1's kernels on the compute stream: "ready" (compute stream, after
    // the arg-max) gates the copies, "read" (copy stream, after them) gates the next arg-max into the
    // same buffers.
    Event ev_depth_ready, ev_depth_read;
    bool depth_read_pending = false;
    // HIP-event stopwatch around the dominant (voting) kernel, for bench.py's roofline
    bool timing = false;
    std::vector<Event> timing_pairs;  // recorded, not yet read: [2 i] before and [2 i + 1] after launch i
    std::vector<Event> timing_pool;
};

namespace {

int set_device(const dsi_context* ctx)
{
    HIP_TRY(hipSetDevice(ctx->device));
    return DSI_OK;
}

// ShapeDSI + setupDSI (mapper_emvs_stereo.cpp:208-241), depth_vector.hpp:76-163
void make_planes(float min_depth, float max_depth, int nz, bool inverse, std::vector<float>* out)
{
    if (min_depth > max_depth) std::swap(min_depth, max_depth);  // depth_vector.hpp:33-36
    out->resize(nz);
    if (!inverse) {
        const float mult = (float)nz / (max_depth - min_depth);  // :88
        for (int i = 0; i < nz; ++i) (*out)[i] = min_depth + (float)i / mult;  // :93
    } else {
        const float inv_min = 1.f / min_depth, inv_max = 1.f / max_depth;  // :131-132
        const float mult = (float)nz / (inv_min - inv_max);
        for (int i = 0; i < nz; ++i) {
            const float rho = inv_max + (float)i / mult;  // :138
            (*out)[i] = 1.f / rho;                        // :145-148
        }
    }
}

float virtual_focal(float cam_fx, float fov_deg, int dim_x)
{
    if (fov_deg < 10.f) return cam_fx;  // mapper_emvs_stereo.cpp:220-224
    const float fov_rad = (float)((double)fov_deg * 3.1415926535897932384626433832795 / 180.0);
    return (float)(0.5 * (double)(float)dim_x / std::tan(0.5 * (double)fov_rad));  // :227-228
}

// Choose the LDS band decomposition for a grid and a packet count.
bool plan_bands(const dsi_mapper* m, size_t n_packets, dsi::BandPlan* bp)
{
    const dsi::Geom& g = m->geom;
    // Q33.31 LDS accumulators, one per cell -- or, lane mapping 8 (opt-in, never chosen automatically), rows of paired 32-bit
    // cells: 2 * ((nx >> 1) + 1) words of 8 bytes
    const size_t row_bytes = (size_t)(m->want_packed == 8 ? dsi::paired_row_words_host(g.nx) : g.nx) * sizeof(unsigned long long);
    const int block_threads = m->want_packed == 8 ? 1024 : (m->want_block > 0 ? m->want_block : 1024);
    // Lane mapping and workgroups per CU, by the records of a packet a band sees (its run):
    // rows + 1 of Ny rows see 1024 * (rows + 1) / Ny events of a packet.
    //  * TWO 1024-thread workgroups per CU (32 waves; half the LDS each) with the packed mapping and its
    //    hand-scheduled scalar run bookkeeping (1) when half the LDS still gives runs of >= ~56
    //    records (346x260x100: 106; measured against one workgroup per CU with either mapping, 10 M
    //    events: 480x360x100 (57) 1.33 vs 1.44 / 1.48 ms, 400x300x64 (85) 0.89 vs 0.91 / 0.96);
    //  * else ONE workgroup per CU; the scalar bookkeeping per run piece then dominates when the run
    //    is short and the vector fill (5) takes over below ~72 records (mapping 1 / mapping 5:
    //    1024x1024x256 (20) 7.6 / 4.25 ms, 800x600x128 (42) 2.43 / 1.84, 720x540x100 (53) 1.68 / 1.48,
    //    640x480x100 (68) 1.55 / 1.43, 512x512x200 (78) 2.81 / 2.63 at 10 M events but 0.216 / 0.222
    //    at a 0.5 M-event window and 0.379 / 0.380 at 1 M).
    // (The packed mapping is 1.1x (240x180) to 3x faster than the per-packet mapping 0.)
    int packed = m->want_packed;
    bool auto_two_per_cu = false;
    if (packed < 0) {
        const long rows_full = std::max<long>(1, (long)(dsi::max_dynamic_lds() / row_bytes) - 1);
        const long rows_half = (long)((dsi::max_dynamic_lds() / 2) / row_bytes) - 1;
        // (round 3: wherever the packed mapping is chosen it is lane mapping 7 -- the same hand-scheduled loop with
        //  DEALT passes: 10 M events, same box, mapping 1 / 7: 346x260x100 1.198 / 1.187 ms, 240x180x100 1.187 / 1.150,
        //  512x512x200 2.80 / 2.53; the vector fill keeps its range: 640x480x100 1.40 (5) vs 1.46 (7), 800x600x128
        //  1.78 vs 2.07, 1024x1024x256 4.32 vs 6.42)
        if (rows_half >= 4 && 1024L * (rows_half + 1) / g.ny >= 56) {
            packed = 7;
            auto_two_per_cu = true;
        } else {
            packed = 1024L * (rows_full + 1) / g.ny < 72 ? 5 : 7;
        }
    }
    // lane mapping 5 keeps 64 tail-bit words per wave behind the band
    const size_t scratch_bytes = (packed == 5 || packed == 6) ? (size_t)(block_threads / 64) * dsi::kVfillScratchWords * 8 : 0;
    const long max_rows_total = (long)((dsi::max_dynamic_lds() - scratch_bytes) / row_bytes);
    if (max_rows_total < 2 || g.nx < 2 || g.ny < 2 || g.ny > 16000) return false;
    long max_owned = max_rows_total - 1;  // + the carry row
    if (m->want_band_rows > 0) {
        max_owned = std::min<long>(max_owned, m->want_band_rows);
    } else {
        // two workgroups per CU (above; a mapping forced by the caller keeps the older, stricter rule)
        const long half_rows = (long)((dsi::max_dynamic_lds() / 2 - scratch_bytes) / row_bytes) - 1;
        if (half_rows >= 4 && (auto_two_per_cu || 1024L * (half_rows + 1) / g.ny >= 96)) max_owned = half_rows;
    }
    int bands = (int)((g.ny + max_owned - 1) / max_owned);
    int band_rows = (g.ny + bands - 1) / bands;  // balanced
    if (m->want_band_rows > 0) band_rows = (int)std::min<long>(m->want_band_rows, max_owned);
    bands = (g.ny + band_rows - 1) / band_rows;
    bp->bands = bands;
    bp->band_rows = band_rows;
    bp->scratch_offset = (int)((size_t)(band_rows + 1) * row_bytes);
    bp->lds_bytes = (size_t)(band_rows + 1) * row_bytes + scratch_bytes;
    bp->block_threads = block_threads;
    bp->row_pad = std::min(g.ny, 4096);  // z0 locations spill up to ~ny rows outside the grid
    // expected events of one packet in one band
    const long run = 1024L * (band_rows + 1) / g.ny;
    bp->packed = packed;
    // mapping 2 sorts S consecutive packets together so that a run holds >= ~512 events
    // (mapping 4, the hand-scheduled loop, packs the runs of consecutive groups into the lanes, so
    //  it only needs runs of a few batches)
    const long want_run = bp->packed == 4 ? 160 : 512;
    int S = 1;
    while (S < 32 && (long)S * std::max<long>(run, 1) < want_run) S <<= 1;
#ifdef DSI_TIMING_EXPERIMENTS  // (tuning knobs exist only in builds made with build.py --experiments)
    if (const char* e = std::getenv("DSI_GROUP_PACKETS")) {
        const int v = std::atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32) S = v;
    }
#endif
    bp->group_packets = S;
    // Persistent workgroups (the grid is what the chip holds at once; workgroups pull work items from
    // per-XCD counters) pay off when only ONE workgroup fits a CU -- nothing else hides the ~5 us it
    // takes to retire a 16-wave, 160 KB workgroup and launch the next (512x512x200, 500 k events:
    // 0.232 -> 0.222 ms).  With two per CU the hardware dispatcher already overlaps them and the item
    // loop only adds a barrier and an atomic (346x260x100: 1.175 ms plain, 1.204 ms persistent).
    const bool two_per_cu = bp->lds_bytes * 2 <= dsi::max_dynamic_lds() && bp->block_threads <= 1024;
    bp->persistent = ((bp->packed == 1 || bp->packed == 3 || bp->packed == 5 || bp->packed == 6 || bp->packed == 7 || bp->packed == 8) && !two_per_cu) ? 1 : 0;
    bp->experiment = 0;
    bp->pass_lg = (m->want_pass_lg >= 1 && m->want_pass_lg <= 6) ? m->want_pass_lg : 0;  // test hook dsi_test_pass_lg
#ifdef DSI_TIMING_EXPERIMENTS
    // Environment knobs of the timing experiments quoted in NOTEBOOK.md.  They are compiled in ONLY by
    // `python -m dvs_mcemvs_amd.build --experiments` (a stray variable in a job's environment must
    // not be able to change -- DSI_EXPERIMENT: corrupt -- the results of the production library).
    if (const char* e = std::getenv("DSI_PERSISTENT")) {  // A/B: 0 off, 1 on wherever the kernel supports it
        const int v = std::atoi(e);
        bp->persistent = (v != 0 && (bp->packed == 1 || bp->packed == 3 || bp->packed == 5 || bp->packed == 6 || bp->packed == 7)) ? 1 : 0;
    }
    if (const char* e = std::getenv("DSI_EXPERIMENT")) {  // 1 no votes, 2 no flush: WRONG results, timing only
        bp->experiment = std::atoi(e);
        static bool warned = false;
        if (!warned && bp->experiment) {
            std::fprintf(stderr, "dsi_engine: DSI_EXPERIMENT=%d -- timing experiment, the DSIs are WRONG\n", bp->experiment);
            warned = true;
        }
    }
    if (const char* e = std::getenv("DSI_PASS_LG")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 6) bp->pass_lg = v;
    }
#endif
    int chunks = m->want_chunks;
    if (chunks <= 0) {
        // Work items = chunks x bands x planes: ~8 per CU keep the tail of the last round short; every
        // chunk beyond the first costs a partial volume to write and to reduce.
        // (round 3: a chunk's partial volume holds raw 64-bit sums, 8 bytes per voxel to write and to read back, so
        //  fewer chunks than in round 2: 346x260x100, 10 M events: 1 / 2 / 4 chunks 2.695 / 2.668 / 2.717 ms per step)
        const long items_target = 4L * 256;
        chunks = (int)std::max<long>(1, (items_target + (long)bands * g.nz - 1) / ((long)bands * g.nz));
        // below ~8 M events one chunk is faster when the planes alone fill the chip 1.5 times: no
        // partial volumes to write and reduce, fewer workgroup set-ups (measured at 346x260x100:
        // 1.85x at 0.1 M events, 1.25x at 1 M, 1.03x at 5 M, 0.99x at 10 M)
        // (round 3, dealt passes + raw partial volumes: one chunk also at 10 M events -- 346x260x100, same box,
        //  1 / 2 / 3 / 4 chunks: 2.633 / 2.675 / 2.717 / 2.751 ms per step)
        if ((long)bands * g.nz >= 768) chunks = 1;
        // keep (chunks * bands) a multiple of 8 so that all XCDs get the same number of pairs
        int step = 8;
        for (int f = 2; f <= 8; f *= 2)
            if (bands % f == 0) step = 8 / f;
        if (chunks > 1) {  // whole groups of 8 pairs -- unless that multiplies the partial volumes (an odd
                           // number of bands would turn 2 chunks into 8: 640x480x100 with 17 bands paid
                           // 0.3 ms per step for it); the pairs beyond the last whole group are dealt plane
                           // by plane over all XCDs anyway
            const int rounded = ((chunks + step - 1) / step) * step;
            if (rounded <= chunks + chunks / 2) chunks = rounded;
        }
        chunks = (int)std::min<size_t>((size_t)chunks, std::max<size_t>(1, n_packets));
        const size_t vol_bytes = (size_t)g.nx * g.ny * g.nz * sizeof(float);
        const size_t budget = (size_t)16 << 30;  // partial DSIs (8 bytes per voxel) may use up to 16 GiB of HBM
        while (chunks > 1 && (size_t)chunks * (2 * vol_bytes + 32) > budget) --chunks;
    }
    bp->chunks = std::max(1, chunks);
    return true;
}

// Band decomposition of the fused vote -> camera fusion -> arg-max kernel (k_vote_fuse_argmax): one
// 1024-thread workgroup per CU, the band as tall as the LDS (and the per-thread register arrays) allow,
// a halo row on either side of the owned rows instead of a carry row, one chunk.
// max_cells (k_vote_fuse_argmax_alg2): cells per 1024-thread workgroup the kernel of mapping m keeps in registers, 0 = the fused
// kernel's own (dsi::fused_max_cells)
bool plan_fused(const dsi_mapper* m, size_t n_packets_max, dsi::BandPlan* bp, int n_cameras = 2,
                size_t (*max_cells)(int mapping) = nullptr)
{
    auto cells = [&](int mapping) { return max_cells ? max_cells(mapping) : dsi::fused_max_cells(mapping, n_cameras); };
    const dsi::Geom& g = m->geom;
    const size_t row_bytes = (size_t)g.nx * sizeof(unsigned long long);
    if (g.nx < 2 || g.ny < 2 || g.ny > 16000 || g.nz > 256) return false;
    int packed = m->want_packed;
    if (!(packed == 1 || packed == 3 || packed == 5 || packed == 6)) {
        // the rule of plan_bands for one workgroup per CU: vector fill below ~72 records per (packet, band)
        const long rows_full = (long)std::min(dsi::max_dynamic_lds() / row_bytes, cells(1) / (size_t)g.nx);
        packed = 1024L * rows_full / g.ny < 72 ? 5 : 1;
    }
    // the hand-scheduled loops address records with 32-bit byte offsets (see vote_device)
    if ((n_packets_max + 1) * dsi::kPacket * sizeof(dsi::EvRec) > 0xffffffffull) packed = packed == 1 ? 3 : (packed == 5 ? 6 : packed);
    const size_t scratch_bytes = (packed == 5 || packed == 6) ? (size_t)(1024 / 64) * dsi::kVfillScratchWords * 8 : 0;
    const long max_rows_total =
        (long)std::min((dsi::max_dynamic_lds() - scratch_bytes) / row_bytes, cells(packed) / (size_t)g.nx);
    if (max_rows_total < 3) return false;
    long max_owned = max_rows_total - 2;  // + the two halo rows
    if (m->want_band_rows > 0) max_owned = std::min<long>(max_owned, m->want_band_rows);
    int bands = (int)((g.ny + max_owned - 1) / max_owned);
    int band_rows = (g.ny + bands - 1) / bands;  // balanced
    if (m->want_band_rows > 0) band_rows = (int)max_owned;
    bands = (g.ny + band_rows - 1) / band_rows;
    *bp = dsi::BandPlan{};
    bp->bands = bands;
    bp->band_rows = band_rows;
    bp->chunks = 1;
    bp->block_threads = 1024;
    bp->packed = packed;
    bp->group_packets = 1;
    bp->row_pad = std::min(g.ny, 4096);
    bp->pass_lg = (m->want_pass_lg >= 1 && m->want_pass_lg <= 6) ? m->want_pass_lg : 0;
    bp->scratch_offset = (int)((size_t)(band_rows + 2) * row_bytes);
    bp->lds_bytes = (size_t)(band_rows + 2) * row_bytes + scratch_bytes;
    bp->persistent = 0;
    bp->halo = 1;
    bp->experiment = 0;
    bp->interleave = -1;  // decided by the caller from the cameras' packet counts (depth_map_of_events_impl)
#ifdef DSI_TIMING_EXPERIMENTS
    if (const char* e = std::getenv("DSI_FUSED_2CU"))  // 0: a small band still runs one workgroup per CU (A/B)
        if (std::atoi(e) == 0) bp->experiment = 300;
    if (const char* e = std::getenv("DSI_FUSED_DEFER"))  // 0: camera 1's fusion + arg-max inside its read-back, as before round 6 (A/B)
        if (std::atoi(e) == 0) bp->experiment = 301;
    if (const char* e = std::getenv("DSI_FUSED_INTERLEAVE"))  // A/B: 0 contiguous pieces, 1 pairs in turn, 2 pairs drawn
        bp->interleave = std::min(2, std::max(0, std::atoi(e)));
#endif
    return true;
}

int upload_async(dsi_context* ctx, void* dst, const void* src, size_t bytes)
{
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return DSI_OK;
}

Event timing_event(dsi_mapper* m)
{
    Event e;
    if (!m->timing_pool.empty()) {
        e = std::move(m->timing_pool.back());
        m->timing_pool.pop_back();
    } else {
        (void)e.create(hipEventDefault);  // (empty on failure: the launch goes untimed)
    }
    return e;
}

struct VoteTimer {  // records an event pair around the voting kernel when timing is on
    dsi_mapper* m;
    Event a, b;
    explicit VoteTimer(dsi_mapper* m_) : m(m_)
    {
        if (!m->timing) return;
        a = timing_event(m);
        b = timing_event(m);
        if (a && b) (void)hipEventRecord(a, m->ctx->stream);
    }
    void stop()
    {
        if (!a || !b) return;
        (void)hipEventRecord(b, m->ctx->stream);
        m->timing_pairs.push_back(std::move(a));
        m->timing_pairs.push_back(std::move(b));
    }
};

// The stream the preparation kernels of an evaluate call go to: the mapper's own second stream,
// ordered after this mapper's previous vote (which still reads the scratch tables), or the
// context's stream when overlapping is off.
int prep_begin(dsi_mapper* m, hipStream_t* ps)
{
    *ps = m->ctx->stream;
    if (!m->prep_overlap) return DSI_OK;
    if (!m->prep_stream) {
        HIP_TRY(m->prep_stream.create(hipStreamNonBlocking));
        HIP_TRY(m->ev_prep.create(hipEventDisableTiming));
        HIP_TRY(m->ev_vote_done.create(hipEventDisableTiming));
    }
    if (m->vote_recorded) HIP_TRY(hipStreamWaitEvent(m->prep_stream, m->ev_vote_done, 0));
    *ps = m->prep_stream;
    return DSI_OK;
}

// the context's stream continues only after the preparation kernels
int prep_end(dsi_mapper* m, hipStream_t ps)
{
    if (ps == m->ctx->stream) return DSI_OK;
    HIP_TRY(hipEventRecord(m->ev_prep, ps));
    HIP_TRY(hipStreamWaitEvent(m->ctx->stream, m->ev_prep, 0));
    return DSI_OK;
}

int vote_done(dsi_mapper* m)
{
    if (!m->prep_stream) return DSI_OK;
    HIP_TRY(hipEventRecord(m->ev_vote_done, m->ctx->stream));
    m->vote_recorded = true;
    return DSI_OK;
}

// before a kernel overwrites the mapper's depth-map buffers: the previous fetch must have read them
int depth_buffers_acquire(dsi_mapper* m)
{
    if (m->depth_read_pending) {
        HIP_TRY(hipStreamWaitEvent(m->ctx->stream, m->ev_depth_read, 0));
        m->depth_read_pending = false;
    }
    return DSI_OK;
}

// after the kernels that produce the depth map have been queued on the mapper's stream
int depth_buffers_ready(dsi_mapper* m)
{
    if (!m->ev_depth_ready) {
        HIP_TRY(m->ev_depth_ready.create(hipEventDisableTiming));
        // (the in-order fetch STORES the maps into mapped host memory from a kernel: the event that says "read" must
        //  release those stores to the system, or the host may see stale maps in non-coherent pinned memory -- ADVICE r05)
        HIP_TRY(m->ev_depth_read.create(hipEventDisableTiming | hipEventReleaseToSystem));
    }
    HIP_TRY(hipEventRecord(m->ev_depth_ready, m->ctx->stream));
    m->depth_valid = true;
    m->filtered_valid = false;
    return DSI_OK;
}

// device -> host copies of the depth map: on the context's copy stream behind the arg-max only (see
// dsi_mapper::ev_depth_ready), or -- in_order -- on the compute stream behind whatever it holds
int depth_buffers_fetch(dsi_mapper* m, float* depth_host, float* conf_host, uint8_t* idx_host, bool wait, bool in_order = false)
{
    dsi_context* ctx = m->ctx;
    hipStream_t cs = ctx->stream;
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    if (!in_order) {
        HIP_TRY(copy_stream_of(ctx, &cs));
        HIP_TRY(hipStreamWaitEvent(cs, m->ev_depth_ready, 0));
    } else {
        // destinations in mapped page-locked memory (dsi_host_alloc): the CUs store the maps there, no copy engine involved
        // (a device -> host copy queued behind this window's kernel would hold up the next window's uploads)
        auto mapped = [](void* host, void** dev) {
            *dev = nullptr;
            if (!host) return true;
            hipPointerAttribute_t attr{};
            if (hipPointerGetAttributes(&attr, host) != hipSuccess) {
                (void)hipGetLastError();  // (an ordinary pointer: not an error of ours)
                return false;
            }
            if (attr.type != hipMemoryTypeHost) return false;
            return hipHostGetDevicePointer(dev, host, 0) == hipSuccess && *dev;
        };
        void *dd = nullptr, *dc = nullptr, *di = nullptr;
        // (the kernel stores the index map as 32-bit words: an interior, misaligned idx_host takes the copy path below)
        if (mapped(depth_host, &dd) && mapped(conf_host, &dc) && mapped(idx_host, &di) && npix % 4 == 0 &&
            reinterpret_cast<uintptr_t>(di) % 4 == 0) {
            HIP_TRY(dsi::launch_store_depth_map(cs, m->depth.p, m->conf.p, m->idx.p, npix, static_cast<float*>(dd),
                                                static_cast<float*>(dc), static_cast<uint8_t*>(di)));
            HIP_TRY(hipEventRecord(m->ev_depth_read, cs));
            m->depth_read_pending = true;
            if (wait) HIP_TRY(hipEventSynchronize(m->ev_depth_read));
            return DSI_OK;
        }
    }
    if (depth_host) HIP_TRY(hipMemcpyAsync(depth_host, m->depth.p, npix * sizeof(float), hipMemcpyDeviceToHost, cs));
    if (conf_host) HIP_TRY(hipMemcpyAsync(conf_host, m->conf.p, npix * sizeof(float), hipMemcpyDeviceToHost, cs));
    if (idx_host) HIP_TRY(hipMemcpyAsync(idx_host, m->idx.p, npix, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(m->ev_depth_read, cs));
    m->depth_read_pending = true;
    if (wait) HIP_TRY(hipEventSynchronize(m->ev_depth_read));
    return DSI_OK;
}

// fillVoxelGrid on device data.  xy: np*1024 z0 locations (reference order);
// centers: np*3.  accumulate != 0: add to the grid's current contents.  ps: the stream the sort and
// coefficient kernels go to (see prep_begin); the caller has already put xy / centers on it.
int vote_device(dsi_mapper* m, const float2* xy, const float* centers, size_t np, bool accumulate,
                hipStream_t ps, const dsi_batch* raw = nullptr)
{
    // raw != nullptr: the events of `raw` have not been through stage A yet (xy / centers are the
    // mapper's buffers to fill).  The LDS-band path with per-packet sorting does stage A inside the
    // sort kernel; the other paths run the two stage-A kernels first.
    auto stage_a = [&]() -> int {
        if (!raw || np == 0) return DSI_OK;
        HIP_TRY(m->H.reserve(np * 9));
        HIP_TRY(m->xy.reserve(np * dsi::kPacket));
        HIP_TRY(dsi::launch_packet_geometry(ps, raw->Rt, (int)np, m->geom, m->centers.p, m->H.p));
        HIP_TRY(dsi::launch_warp_z0(ps, raw->x, raw->y, raw->first, (int)np, m->H.p, m->lut_dev.p, m->sensor_w, m->sensor_h,
                                    m->xy.p));
        xy = m->xy.p;
        return DSI_OK;
    };
    dsi_context* ctx = m->ctx;
    dsi_grid* g = m->grid;
    const dsi::Geom& geom = m->geom;
    dsi::BandPlan bp{};
    int algo = m->algo;
    const bool can_band = plan_bands(m, np, &bp);
    if (algo == DSI_VOTE_AUTO) algo = can_band ? DSI_VOTE_LDS_BANDS : DSI_VOTE_GLOBAL_ATOMIC;
    if (algo == DSI_VOTE_LDS_BANDS && !can_band)
        return fail(DSI_ERR_INVALID, "grid rows of %d floats do not fit the LDS band kernel", geom.nx);

    m->info = dsi_vote_info_t{};
    m->info.algo = algo;
    m->info.n_packets = np;
    m->depth_valid = false;

    if (algo == DSI_VOTE_GLOBAL_ATOMIC) {
        if (int rc = stage_a()) return rc;
        if (int rc = prep_end(m, ps)) return rc;
        if (!accumulate) HIP_TRY(hipMemsetAsync(g->data, 0, g->n * sizeof(float), ctx->stream));
        VoteTimer vt(m);
        HIP_TRY(dsi::launch_vote_global(ctx->stream, xy, centers, (int)np, m->planes_dev.p, geom, g->data));
        vt.stop();
        return vote_done(m);
    }

    // the hand-scheduled loops address records with 32-bit byte offsets (12 B per record):
    // beyond 2^32 / 12 records (349,525 packets = 358 M events in ONE call) use the compiled loops
    if ((np + 1) * dsi::kPacket * sizeof(dsi::EvRec) > 0xffffffffull) {
        if (bp.packed == 1 || bp.packed == 7) bp.packed = 3;
        if (bp.packed == 8) return fail(DSI_ERR_INVALID, "lane mapping 8 (paired cells) addresses records with 32 bits: %zu packets are too many", np);
        if (bp.packed == 4) bp.packed = 2;
        if (bp.packed == 5) bp.packed = 6;
    }

    m->info.bands = bp.bands;
    m->info.band_rows = bp.band_rows;
    m->info.chunks = bp.chunks;
    m->info.block_threads = bp.block_threads;
    m->info.lds_bytes = bp.lds_bytes;
    m->info.packed = bp.packed;
    m->info.group_packets = bp.group_packets;
    if (np == 0) {
        if (int rc = prep_end(m, ps)) return rc;
        if (!accumulate) HIP_TRY(hipMemsetAsync(g->data, 0, g->n * sizeof(float), ctx->stream));
        return vote_done(m);
    }
    HIP_TRY(m->sxy.reserve(np * dsi::kPacket + 1));  // + the multiplicity-0 dummy record
    HIP_TRY(m->nvalid.reserve(np + (size_t)geom.nz + 9));  // + one "needs IEEE divide" word per plane + 8 work counters + the paired cells' overflow word
    HIP_TRY(m->rowstart.reserve(np * (size_t)(geom.ny + 2 * bp.row_pad + 3) + 2));  // (+ slack: k_plane_coef copies 32-bit words)
    HIP_TRY(m->coef.reserve(np * geom.nz + 1));       // + the dummy record's "coefficients"
    // Wide grids with many packets (the vector fill): no cut table -- at 1024 x 1024 x 256 with 100 M events it is 6.1 GB per
    // camera and 3.9 ms to write -- but the packets' row tables transposed (u16 [ny + 2 pad + 3][stride], 0.6 GB there), from
    // which the voting kernel's passes derive their runs (BandPlan::cuts_inline).  Below ~8 k packets the table stays: a work
    // item is then short and the two dependent look-ups at its start would show.
    bp.rs_stride = (int)((np + 63) / 64 * 64);
    // (the voting kernel addresses the transposed table with 32-bit byte offsets)
    const bool rs_fits = (size_t)(geom.ny + 2 * bp.row_pad + 3) * (size_t)bp.rs_stride * 2 < ((size_t)1 << 32);
    bp.cuts_inline = ((bp.packed == 5 || bp.packed == 6) && np >= (size_t)m->cuts_inline_min_packets && rs_fits) ? 1 : 0;
    if (bp.cuts_inline)
        HIP_TRY(m->cuts.reserve(((size_t)(geom.ny + 2 * bp.row_pad + 3) * (size_t)bp.rs_stride + 1) / 2));  // (u16 entries in u32 words)
    else
        HIP_TRY(m->cuts.reserve(np * geom.nz * bp.bands));
    m->info_cuts_inline = bp.cuts_inline != 0;
    HIP_TRY(m->seam.reserve((size_t)bp.chunks * geom.nz * bp.bands * 2 * geom.nx));
    const bool direct = (bp.chunks == 1 && !accumulate);
    bp.raw_out = direct ? 0 : 1;
    if (!direct) HIP_TRY(m->partials.reserve((size_t)bp.chunks * dsi::partial_stride(g->n)));

    if (bp.packed == 2 || bp.packed == 4) {
        if (int rc = stage_a()) return rc;
        const int S = bp.group_packets;
        const size_t ngroups = (np + S - 1) / S;
        HIP_TRY(m->spk.reserve(np * dsi::kPacket));
        HIP_TRY(m->gcuts.reserve(ngroups * geom.nz * bp.bands));
        HIP_TRY(m->rowstart.reserve(ngroups * (size_t)(geom.ny + 2 * bp.row_pad + 3)));
        HIP_TRY(dsi::launch_sort_groups(ps, xy, (int)np, S, geom.ny, geom.nz, bp.row_pad, m->sxy.p, m->spk.p,
                                        m->nvalid.p, m->rowstart.p));
        // per-packet coefficients + row-bin ranges (cuts buffer), then the per-group runs
        HIP_TRY(dsi::launch_plane_coef(ps, centers, m->planes_dev.p, m->rowstart.p, m->nvalid.p, (int)np,
                                       geom, bp, m->coef.p, m->cuts.p));
        HIP_TRY(dsi::launch_group_cuts(ps, m->cuts.p, m->rowstart.p, (int)np, S, geom, bp, m->gcuts.p));
        if (int rc = prep_end(m, ps)) return rc;
        VoteTimer vt(m);
        HIP_TRY(dsi::launch_vote_groups(ctx->stream, m->sxy.p, m->spk.p, m->coef.p, m->gcuts.p, m->nvalid.p + np, (int)np, S, geom,
                                        bp, direct ? (void*)g->data : (void*)m->partials.p, m->seam.p));
        vt.stop();
    } else {
    if (raw && !m->keep_z0) {
        HIP_TRY(dsi::launch_sort_packets_raw(ps, raw->Rt, raw->x, raw->y, raw->first, m->lut_dev.p, m->sensor_w, m->sensor_h, geom,
                                             m->centers.p, (int)np, bp.row_pad, m->sxy.p, m->nvalid.p,
                                             m->rowstart.p, m->unit_multiplicity));
    } else {
        if (int rc = stage_a()) return rc;
        HIP_TRY(dsi::launch_sort_packets(ps, xy, (int)np, geom.ny, geom.nz, bp.row_pad, m->sxy.p, m->nvalid.p,
                                         m->rowstart.p));
    }
    HIP_TRY(dsi::launch_plane_coef(ps, centers, m->planes_dev.p, m->rowstart.p, m->nvalid.p, (int)np,
                                   geom, bp, m->coef.p, m->cuts.p));
    if (int rc = prep_end(m, ps)) return rc;
    VoteTimer vt(m);
    HIP_TRY(dsi::launch_vote_bands(ctx->stream, m->sxy.p, m->coef.p, m->cuts.p, m->nvalid.p + np, (int)np, geom, bp,
                                   direct ? (void*)g->data : (void*)m->partials.p, m->seam.p));
    vt.stop();
    }
    // seam rows from the exact 64-bit sums of the two bands that meet there; then (several chunks, or accumulation) the
    // sum over the chunks' raw partial volumes -- which takes the seam rows straight from the bands' sums when it can
    const bool fold = !direct && dsi::reduce_can_fold_seams(geom, g->n);
    if (!fold)
        HIP_TRY(dsi::launch_seam_rows(ctx->stream, m->seam.p, bp.chunks, geom, bp, direct ? (void*)g->data : (void*)m->partials.p));
    if (!direct)
        HIP_TRY(dsi::launch_reduce_partials(ctx->stream, m->partials.p, bp.chunks, g->n, g->data, accumulate ? 1 : 0,
                                            fold ? m->seam.p : nullptr, &geom, &bp));
    return vote_done(m);
}

bool same_shape(const dsi_grid* a, const dsi_grid* b)
{
    return a->nx == b->nx && a->ny == b->ny && a->nz == b->nz;
}

}  // namespace

extern "C" {

const char* dsi_last_error(void) { return g_last_error.c_str(); }
int dsi_abi_version(void) { return DSI_ENGINE_ABI_VERSION; }

int dsi_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ------------------------------------------------------------------ context */
int dsi_context_create(int device_id, dsi_context_t** out)
{
    REQUIRE(out, DSI_ERR_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(DSI_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
    REQUIRE(device_id >= 0 && device_id < n, DSI_ERR_NO_DEVICE, "device %d out of range (%d devices)",
            device_id, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DSI_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 only", device_id,
                    prop.gcnArchName);
    HIP_TRY(hipSetDevice(device_id));
    dsi_context* ctx = new (std::nothrow) dsi_context();
    REQUIRE(ctx, DSI_ERR_INVALID, "out of host memory");
    ctx->device = device_id;
    hipError_t e = ctx->stream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = upload_stream_acquire(device_id, &ctx->upload_stream);
    if (e == hipSuccess) e = ctx->t0.create(hipEventDefault);
    if (e == hipSuccess) e = ctx->t1.create(hipEventDefault);
    if (e == hipSuccess) e = ctx->ms_accum.reserve(1);
    if (e != hipSuccess) {
        delete ctx;
        return fail(DSI_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return DSI_OK;
}

int dsi_context_destroy(dsi_context_t* ctx)
{
    if (!ctx) return DSI_OK;
    REQUIRE(ctx->children.load() == 0, DSI_ERR_CONTEXT,
            "%d object(s) created from this context (grids, mappers, batches, scores, projectors) are still alive: destroy them first",
            ctx->children.load());
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->upload_stream) (void)hipStreamSynchronize(ctx->upload_stream);
    delete ctx;
    return DSI_OK;
}

int dsi_context_synchronize(dsi_context_t* ctx)
{
    REQUIRE(ctx, DSI_ERR_INVALID, "ctx is null");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DSI_OK;
}

int dsi_context_wait_for(dsi_context_t* ctx, dsi_context_t* other)
{
    REQUIRE(ctx && other, DSI_ERR_INVALID, "ctx is null");
    REQUIRE(ctx->device == other->device, DSI_ERR_INVALID, "contexts are on different devices");
    if (ctx == other) return DSI_OK;
    if (int rc = set_device(ctx)) return rc;
    if (!other->sync_ev) HIP_TRY(other->sync_ev.create(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(other->sync_ev, other->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, other->sync_ev, 0));
    return DSI_OK;
}

void* dsi_context_stream(dsi_context_t* ctx) { return ctx ? (void*)ctx->stream.h : nullptr; }
int dsi_context_device(dsi_context_t* ctx) { return ctx ? ctx->device : -1; }

int dsi_context_timer_start(dsi_context_t* ctx)
{
    REQUIRE(ctx, DSI_ERR_INVALID, "ctx is null");
    HIP_TRY(hipEventRecord(ctx->t0, ctx->stream));
    return DSI_OK;
}

int dsi_context_timer_stop(dsi_context_t* ctx, float* elapsed_ms)
{
    REQUIRE(ctx && elapsed_ms, DSI_ERR_INVALID, "null argument");
    HIP_TRY(hipEventRecord(ctx->t1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->t1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, ctx->t0, ctx->t1));
    return DSI_OK;
}

int dsi_context_timeline_mark(dsi_context_t* ctx)
{
    REQUIRE(ctx, DSI_ERR_INVALID, "context is null");
    if (int rc = set_device(ctx)) return rc;
    if (ctx->n_marks == ctx->marks.size()) {
        Event e;
        HIP_TRY(e.create(hipEventDefault));
        ctx->marks.push_back(std::move(e));
    }
    HIP_TRY(hipEventRecord(ctx->marks[ctx->n_marks], ctx->stream));
    ++ctx->n_marks;
    return DSI_OK;
}

int dsi_context_timeline_read(dsi_context_t* ctx, float* intervals_ms, size_t capacity, size_t* n_intervals)
{
    REQUIRE(ctx && n_intervals, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    const size_t n = ctx->n_marks > 0 ? ctx->n_marks - 1 : 0;
    *n_intervals = n;
    if (ctx->n_marks) HIP_TRY(hipEventSynchronize(ctx->marks[ctx->n_marks - 1]));
    for (size_t i = 0; i < n && i < capacity && intervals_ms; ++i)
        HIP_TRY(hipEventElapsedTime(&intervals_ms[i], ctx->marks[i], ctx->marks[i + 1]));
    ctx->n_marks = 0;
    return DSI_OK;
}

/* ------------------------------------------------------------------- Grid3D */
static int grid_make(dsi_context_t* ctx, int nx, int ny, int nz, void* wrap, dsi_grid_t** out)
{
    REQUIRE(ctx && out, DSI_ERR_INVALID, "null argument");
    *out = nullptr;
    REQUIRE(nx > 0 && ny > 0 && nz > 0, DSI_ERR_INVALID, "grid dimensions must be positive (%d,%d,%d)", nx,
            ny, nz);
    if (int rc = set_device(ctx)) return rc;
    dsi_grid* g = new (std::nothrow) dsi_grid();
    REQUIRE(g, DSI_ERR_INVALID, "out of host memory");
    g->ctx = ctx;
    g->nx = nx;
    g->ny = ny;
    g->nz = nz;
    g->n = (size_t)nx * ny * nz;
    if (wrap) {
        g->data = static_cast<float*>(wrap);
    } else {
        hipError_t e = g->own.reserve(g->n);
        if (e == hipSuccess) e = hipMemsetAsync(g->own.p, 0, g->n * sizeof(float), ctx->stream);
        if (e != hipSuccess) {
            const size_t bytes = g->n * sizeof(float);
            delete g;
            return fail(DSI_ERR_HIP, "grid allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        }
        g->data = g->own.p;
    }
    ++ctx->children;
    *out = g;
    return DSI_OK;
}

int dsi_grid_create(dsi_context_t* ctx, int nx, int ny, int nz, dsi_grid_t** out)
{
    return grid_make(ctx, nx, ny, nz, nullptr, out);
}

int dsi_grid_wrap(dsi_context_t* ctx, int nx, int ny, int nz, void* data_dev, dsi_grid_t** out)
{
    REQUIRE(data_dev, DSI_ERR_INVALID, "data_dev is null");
    // the voxel-wise kernels sweep volumes as float4
    REQUIRE((reinterpret_cast<uintptr_t>(data_dev) & 15u) == 0, DSI_ERR_INVALID,
            "wrapped device memory must be 16-byte aligned");
    return grid_make(ctx, nx, ny, nz, data_dev, out);
}

int dsi_grid_destroy(dsi_grid_t* g)
{
    if (!g) return DSI_OK;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    --g->ctx->children;
    delete g;
    return DSI_OK;
}

int dsi_grid_dims(const dsi_grid_t* g, int* nx, int* ny, int* nz)
{
    REQUIRE(g, DSI_ERR_INVALID, "grid is null");
    if (nx) *nx = g->nx;
    if (ny) *ny = g->ny;
    if (nz) *nz = g->nz;
    return DSI_OK;
}

int dsi_grid_reset(dsi_grid_t* g)
{
    REQUIRE(g, DSI_ERR_INVALID, "grid is null");
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(hipMemsetAsync(g->data, 0, g->n * sizeof(float), g->ctx->stream));
    return DSI_OK;
}

void* dsi_grid_device_ptr(dsi_grid_t* g) { return g ? g->data : nullptr; }

int dsi_grid_upload(dsi_grid_t* g, const float* host)
{
    REQUIRE(g && host, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(g->data, host, g->n * sizeof(float), hipMemcpyHostToDevice, g->ctx->stream));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    return DSI_OK;
}

int dsi_grid_download(dsi_grid_t* g, float* host)
{
    REQUIRE(g && host, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(host, g->data, g->n * sizeof(float), hipMemcpyDeviceToHost, g->ctx->stream));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    return DSI_OK;
}

static int check_pair(const dsi_grid_t* dst, const dsi_grid_t* src)
{
    REQUIRE(dst && src, DSI_ERR_INVALID, "null grid");
    // grids of two contexts (streams) of one device may be combined: the op runs on dst's stream and
    // the caller orders the streams (dsi_context_wait_for)
    REQUIRE(dst->ctx->device == src->ctx->device, DSI_ERR_CONTEXT, "grids live on different devices");
    REQUIRE(same_shape(dst, src), DSI_ERR_SHAPE, "grid shapes differ: (%d,%d,%d) vs (%d,%d,%d)", dst->nx,
            dst->ny, dst->nz, src->nx, src->ny, src->nz);
    return set_device(dst->ctx);
}

int dsi_grid_fuse2(dsi_grid_t* dst, const dsi_grid_t* src, int op)
{
    if (int rc = check_pair(dst, src)) return rc;
    REQUIRE(op >= 1 && op <= 6, DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    HIP_TRY(dsi::launch_fuse2(dst->ctx->stream, dst->data, src->data, dst->n, op));
    return DSI_OK;
}

int dsi_grid_fuse2_into(dsi_grid_t* dst, const dsi_grid_t* a, const dsi_grid_t* b, int op)
{
    if (int rc = check_pair(dst, a)) return rc;
    if (int rc = check_pair(dst, b)) return rc;
    REQUIRE(op >= 1 && op <= 6, DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    REQUIRE(dst != a && dst != b, DSI_ERR_INVALID, "dst must differ from the operands (use dsi_grid_fuse2 in place)");
    HIP_TRY(dsi::launch_fuse2_into(dst->ctx->stream, dst->data, a->data, b->data, dst->n, op));
    return DSI_OK;
}

int dsi_grid_fuse_hm_n(dsi_grid_t* dst, const dsi_grid_t* src, int n)
{
    if (int rc = check_pair(dst, src)) return rc;
    REQUIRE(n >= 2, DSI_ERR_INVALID, "n-ary harmonic mean needs n >= 2 (got %d)", n);
    HIP_TRY(dsi::launch_fuse_hm_n(dst->ctx->stream, dst->data, src->data, dst->n, n));
    return DSI_OK;
}

static bool valid_acc_mode(int mode) { return mode >= DSI_ACC_SUM && mode <= DSI_ACC_MAX; }
// the one-pass n-ary fusions also take DSI_ACC_GM_TREE (n = 2, 4, 8): not an accumulation, so not in the streaming API
static bool valid_fuse_n_mode(int mode, int n)
{
    return valid_acc_mode(mode) || (mode == DSI_ACC_GM_TREE && (n == 2 || n == 4 || n == 8));
}

int dsi_acc_reduce_op(int mode)
{
    if (!valid_acc_mode(mode)) return -1;
    if (mode == DSI_ACC_MIN) return DSI_REDUCE_MIN;
    if (mode == DSI_ACC_MAX) return DSI_REDUCE_MAX;
    return DSI_REDUCE_SUM;
}

int dsi_grid_accumulate_begin(dsi_grid_t* dst, int mode)
{
    REQUIRE(dst, DSI_ERR_INVALID, "grid is null");
    REQUIRE(valid_acc_mode(mode), DSI_ERR_BAD_OP, "bad accumulate mode %d", mode);
    if (int rc = set_device(dst->ctx)) return rc;
    if (mode == DSI_ACC_MIN || mode == DSI_ACC_MAX) {
        const float v = mode == DSI_ACC_MIN ? INFINITY : -INFINITY;
        HIP_TRY(dsi::launch_fill(dst->ctx->stream, dst->data, dst->n, v));
    } else {
        HIP_TRY(hipMemsetAsync(dst->data, 0, dst->n * sizeof(float), dst->ctx->stream));
    }
    return DSI_OK;
}

int dsi_grid_accumulate(dsi_grid_t* dst, const dsi_grid_t* src, int mode)
{
    if (int rc = check_pair(dst, src)) return rc;
    REQUIRE(valid_acc_mode(mode), DSI_ERR_BAD_OP, "bad accumulate mode %d", mode);
    HIP_TRY(dsi::launch_accumulate(dst->ctx->stream, dst->data, src->data, dst->n, mode));
    return DSI_OK;
}

int dsi_grid_fuse_n(dsi_grid_t* dst, const dsi_grid_t* const* srcs, int n, int mode)
{
    REQUIRE(dst && srcs, DSI_ERR_INVALID, "null argument");
    REQUIRE(valid_fuse_n_mode(mode, n), DSI_ERR_BAD_OP, "bad fusion mode %d for %d grids (DSI_ACC_GM_TREE needs 2, 4 or 8)", mode, n);
    REQUIRE(n >= 1 && n <= 8, DSI_ERR_INVALID, "1 <= n <= 8 sources (got %d)", n);
    const float* ptrs[8];
    for (int i = 0; i < n; ++i) {
        if (int rc = check_pair(dst, srcs[i])) return rc;
        REQUIRE(srcs[i] != dst, DSI_ERR_INVALID, "dst must not be one of the sources");
        ptrs[i] = srcs[i]->data;
    }
    HIP_TRY(dsi::launch_fuse_n(dst->ctx->stream, dst->data, ptrs, n, dst->n, mode));
    return DSI_OK;
}

int dsi_grid_finalize(dsi_grid_t* dst, int mode, int n)
{
    REQUIRE(dst, DSI_ERR_INVALID, "grid is null");
    REQUIRE(valid_acc_mode(mode), DSI_ERR_BAD_OP, "bad finalize mode %d", mode);
    REQUIRE(n >= 1, DSI_ERR_INVALID, "number of maps must be >= 1 (got %d)", n);
    if (int rc = set_device(dst->ctx)) return rc;
    HIP_TRY(dsi::launch_finalize(dst->ctx->stream, dst->data, dst->n, mode, n));
    return DSI_OK;
}

int dsi_grid_collapse_max_z_dev(dsi_grid_t* g, float* conf_dev, uint8_t* idx_dev, const float* planes_dev,
                                float* depth_dev)
{
    REQUIRE(g && conf_dev && idx_dev, DSI_ERR_INVALID, "null argument");
    REQUIRE(g->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", g->nz);
    REQUIRE(!depth_dev || planes_dev, DSI_ERR_INVALID, "depth output needs the plane depths");
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(dsi::launch_collapse_max_z(g->ctx->stream, g->data, g->nx, g->ny, g->nz, conf_dev, idx_dev,
                                       planes_dev, depth_dev));
    return DSI_OK;
}

// the context's grow-only scratch of the host-output collapses: conf[npix] f32 + idx[npix] u8
static int collapse_scratch(dsi_context* ctx, size_t npix, float** conf, uint8_t** idx)
{
    const size_t need = npix * sizeof(float) + npix;
    if (ctx->collapse_scratch.cap < need) {
        if (ctx->collapse_scratch.p) HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx->collapse_scratch.reserve(need));  // (growth frees first)
    }
    *conf = reinterpret_cast<float*>(ctx->collapse_scratch.p);
    *idx = reinterpret_cast<uint8_t*>(*conf + npix);
    return DSI_OK;
}

// copy a collapse's outputs from the scratch to the host and wait
static int collapse_download(dsi_context* ctx, size_t npix, const float* conf, const uint8_t* idx, float* conf_host,
                             uint8_t* idx_host)
{
    HIP_TRY(hipMemcpyAsync(conf_host, conf, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(idx_host, idx, npix, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DSI_OK;
}

int dsi_grid_collapse_max_z(dsi_grid_t* g, float* conf_host, uint8_t* idx_host)
{
    REQUIRE(g && conf_host && idx_host, DSI_ERR_INVALID, "null argument");
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    float* conf;
    uint8_t* idx;
    if (int rc = collapse_scratch(ctx, npix, &conf, &idx)) return rc;
    if (int rc = dsi_grid_collapse_max_z_dev(g, conf, idx, nullptr, nullptr)) return rc;
    return collapse_download(ctx, npix, conf, idx, conf_host, idx_host);
}

// ---- focus-based collapses and local focus (cartesian3dgrid.cpp:139-483) ----

static int check_focus_args(const dsi_grid_t* g, int method, int half_patchsize)
{
    REQUIRE(method >= DSI_FOCUS_LOCAL_VAR && method <= DSI_FOCUS_DOG, DSI_ERR_BAD_OP,
            "focus method %d is not one of 0..4 (LocalVar, LocalMeanSquare, GradMag, LaplacianMag, DoG)", method);
    REQUIRE(half_patchsize >= 0 && half_patchsize <= 8, DSI_ERR_INVALID, "half_patchsize must be in 0..8 (got %d)",
            half_patchsize);
    REQUIRE(g->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", g->nz);
    return DSI_OK;
}

// the focus collapse of g on ctx's stream, with ctx's key scratch
static int focus_collapse(dsi_context* ctx, const dsi_grid_t* g, int method, int half_patchsize, float* conf, uint8_t* idx,
                          const float* planes, float* depth)
{
    const size_t words = (size_t)dsi::focus_chunks(g->nx, g->ny, g->nz) * g->nx * g->ny;
    HIP_TRY(ctx->focus_keys.reserve(words));
    HIP_TRY(dsi::launch_focus_collapse(ctx->stream, g->data, g->nx, g->ny, g->nz, method, half_patchsize, ctx->focus_keys.p,
                                       conf, idx, planes, depth));
    return DSI_OK;
}

int dsi_grid_collapse_focus_dev(dsi_grid_t* g, int method, int half_patchsize, float* conf_dev, uint8_t* idx_dev,
                                const float* planes_dev, float* depth_dev)
{
    REQUIRE(g && conf_dev && idx_dev, DSI_ERR_INVALID, "null argument");
    if (int rc = check_focus_args(g, method, half_patchsize)) return rc;
    REQUIRE(!depth_dev || planes_dev, DSI_ERR_INVALID, "depth output needs the plane depths");
    if (int rc = set_device(g->ctx)) return rc;
    return focus_collapse(g->ctx, g, method, half_patchsize, conf_dev, idx_dev, planes_dev, depth_dev);
}

int dsi_grid_collapse_focus(dsi_grid_t* g, int method, int half_patchsize, float* conf_host, uint8_t* idx_host)
{
    REQUIRE(g && conf_host && idx_host, DSI_ERR_INVALID, "null argument");
    if (int rc = check_focus_args(g, method, half_patchsize)) return rc;
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    float* conf;
    uint8_t* idx;
    if (int rc = collapse_scratch(ctx, npix, &conf, &idx)) return rc;
    if (int rc = focus_collapse(ctx, g, method, half_patchsize, conf, idx, nullptr, nullptr)) return rc;
    return collapse_download(ctx, npix, conf, idx, conf_host, idx_host);
}

int dsi_grid_collapse_min_z(dsi_grid_t* g, float* val_host, uint8_t* idx_host)
{
    REQUIRE(g && val_host && idx_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(g->nz <= 256, DSI_ERR_INVALID, "arg-min indices are u8: dimZ must be <= 256 (got %d)", g->nz);
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    float* val;
    uint8_t* idx;
    if (int rc = collapse_scratch(ctx, npix, &val, &idx)) return rc;
    HIP_TRY(dsi::launch_collapse_min_z(ctx->stream, g->data, g->nx, g->ny, g->nz, val, idx));
    return collapse_download(ctx, npix, val, idx, val_host, idx_host);
}

static int release_to(dsi_context* owner, dsi_context* reader);

int dsi_grid_local_focus(dsi_grid_t* dst, const dsi_grid_t* src, int focus_method)
{
    if (int rc = check_pair(dst, src)) return rc;
    dsi_context* ctx = dst->ctx;
    if (dst != src) {  // src may live in another context of the device: read it after its stream's work, as the reference would
        if (int rc = dsi_context_wait_for(ctx, src->ctx)) return rc;
        HIP_TRY(dsi::launch_local_focus(ctx->stream, src->data, dst->data, dst->nx, dst->ny, dst->nz, focus_method));
        return release_to(src->ctx, ctx);
    }
    // in place: every tile reads its neighbours' planes, so the new volume goes to scratch first
    HIP_TRY(ctx->focus_volume.reserve(dst->n));
    HIP_TRY(dsi::launch_local_focus(ctx->stream, src->data, ctx->focus_volume.p, dst->nx, dst->ny, dst->nz, focus_method));
    HIP_TRY(hipMemcpyAsync(dst->data, ctx->focus_volume.p, dst->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return DSI_OK;
}

int dsi_grid_mean_square(dsi_grid_t* g, double* out)
{
    REQUIRE(g && out, DSI_ERR_INVALID, "null argument");
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipMemsetAsync(ctx->ms_accum.p, 0, sizeof(double), ctx->stream));
    HIP_TRY(dsi::launch_mean_square(ctx->stream, g->data, g->n, ctx->ms_accum.p));
    double sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, ctx->ms_accum.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out = sum / (double)g->n;  // cartesian3dgrid.cpp:173
    return DSI_OK;
}

// ---- volume filters: cartesian3dgrid_filter.cpp, gaussianiir3d.cpp ----

int dsi_grid_laplacian(dsi_grid_t* g)
{
    REQUIRE(g, DSI_ERR_INVALID, "grid is null");
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    // every voxel reads its neighbours: the result goes to scratch and is copied back (the grid keeps its storage)
    HIP_TRY(ctx->filter_a.reserve(g->n));
    HIP_TRY(dsi::launch_stencil3d(ctx->stream, g->data, ctx->filter_a.p, g->nx, g->ny, g->nz, false, 0.f));
    HIP_TRY(hipMemcpyAsync(g->data, ctx->filter_a.p, g->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return DSI_OK;
}

int dsi_grid_smooth_diffuse(dsi_grid_t* g, float sigma, int* steps_out)
{
    REQUIRE(g, DSI_ERR_INVALID, "grid is null");
    REQUIRE(std::isfinite(sigma) && sigma > 0.f, DSI_ERR_INVALID, "sigma = %g: the diffusion needs a finite sigma > 0", (double)sigma);
    // cartesian3dgrid_filter.cpp:24-27, in fp32
    const float dt_cfl = 1.f / 12.f;
    const float t_final = 0.5f * sigma * sigma;
    const float dt = std::min(0.5f * dt_cfl, 0.5f * t_final);
    REQUIRE(t_final > 0.f && dt > 0.f, DSI_ERR_INVALID, "sigma = %g: sigma * sigma underflows", (double)sigma);
    const float steps_f = std::ceil(t_final / dt);
    REQUIRE(steps_f <= 1.0e6f, DSI_ERR_INVALID, "sigma = %g asks for %g diffusion steps (at most 1e6)", (double)sigma, (double)steps_f);
    const int steps = (int)steps_f;
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(ctx->filter_a.reserve(g->n));
    float *from = g->data, *to = ctx->filter_a.p;
    for (int i = 0; i < steps; ++i) {
        HIP_TRY(dsi::launch_stencil3d(ctx->stream, from, to, g->nx, g->ny, g->nz, true, dt));
        std::swap(from, to);
    }
    if (from != g->data)  // an odd number of steps ended in the scratch volume
        HIP_TRY(hipMemcpyAsync(g->data, from, g->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    if (steps_out) *steps_out = steps;
    return DSI_OK;
}

namespace {

struct IirAxis {
    float nu, boundaryscale, postscale;
};

// gaussianiir3d.cpp:158-163
IirAxis iir_axis(float sigma, int numsteps)
{
    const float sigma2 = sigma * sigma;
    const double lambda = (double)sigma2 / (2.0 * numsteps);
    const double dnu = (1.0 + 2.0 * lambda - std::sqrt(1.0 + 4.0 * lambda)) / (2.0 * lambda);
    return IirAxis{(float)dnu, (float)(1.0 / (1.0 - dnu)), (float)std::pow(dnu / lambda, (double)numsteps)};
}

// the 3-sigma gaussianiir3d on nx * ny * nz floats of device memory, on the context's stream
int iir3d_run(dsi_context* ctx, float* vol, int nx, int ny, int nz, float sigma_x, float sigma_y, float sigma_z, int numsteps)
{
    const float sigma[3] = {sigma_x, sigma_y, sigma_z};
    IirAxis ax[3];
    float postscale = 1.f;
    for (int a = 0; a < 3; ++a) {
        ax[a] = iir_axis(sigma[a], numsteps);
        postscale *= ax[a].postscale;
    }
    for (int a = 0; a < 3; ++a)
        HIP_TRY(dsi::launch_iir_axis(ctx->stream, vol, nx, ny, nz, a, ax[a].nu, ax[a].boundaryscale, numsteps, a == 2, postscale));
    return DSI_OK;
}

}  // namespace

int dsi_grid_smooth_iir(dsi_grid_t* g, float sigma_x, float sigma_y, float sigma_z, int numsteps)
{
    REQUIRE(g, DSI_ERR_INVALID, "grid is null");
    REQUIRE(numsteps <= 16, DSI_ERR_INVALID, "numsteps = %d (at most 16)", numsteps);
    if (sigma_x <= 0 || sigma_y <= 0 || sigma_z <= 0 || numsteps <= 0) return DSI_OK;  // gaussianiir3d.cpp:153-154
    if (int rc = set_device(g->ctx)) return rc;
    return iir3d_run(g->ctx, g->data, g->nx, g->ny, g->nz, sigma_x, sigma_y, sigma_z, numsteps);
}

int dsi_grid_mean_std(dsi_grid_t* g, double* mean, double* stddev)
{
    REQUIRE(g && mean && stddev, DSI_ERR_INVALID, "null argument");
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(ctx->filter_words.reserve(dsi::volume_sum_words()));
    HIP_TRY(dsi::launch_volume_mean_std(ctx->stream, g->data, g->n, ctx->filter_words.p));
    double r[2];
    HIP_TRY(hipMemcpyAsync(r, ctx->filter_words.p, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *mean = r[0];
    *stddev = r[1];
    return DSI_OK;
}

int dsi_grid_moran_index(dsi_grid_t* g, float sigma, double* out)
{
    REQUIRE(g && out, DSI_ERR_INVALID, "null argument");
    REQUIRE(!std::isnan(sigma) && sigma < 1.0e3f, DSI_ERR_INVALID, "sigma = %g (a number below 1000)", (double)sigma);
    if (sigma < 0.2) sigma = 0.2;  // cartesian3dgrid_filter.cpp:115-119: a double comparison, an fp32 value
    double mean = 0, stddev = 0;
    if (int rc = dsi_grid_mean_std(g, &mean, &stddev)) return rc;
    REQUIRE(stddev > 0 && std::isfinite(stddev), DSI_ERR_INVALID, "the grid's deviation is %g: Moran's index is undefined", stddev);
    dsi_context* ctx = g->ctx;
    // the centre weight: a unit impulse in a k^3 volume through the same kernels (:138-146)
    const int half = (int)(2 * std::ceil(3.f * sigma));
    const int k = 2 * half + 1;
    const size_t nk = (size_t)k * k * k, centre = (size_t)half + (size_t)k * ((size_t)half + (size_t)k * half);
    HIP_TRY(ctx->filter_a.reserve(std::max(g->n, nk)));
    HIP_TRY(ctx->filter_b.reserve(g->n));
    static const float one = 1.f;  // outlives the asynchronous copy on every path
    float c = 0.f;
    HIP_TRY(hipMemsetAsync(ctx->filter_a.p, 0, nk * sizeof(float), ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->filter_a.p + centre, &one, sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = iir3d_run(ctx, ctx->filter_a.p, k, k, k, sigma, sigma, sigma, 3)) return rc;
    HIP_TRY(hipMemcpyAsync(&c, ctx->filter_a.p + centre, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // the standardized volume and its smoothed copy (:126-135)
    const float inv_stddev = (float)(1.0 / stddev);
    HIP_TRY(dsi::launch_volume_standardize(ctx->stream, g->data, g->n, mean, inv_stddev, ctx->filter_a.p, ctx->filter_b.p));
    if (int rc = iir3d_run(ctx, ctx->filter_b.p, g->nx, g->ny, g->nz, sigma, sigma, sigma, 3)) return rc;
    HIP_TRY(dsi::launch_volume_moran_numerator(ctx->stream, ctx->filter_a.p, ctx->filter_b.p, g->n, c, ctx->filter_words.p));
    double numer = 0;
    HIP_TRY(hipMemcpyAsync(&numer, ctx->filter_words.p + 2, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const float sum_weights = 1.f - c;
    const double denom = (double)sum_weights * ((double)g->n - 1.0);  // :194-195
    *out = numer / (denom + 1e-6);
    return DSI_OK;
}

// ---- the rest of Grid3D: binary ops, min/max, slices, slice images ----

int dsi_grid_binary_op(dsi_grid_t* dst, const dsi_grid_t* src, int op)
{
    if (int rc = check_pair(dst, src)) return rc;
    REQUIRE(op >= DSI_GRID_OP_SUBTRACT && op <= DSI_GRID_OP_CUBIC_MEAN, DSI_ERR_BAD_OP,
            "grid op %d is not one of 1..4 (subtract, ratio, quadratic mean, cubic mean)", op);
    // dst == src is op(a, a): every voxel is read (both operands) before it is written, by the same thread
    HIP_TRY(dsi::launch_grid_binary(dst->ctx->stream, dst->data, src->data, dst->n, op));
    return DSI_OK;
}

int dsi_grid_min_max(dsi_grid_t* g, float* min_val, float* max_val, uint64_t* min_pos, uint64_t* max_pos)
{
    REQUIRE(g && min_val && max_val, DSI_ERR_INVALID, "null argument");
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(ctx->grid_words.reserve(dsi::grid_min_max_words()));
    HIP_TRY(dsi::launch_grid_min_max(ctx->stream, g->data, g->n, ctx->grid_words.p, 0));
    unsigned long long r[3];
    HIP_TRY(hipMemcpyAsync(r, ctx->grid_words.p, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t lo = (uint32_t)r[0], hi = (uint32_t)(r[0] >> 32);  // (float min, float max) in the first word
    std::memcpy(min_val, &lo, 4);
    std::memcpy(max_val, &hi, 4);
    if (min_pos) *min_pos = r[1];
    if (max_pos) *max_pos = r[2];
    return DSI_OK;
}

static int check_slice_args(const dsi_grid_t* g, unsigned slice_idx, unsigned dim_idx)
{
    REQUIRE(dim_idx <= 2u, DSI_ERR_INVALID, "dimIdx should be 0, 1 or 2 (got %u)", dim_idx);
    const unsigned size = (unsigned)(dim_idx == 0 ? g->nx : (dim_idx == 1 ? g->ny : g->nz));
    REQUIRE(slice_idx < size, DSI_ERR_INVALID, "slice %u is outside dimension %u of size %u", slice_idx, dim_idx, size);
    return DSI_OK;
}

static size_t slice_elems(const dsi_grid_t* g, unsigned dim_idx)
{
    return dim_idx == 0 ? (size_t)g->ny * g->nz : (dim_idx == 1 ? (size_t)g->nx * g->nz : (size_t)g->nx * g->ny);
}

int dsi_grid_get_slice_dev(dsi_grid_t* g, unsigned slice_idx, unsigned dim_idx, float* slice_dev)
{
    REQUIRE(g && slice_dev, DSI_ERR_INVALID, "null argument");
    if (int rc = check_slice_args(g, slice_idx, dim_idx)) return rc;
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(dsi::launch_grid_get_slice(g->ctx->stream, g->data, g->nx, g->ny, g->nz, (int)slice_idx, (int)dim_idx, slice_dev));
    return DSI_OK;
}

int dsi_grid_get_slice(dsi_grid_t* g, unsigned slice_idx, unsigned dim_idx, float* slice_host)
{
    REQUIRE(g && slice_host, DSI_ERR_INVALID, "null argument");
    if (int rc = check_slice_args(g, slice_idx, dim_idx)) return rc;
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t bytes = slice_elems(g, dim_idx) * sizeof(float);
    HIP_TRY(ctx->grid_bytes.reserve(bytes));
    float* dev = reinterpret_cast<float*>(ctx->grid_bytes.p);
    if (int rc = dsi_grid_get_slice_dev(g, slice_idx, dim_idx, dev)) return rc;
    HIP_TRY(hipMemcpyAsync(slice_host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DSI_OK;
}

int dsi_grid_accumulate_z_slice(dsi_grid_t* g, unsigned iz, const float* img_host, int rows, int cols)
{
    REQUIRE(g && img_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(rows >= 0 && cols >= 0 && rows <= g->ny && cols <= g->nx, DSI_ERR_INVALID,
            "a %d x %d image does not fit the %d x %d plane", rows, cols, g->ny, g->nx);
    REQUIRE(iz < (unsigned)g->nz, DSI_ERR_INVALID, "slice %u is outside dimZ = %d", iz, g->nz);
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t bytes = (size_t)rows * cols * sizeof(float);
    if (bytes == 0) return DSI_OK;
    HIP_TRY(ctx->grid_bytes.reserve(bytes));
    float* dev = reinterpret_cast<float*>(ctx->grid_bytes.p);
    HIP_TRY(hipMemcpyAsync(dev, img_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(dsi::launch_grid_accumulate_z_slice(ctx->stream, g->data, g->nx, g->ny, (int)iz, dev, rows, cols));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the image and the scratch are free again on return
    return DSI_OK;
}

int dsi_grid_value_at(dsi_grid_t* g, uint64_t p, float* out)
{
    REQUIRE(g && out, DSI_ERR_INVALID, "null argument");
    REQUIRE(p < g->n, DSI_ERR_INVALID, "voxel %llu is outside the grid of %zu cells", (unsigned long long)p, g->n);
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(out, g->data + p, sizeof(float), hipMemcpyDeviceToHost, g->ctx->stream));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    return DSI_OK;
}

int dsi_grid_set_value_at(dsi_grid_t* g, uint64_t p, float v)
{
    REQUIRE(g, DSI_ERR_INVALID, "grid is null");
    REQUIRE(p < g->n, DSI_ERR_INVALID, "voxel %llu is outside the grid of %zu cells", (unsigned long long)p, g->n);
    if (int rc = set_device(g->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(g->data + p, &v, sizeof(float), hipMemcpyHostToDevice, g->ctx->stream));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    return DSI_OK;
}

int dsi_grid_accumulate_value_at(dsi_grid_t* g, uint64_t p, float v)
{
    float old = 0.f;
    if (int rc = dsi_grid_value_at(g, p, &old)) return rc;
    return dsi_grid_set_value_at(g, p, old + v);  // one fp32 addition, as data_array_.at(p) += fval
}

static size_t slices_words(const dsi_grid_t* g, unsigned dim_idx)
{
    const size_t n_slices = (size_t)(dim_idx == 0 ? g->nx : (dim_idx == 1 ? g->ny : g->nz));
    return dsi::grid_min_max_words() + 2 * n_slices;
}

int dsi_grid_slices_u8_dev(dsi_grid_t* g, unsigned dim_idx, int normalize_by_minmax, uint8_t* out_dev)
{
    REQUIRE(g && out_dev, DSI_ERR_INVALID, "null argument");
    REQUIRE(dim_idx <= 2u, DSI_ERR_INVALID, "dimIdx should be 0, 1 or 2 (got %u)", dim_idx);
    REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 3u) == 0, DSI_ERR_INVALID, "the device output must be 4-byte aligned");
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(ctx->grid_words.reserve(slices_words(g, dim_idx)));
    HIP_TRY(dsi::launch_grid_slices_u8(ctx->stream, g->data, g->nx, g->ny, g->nz, (int)dim_idx, normalize_by_minmax != 0,
                                       ctx->grid_words.p, out_dev));
    return DSI_OK;
}

int dsi_grid_slices_u8(dsi_grid_t* g, unsigned dim_idx, int normalize_by_minmax, uint8_t* out_host)
{
    REQUIRE(g && out_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(dim_idx <= 2u, DSI_ERR_INVALID, "dimIdx should be 0, 1 or 2 (got %u)", dim_idx);
    dsi_context* ctx = g->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(ctx->grid_bytes.reserve(g->n));
    if (int rc = dsi_grid_slices_u8_dev(g, dim_idx, normalize_by_minmax, ctx->grid_bytes.p)) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, ctx->grid_bytes.p, g->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DSI_OK;
}

/* --------------------------------------------------------------- MapperEMVS */
int dsi_mapper_create(dsi_context_t* ctx, const dsi_mapper_config_t* cfg, dsi_mapper_t** out)
{
    REQUIRE(ctx && cfg && out, DSI_ERR_INVALID, "null argument");
    *out = nullptr;
    REQUIRE(cfg->sensor_width > 0 && cfg->sensor_height > 0, DSI_ERR_INVALID, "sensor size must be positive");
    REQUIRE(cfg->sensor_width <= 65536 && cfg->sensor_height <= 65536, DSI_ERR_INVALID,
            "event coordinates are u16");
    // glog CHECKs of setupDSI (mapper_emvs_stereo.cpp:210-211) and PinholeCamera
    // (geometry_utils.hpp:36-41) become error codes
    REQUIRE(cfg->min_depth > 0.f, DSI_ERR_INVALID, "min_depth must be > 0");
    REQUIRE(cfg->max_depth > cfg->min_depth, DSI_ERR_INVALID, "max_depth must be > min_depth");
    REQUIRE(cfg->dim_z >= 1 && cfg->dim_z <= 256, DSI_ERR_INVALID, "dimZ must be in 1..256 (main.cpp:156)");
    REQUIRE(cfg->dim_x >= 0 && cfg->dim_y >= 0, DSI_ERR_INVALID, "dimX/dimY must be >= 0");
    REQUIRE(cfg->plane_begin >= 0 && cfg->plane_count >= 0 && cfg->plane_begin < cfg->dim_z &&
                cfg->plane_begin + cfg->plane_count <= cfg->dim_z,
            DSI_ERR_INVALID, "plane range must lie inside [0, dimZ)");
    REQUIRE(cfg->K[0] > 0.f && cfg->K[1] > 0.f && cfg->K[2] > 0.f && cfg->K[3] > 0.f, DSI_ERR_INVALID,
            "camera fx, fy, cx, cy must be > 0");
    if (int rc = set_device(ctx)) return rc;

    dsi_mapper* m = new (std::nothrow) dsi_mapper();
    REQUIRE(m, DSI_ERR_INVALID, "out of host memory");
    m->ctx = ctx;
    ++ctx->children;
    m->sensor_w = cfg->sensor_width;
    m->sensor_h = cfg->sensor_height;
    dsi::Geom& g = m->geom;
    g.nx = cfg->dim_x > 0 ? cfg->dim_x : cfg->sensor_width;   // :216
    g.ny = cfg->dim_y > 0 ? cfg->dim_y : cfg->sensor_height;  // :217
    g.nz = cfg->dim_z;
    g.kfx = cfg->K[0];
    g.kfy = cfg->K[1];
    g.kcx = cfg->K[2];
    g.kcy = cfg->K[3];
    const float f = virtual_focal(cfg->K[0], cfg->fov_deg, g.nx);
    g.vfx = f;  // :236-239: PinholeCamera(dimX, dimY, f, f, cam.cx(), cam.cy())
    g.vfy = f;
    g.vcx = cfg->K[2];
    g.vcy = cfg->K[3];
    make_planes(cfg->min_depth, cfg->max_depth, cfg->dim_z, cfg->inverse_depth != 0, &m->planes);
    g.z0 = m->planes[0];  // :111, :163 -- of the full depth vector, also for a plane shard
    m->planes_full = m->planes;
    m->plane_begin = cfg->plane_begin;
#ifdef DSI_TIMING_EXPERIMENTS
    if (const char* e = std::getenv("DSI_PREP_OVERLAP")) m->prep_overlap = std::atoi(e) != 0;
#endif
    g.nz = cfg->plane_count > 0 ? cfg->plane_count : cfg->dim_z - cfg->plane_begin;
    m->planes = std::vector<float>(m->planes.begin() + m->plane_begin, m->planes.begin() + m->plane_begin + g.nz);

    int rc = DSI_OK;
    hipError_t e = m->planes_dev.reserve(g.nz);
    if (e == hipSuccess)
        e = hipMemcpy(m->planes_dev.p, m->planes.data(), g.nz * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && cfg->lut) {
        const size_t n = (size_t)cfg->sensor_width * cfg->sensor_height;
        e = m->lut_dev.reserve(n);
        if (e == hipSuccess) e = hipMemcpy(m->lut_dev.p, cfg->lut, n * sizeof(float2), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) rc = fail(DSI_ERR_HIP, "mapper setup failed: %s", hipGetErrorString(e));
    if (rc == DSI_OK) rc = dsi_grid_create(ctx, g.nx, g.ny, g.nz, &m->grid);  // :240
    if (rc != DSI_OK) {  // (the grid, the last step, does not exist)
        --ctx->children;
        delete m;
        return rc;
    }
    *out = m;
    return DSI_OK;
}

int dsi_mapper_destroy(dsi_mapper_t* m)
{
    if (!m) return DSI_OK;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    if (m->prep_stream) (void)hipStreamSynchronize(m->prep_stream);
    if (m->ev_depth_ready && m->ctx->copy_stream) (void)hipStreamSynchronize(m->ctx->copy_stream);
    if (m->grid) dsi_grid_destroy(m->grid);
    --m->ctx->children;
    delete m;
    return DSI_OK;
}

dsi_grid_t* dsi_mapper_grid(dsi_mapper_t* m) { return m ? m->grid : nullptr; }

int dsi_mapper_plane_begin(const dsi_mapper_t* m) { return m ? m->plane_begin : 0; }

int dsi_mapper_full_depths(const dsi_mapper_t* m, float* raw_depths, int* dim_z)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    if (raw_depths) std::memcpy(raw_depths, m->planes_full.data(), m->planes_full.size() * sizeof(float));
    if (dim_z) *dim_z = (int)m->planes_full.size();
    return DSI_OK;
}

int dsi_mapper_geometry(const dsi_mapper_t* m, float* Kv, float* raw_depths, int* nx, int* ny, int* nz)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    if (Kv) {
        Kv[0] = m->geom.vfx;
        Kv[1] = m->geom.vfy;
        Kv[2] = m->geom.vcx;
        Kv[3] = m->geom.vcy;
    }
    if (raw_depths) std::memcpy(raw_depths, m->planes.data(), m->planes.size() * sizeof(float));
    if (nx) *nx = m->geom.nx;
    if (ny) *ny = m->geom.ny;
    if (nz) *nz = m->geom.nz;
    return DSI_OK;
}

int dsi_mapper_set_vote_algo(dsi_mapper_t* m, int algo)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(algo >= DSI_VOTE_AUTO && algo <= DSI_VOTE_LDS_BANDS, DSI_ERR_INVALID, "unknown vote algorithm %d",
            algo);
    m->algo = algo;
    return DSI_OK;
}

int dsi_mapper_set_band_params(dsi_mapper_t* m, int band_rows, int chunks, int block_threads)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(band_rows >= 0 && chunks >= 0, DSI_ERR_INVALID, "band_rows and chunks must be >= 0");
    REQUIRE(block_threads == 0 || block_threads == 256 || block_threads == 512 || block_threads == 1024,
            DSI_ERR_INVALID, "block_threads must be 0, 256, 512 or 1024");
    m->want_band_rows = band_rows;
    m->want_chunks = chunks;
    m->want_block = block_threads;
    return DSI_OK;
}

int dsi_mapper_set_packed_lanes(dsi_mapper_t* m, int mode)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(mode >= -1 && mode <= 8, DSI_ERR_INVALID, "mode must be -1 (auto) or 0..8");
    m->want_packed = mode;
    return DSI_OK;
}

int dsi_mapper_paired_overflow(dsi_mapper_t* m, int* overflowed)
{
    REQUIRE(m && overflowed, DSI_ERR_INVALID, "null argument");
    *overflowed = 0;
    if (m->info.algo != DSI_VOTE_LDS_BANDS || m->info.packed != 8 || m->info.n_packets == 0) return DSI_OK;
    if (int rc = set_device(m->ctx)) return rc;
    uint32_t word = 0;
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    HIP_TRY(hipMemcpy(&word, m->nvalid.p + m->info.n_packets + (size_t)m->geom.nz + 8, sizeof word, hipMemcpyDeviceToHost));
    *overflowed = word != 0u ? 1 : 0;
    return DSI_OK;
}

int dsi_mapper_set_inline_cuts(dsi_mapper_t* m, long long min_packets)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    m->cuts_inline_min_packets = min_packets < 0 ? (size_t)8192 : (size_t)min_packets;
    return DSI_OK;
}

int dsi_mapper_fill_voxel_grid(dsi_mapper_t* m, const float* xy_z0, const float* centers, size_t n_packets)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(n_packets == 0 || (xy_z0 && centers), DSI_ERR_INVALID, "null input");
    REQUIRE(n_packets < ((size_t)1 << 21), DSI_ERR_INVALID, "too many packets in one call");
    dsi_context* ctx = m->ctx;
    if (int rc = set_device(ctx)) return rc;
    if (n_packets == 0) return DSI_OK;
    HIP_TRY(m->xy.reserve(n_packets * dsi::kPacket));
    HIP_TRY(m->centers.reserve(n_packets * 3));
    if (int rc = upload_async(ctx, m->xy.p, xy_z0, n_packets * dsi::kPacket * sizeof(float2))) return rc;
    if (int rc = upload_async(ctx, m->centers.p, centers, n_packets * 3 * sizeof(float))) return rc;
    // (host inputs were uploaded on the context's stream: no second stream here)
    int rc = vote_device(m, m->xy.p, m->centers.p, n_packets, /*accumulate=*/true, ctx->stream);
    // the host buffers are pageable: do not return before the copies have read them
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rc;
}

static int batch_create(dsi_context_t* ctx, const uint16_t* x, const uint16_t* y, size_t n_events,
                        const uint32_t* packet_first, const float* Rt, size_t n_packets, dsi_batch_t** out,
                        bool wait)
{
    REQUIRE(ctx && out, DSI_ERR_INVALID, "null argument");
    *out = nullptr;
    REQUIRE(n_events == 0 || (x && y), DSI_ERR_INVALID, "null event arrays");
    REQUIRE(n_packets == 0 || Rt, DSI_ERR_INVALID, "null pose array");
    REQUIRE(n_events < ((size_t)1 << 32), DSI_ERR_INVALID, "at most 2^32-1 events per batch");
    REQUIRE(n_packets < ((size_t)1 << 21), DSI_ERR_INVALID, "too many packets in one batch");
    bool regular = true;  // packet k starts at event k * 1024 (no pose look-up failed, mapper_emvs_stereo.cpp:95-99)
    for (size_t k = 0; k < n_packets; ++k) {
        const size_t first = packet_first ? packet_first[k] : k * dsi::kPacket;
        REQUIRE(first + dsi::kPacket <= n_events, DSI_ERR_INVALID,
                "packet %zu [%zu, %zu) exceeds the %zu events given", k, first, first + dsi::kPacket, n_events);
        regular = regular && first == k * dsi::kPacket;
    }
    // ... then the table is implied and does not travel: the runtime moves a copy of a few KB with a shader, which waits for
    // a free CU behind a persistent voting kernel and held up a window's other uploads by 0.2 ms (profiles/r05_cpp_window_stream_timeline.txt)
    if (regular) packet_first = nullptr;
    if (int rc = set_device(ctx)) return rc;
    dsi_batch* b = new (std::nothrow) dsi_batch();
    REQUIRE(b, DSI_ERR_INVALID, "out of host memory");
    b->ctx = ctx;
    ++ctx->children;
    b->n_events = n_events;
    b->n_packets = n_packets;
    // one block: Rt | first | x | y (256-byte aligned parts), uploaded on the context's stream
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t rt_bytes = up(std::max<size_t>(n_packets, 1) * 12 * sizeof(float));
    const size_t first_bytes = packet_first ? up(std::max<size_t>(n_packets, 1) * sizeof(uint32_t)) : 0;
    const size_t ev_bytes = up(std::max<size_t>(n_events, 1) * sizeof(uint16_t));
    if (!pool_take(ctx, rt_bytes + first_bytes + 2 * ev_bytes, &b->block)) {
        --ctx->children;
        delete b;
        return fail(DSI_ERR_HIP, "batch allocation of %zu bytes failed", rt_bytes + first_bytes + 2 * ev_bytes);
    }
    char* base = static_cast<char*>(b->block.p);
    b->Rt = reinterpret_cast<float*>(base);
    b->first = packet_first ? reinterpret_cast<uint32_t*>(base + rt_bytes) : nullptr;
    b->x = reinterpret_cast<uint16_t*>(base + rt_bytes + first_bytes);
    b->y = reinterpret_cast<uint16_t*>(base + rt_bytes + first_bytes + ev_bytes);
    hipStream_t cs = ctx->upload_stream;
    hipError_t e = b->ready.create(hipEventDisableTiming);
    // the block's previous reader (a kernel on the compute stream) must be done before we overwrite it
    if (e == hipSuccess) e = hipStreamWaitEvent(cs, b->block.freed, 0);
    if (e == hipSuccess && n_events) e = hipMemcpyAsync(b->x, x, n_events * sizeof(uint16_t), hipMemcpyHostToDevice, cs);
    if (e == hipSuccess && n_events)
        e = hipMemcpyAsync(b->y, y, n_events * sizeof(uint16_t), hipMemcpyHostToDevice, cs);
    if (e == hipSuccess && n_packets)
        e = hipMemcpyAsync(b->Rt, Rt, n_packets * 12 * sizeof(float), hipMemcpyHostToDevice, cs);
    if (e == hipSuccess && n_packets && packet_first)
        e = hipMemcpyAsync(b->first, packet_first, n_packets * sizeof(uint32_t), hipMemcpyHostToDevice, cs);
    if (e == hipSuccess) e = hipEventRecord(b->ready, cs);
    // the host arrays are the caller's: they must be consumed before this call returns (this waits
    // for the copies only, not for whatever the compute stream is doing) -- unless the caller
    // vouches for them (dsi_batch_create_async: page-locked memory, left alone until uploaded)
    if (e == hipSuccess && wait) e = hipStreamSynchronize(cs);
    if (e != hipSuccess) {
        dsi_batch_destroy(b);  // (not a plain delete: the block goes back to the pool)
        return fail(DSI_ERR_HIP, "batch upload failed: %s", hipGetErrorString(e));
    }
    *out = b;
    return DSI_OK;
}

int dsi_batch_create(dsi_context_t* ctx, const uint16_t* x, const uint16_t* y, size_t n_events,
                     const uint32_t* packet_first, const float* Rt, size_t n_packets, dsi_batch_t** out)
{
    return batch_create(ctx, x, y, n_events, packet_first, Rt, n_packets, out, /*wait=*/true);
}

int dsi_batch_create_async(dsi_context_t* ctx, const uint16_t* x, const uint16_t* y, size_t n_events,
                           const uint32_t* packet_first, const float* Rt, size_t n_packets, dsi_batch_t** out)
{
    return batch_create(ctx, x, y, n_events, packet_first, Rt, n_packets, out, /*wait=*/false);
}

int dsi_batch_uploaded(const dsi_batch_t* b)
{
    if (!b || !b->ready) return 1;
    // (anything but "not ready" ends a caller's polling loop: a failed copy surfaces at the next synchronisation)
    return hipEventQuery(b->ready) == hipErrorNotReady ? 0 : 1;
}

int dsi_host_alloc(size_t bytes, void** out)
{
    REQUIRE(out, DSI_ERR_INVALID, "out is null");
    *out = nullptr;
    REQUIRE(bytes > 0, DSI_ERR_INVALID, "bytes must be > 0");
    // coherent + mapped whatever HIP_HOST_COHERENT says: kernels store depth maps into these blocks
    // (dsi_mapper_fetch_depth_map_in_order) and the host reads them after an event
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    return DSI_OK;
}

int dsi_host_free(void* p)
{
    if (!p) return DSI_OK;
    HIP_TRY(hipHostFree(p));
    return DSI_OK;
}

int dsi_batch_destroy(dsi_batch_t* b)
{
    if (!b) return DSI_OK;
    (void)hipSetDevice(b->ctx->device);
    // an upload that nobody waited for yet (async batch destroyed unused): order the block's reuse after it
    if (b->ready) (void)hipStreamWaitEvent(b->ctx->stream, b->ready, 0);
    pool_give(b->ctx, b->block);  // no wait: the block's "freed" event orders its reuse
    --b->ctx->children;
    delete b;
    return DSI_OK;
}

size_t dsi_batch_num_packets(const dsi_batch_t* b) { return b ? b->n_packets : 0; }

int dsi_mapper_evaluate_batch(dsi_mapper_t* m, const dsi_batch_t* batch)
{
    REQUIRE(m && batch, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx == batch->ctx, DSI_ERR_CONTEXT, "mapper and batch belong to different contexts");
    dsi_context* ctx = m->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t np = batch->n_packets;
    hipStream_t ps = ctx->stream;
    if (np) {
        HIP_TRY(m->centers.reserve(np * 3));
        if (int rc = prep_begin(m, &ps)) return rc;
        if (batch->ready) HIP_TRY(hipStreamWaitEvent(ps, batch->ready, 0));  // uploaded on the copy stream
    }
    // stage A (:108-142) happens inside vote_device (fused into the packet sort on the default path);
    // resetGrid (:145) is folded into the vote: accumulate = false
    return vote_device(m, m->xy.p, m->centers.p, np, /*accumulate=*/false, ps, batch);
}

int dsi_pose_at(const double* traj_times, const double* traj_poses, size_t n_poses, double t, double* out)
{
    REQUIRE(traj_times && traj_poses && out, DSI_ERR_INVALID, "null argument");
    dsi::host::Pose T;
    if (!dsi::host::pose_at(traj_times, traj_poses, n_poses, t, &T))
        return fail(DSI_ERR_INVALID, "cannot extrapolate the trajectory to t=%.9f", t);
    T.to7(out);
    return DSI_OK;
}

int dsi_packetize(const double* ts, size_t n_events, const double* traj_times, const double* traj_poses,
                  size_t n_poses, const double* T_rv_w, uint32_t* packet_first, float* Rt, size_t* n_packets)
{
    REQUIRE(n_packets && T_rv_w && traj_times && traj_poses, DSI_ERR_INVALID, "null argument");
    REQUIRE(n_events == 0 || ts, DSI_ERR_INVALID, "null timestamps");
    REQUIRE(n_events < ((size_t)1 << 32), DSI_ERR_INVALID, "at most 2^32-1 events");
    *n_packets = 0;
    std::vector<uint32_t> first;
    std::vector<float> rt;
    if (!dsi::host::packetize(ts, n_events, traj_times, traj_poses, n_poses, dsi::host::Pose::from7(T_rv_w),
                              &first, &rt))
        return fail(DSI_ERR_TOO_FEW_EVENTS, "number of events (%zu) < packet size (%d)", n_events,
                    DSI_PACKET_SIZE);
    *n_packets = first.size();
    if (packet_first && !first.empty()) std::memcpy(packet_first, first.data(), first.size() * sizeof(uint32_t));
    if (Rt && !rt.empty()) std::memcpy(Rt, rt.data(), rt.size() * sizeof(float));
    return DSI_OK;
}

int dsi_packetize_strided(const void* ts_first, size_t stride_bytes, size_t n_events, const double* traj_times,
                          const double* traj_poses, size_t n_poses, const double* T_rv_w, uint32_t* packet_first, float* Rt,
                          size_t* n_packets)
{
    REQUIRE(n_packets && T_rv_w && traj_times && traj_poses, DSI_ERR_INVALID, "null argument");
    REQUIRE(n_events == 0 || ts_first, DSI_ERR_INVALID, "null timestamps");
    REQUIRE(stride_bytes >= sizeof(double), DSI_ERR_INVALID, "stride of %zu bytes is smaller than a timestamp", stride_bytes);
    REQUIRE(n_events < ((size_t)1 << 32), DSI_ERR_INVALID, "at most 2^32-1 events");
    *n_packets = 0;
    std::vector<uint32_t> first;
    std::vector<float> rt;
    const char* base = static_cast<const char*>(ts_first);
    auto ts_of = [base, stride_bytes](size_t i) {
        double t;
        std::memcpy(&t, base + i * stride_bytes, sizeof t);  // (no alignment assumed)
        return t;
    };
    if (!dsi::host::packetize_with(ts_of, n_events, traj_times, traj_poses, n_poses, dsi::host::Pose::from7(T_rv_w), &first, &rt))
        return fail(DSI_ERR_TOO_FEW_EVENTS, "number of events (%zu) < packet size (%d)", n_events, DSI_PACKET_SIZE);
    *n_packets = first.size();
    if (packet_first && !first.empty()) std::memcpy(packet_first, first.data(), first.size() * sizeof(uint32_t));
    if (Rt && !rt.empty()) std::memcpy(Rt, rt.data(), rt.size() * sizeof(float));
    return DSI_OK;
}

int dsi_mapper_evaluate(dsi_mapper_t* m, const uint16_t* x, const uint16_t* y, const double* ts,
                        size_t n_events, const double* traj_times, const double* traj_poses, size_t n_poses,
                        const double* T_rv_w, size_t* n_voted)
{
    REQUIRE(m && traj_times && traj_poses && T_rv_w, DSI_ERR_INVALID, "null argument");
    REQUIRE(n_events == 0 || (x && y && ts), DSI_ERR_INVALID, "null event arrays");
    REQUIRE(n_events < ((size_t)1 << 32), DSI_ERR_INVALID, "at most 2^32-1 events");
    if (n_voted) *n_voted = 0;
    std::vector<uint32_t> first;
    std::vector<float> rt;
    if (!dsi::host::packetize(ts, n_events, traj_times, traj_poses, n_poses, dsi::host::Pose::from7(T_rv_w),
                              &first, &rt))
        return fail(DSI_ERR_TOO_FEW_EVENTS, "number of events (%zu) < packet size (%d)", n_events,
                    DSI_PACKET_SIZE);
    dsi_batch_t* b = nullptr;
    int rc = dsi_batch_create(m->ctx, x, y, n_events, first.data(), rt.data(), first.size(), &b);
    if (rc != DSI_OK) return rc;
    rc = dsi_mapper_evaluate_batch(m, b);
    std::string keep = g_last_error;
    dsi_batch_destroy(b);  // synchronises the stream
    g_last_error = keep;
    if (rc == DSI_OK && n_voted) *n_voted = first.size() * (size_t)DSI_PACKET_SIZE;
    return rc;
}

// A kernel on `reader`'s stream has just been queued that READS a grid of context `owner`: whatever `owner`
// queues from now on (the next vote or fusion overwriting that grid) must start after it (the
// one-way wait_for before the arg-max left a write-after-read hazard for grids of another context).  Device-
// side ordering only; nothing to do within one context (one in-order stream).
static int release_to(dsi_context* owner, dsi_context* reader)
{
    if (owner == reader) return DSI_OK;
    return dsi_context_wait_for(owner, reader);
}

int dsi_mapper_depth_map_of(dsi_mapper_t* m, dsi_grid_t* g)
{
    REQUIRE(m && g, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx->device == g->ctx->device, DSI_ERR_CONTEXT, "mapper and grid live on different devices");
    REQUIRE(same_shape(m->grid, g), DSI_ERR_SHAPE, "grid shape differs from the mapper's DSI");
    if (int rc = set_device(m->ctx)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    HIP_TRY(m->conf.reserve(npix));
    HIP_TRY(m->depth.reserve(npix));
    HIP_TRY(m->idx.reserve(npix));
    // The arg-max writes the MAPPER's buffers and the filters / copies that follow run on the mapper's
    // stream, so the kernel goes to the mapper's stream; a grid that lives in another context (stream)
    // of the same device is first waited for: everything queued on its stream so far.
    REQUIRE(g->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", g->nz);
    if (int rc = dsi_context_wait_for(m->ctx, g->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    HIP_TRY(dsi::launch_collapse_max_z(m->ctx->stream, g->data, g->nx, g->ny, g->nz, m->conf.p, m->idx.p,
                                       m->planes_dev.p, m->depth.p));
    if (int rc = release_to(g->ctx, m->ctx)) return rc;
    return depth_buffers_ready(m);
}

int dsi_mapper_depth_map_of_focus(dsi_mapper_t* m, dsi_grid_t* g, int method)
{
    if (method < DSI_FOCUS_LOCAL_VAR || method > DSI_FOCUS_DOG) return dsi_mapper_depth_map_of(m, g);  // :366-367
    REQUIRE(m && g, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx->device == g->ctx->device, DSI_ERR_CONTEXT, "mapper and grid live on different devices");
    REQUIRE(same_shape(m->grid, g), DSI_ERR_SHAPE, "grid shape differs from the mapper's DSI");
    if (int rc = check_focus_args(g, method, 1)) return rc;  // collapseZSliceByGradMag's default half_patchsize
    if (int rc = set_device(m->ctx)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    HIP_TRY(m->conf.reserve(npix));
    HIP_TRY(m->depth.reserve(npix));
    HIP_TRY(m->idx.reserve(npix));
    if (int rc = dsi_context_wait_for(m->ctx, g->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    if (int rc = focus_collapse(m->ctx, g, method, 1, m->conf.p, m->idx.p, m->planes_dev.p, m->depth.p)) return rc;
    if (int rc = release_to(g->ctx, m->ctx)) return rc;
    return depth_buffers_ready(m);
}

int dsi_mapper_depth_map_of_fusion(dsi_mapper_t* m, const dsi_grid_t* a, const dsi_grid_t* b, int op)
{
    REQUIRE(m && a && b, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx->device == a->ctx->device && m->ctx->device == b->ctx->device, DSI_ERR_CONTEXT,
            "mapper and grids live on different devices");
    REQUIRE(same_shape(m->grid, a) && same_shape(m->grid, b), DSI_ERR_SHAPE, "grid shape differs from the mapper's DSI");
    REQUIRE(op >= 1 && op <= 6, DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    REQUIRE(a->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", a->nz);
    if (int rc = set_device(m->ctx)) return rc;
    const size_t npix = (size_t)a->nx * a->ny;
    HIP_TRY(m->conf.reserve(npix));
    HIP_TRY(m->depth.reserve(npix));
    HIP_TRY(m->idx.reserve(npix));
    if (int rc = dsi_context_wait_for(m->ctx, a->ctx)) return rc;
    if (int rc = dsi_context_wait_for(m->ctx, b->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    HIP_TRY(dsi::launch_collapse_max_z_fused(m->ctx->stream, a->data, b->data, a->nx, a->ny, a->nz, op, m->conf.p,
                                             m->idx.p, m->planes_dev.p, m->depth.p));
    if (int rc = release_to(a->ctx, m->ctx)) return rc;
    if (int rc = release_to(b->ctx, m->ctx)) return rc;
    return depth_buffers_ready(m);
}

int dsi_mapper_depth_map_of_fusion_n(dsi_mapper_t* m, const dsi_grid_t* const* srcs, int n, int mode)
{
    REQUIRE(m && srcs, DSI_ERR_INVALID, "null argument");
    REQUIRE(valid_fuse_n_mode(mode, n), DSI_ERR_BAD_OP, "bad fusion mode %d for %d grids (DSI_ACC_GM_TREE needs 2, 4 or 8)", mode, n);
    REQUIRE(n >= 1 && n <= 8, DSI_ERR_INVALID, "1 <= n <= 8 sources (got %d)", n);
    const float* ptrs[8];
    for (int i = 0; i < n; ++i) {
        REQUIRE(srcs[i], DSI_ERR_INVALID, "source %d is null", i);
        REQUIRE(m->ctx->device == srcs[i]->ctx->device, DSI_ERR_CONTEXT, "mapper and grids live on different devices");
        REQUIRE(same_shape(m->grid, srcs[i]), DSI_ERR_SHAPE, "grid shape differs from the mapper's DSI");
        ptrs[i] = srcs[i]->data;
    }
    REQUIRE(m->grid->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", m->grid->nz);
    if (int rc = set_device(m->ctx)) return rc;
    const size_t npix = (size_t)m->grid->nx * m->grid->ny;
    HIP_TRY(m->conf.reserve(npix));
    HIP_TRY(m->depth.reserve(npix));
    HIP_TRY(m->idx.reserve(npix));
    for (int i = 0; i < n; ++i)
        if (int rc = dsi_context_wait_for(m->ctx, srcs[i]->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    HIP_TRY(dsi::launch_collapse_max_z_fused_n(m->ctx->stream, ptrs, n, mode, m->grid->nx, m->grid->ny, m->grid->nz,
                                               m->conf.p, m->idx.p, m->planes_dev.p, m->depth.p));
    for (int i = 0; i < n; ++i)
        if (int rc = release_to(srcs[i]->ctx, m->ctx)) return rc;
    return depth_buffers_ready(m);
}

static int depth_map_of_events_impl(dsi_mapper_t* out, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches, int n,
                                    int op, bool gm_tree4);

int dsi_mapper_depth_map_of_events(dsi_mapper_t* out, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches, int n,
                                   int op)
{
    REQUIRE(out && mappers && batches, DSI_ERR_INVALID, "null argument");
    REQUIRE(n >= 1 && n <= 3, DSI_ERR_INVALID, "1, 2 or 3 cameras (got %d)", n);
    REQUIRE(n == 1 || (op >= 1 && op <= 6), DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    return depth_map_of_events_impl(out, mappers, batches, n, op, false);
}

int dsi_mapper_depth_map_of_events_n(dsi_mapper_t* out, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches, int n,
                                     int mode)
{
    REQUIRE(out && mappers && batches, DSI_ERR_INVALID, "null argument");
    REQUIRE(mode == DSI_ACC_GM_TREE, DSI_ERR_BAD_OP, "the DSI-less n-camera path fuses by the geometric-mean tree (DSI_ACC_GM_TREE); got mode %d", mode);
    REQUIRE(n == 2 || n == 4, DSI_ERR_INVALID, "the geometric-mean tree takes 2 or 4 cameras here (got %d)", n);
    // (two cameras: the tree IS the reference's 2-ary op, cartesian3dgrid.h:150-156)
    return depth_map_of_events_impl(out, mappers, batches, n, DSI_FUSE_GM, n == 4);
}

static int depth_map_of_events_impl(dsi_mapper_t* out, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches, int n,
                                    int op, bool gm_tree4)
{
    dsi_context* ctx = out->ctx;
    size_t np_max = 0;
    for (int i = 0; i < n; ++i) {
        REQUIRE(mappers[i] && batches[i], DSI_ERR_INVALID, "camera %d: null mapper or batch", i);
        REQUIRE(mappers[i]->ctx == ctx && batches[i]->ctx == ctx, DSI_ERR_CONTEXT,
                "mappers, batches and the output mapper must share one context");
        REQUIRE(same_shape(out->grid, mappers[i]->grid), DSI_ERR_SHAPE, "camera %d: DSI shape differs from the output mapper's", i);
        for (int k = 0; k < i; ++k)
            REQUIRE(mappers[i] != mappers[k], DSI_ERR_INVALID, "the cameras need distinct mappers (their tables are per mapper)");
    }
    // process1.cpp:169-191: the third camera enters only through min (1), harmonicMeanTwoGrids(g, 3) (2) and max (6);
    // "case 3: break; case 4: break; case 5: break;" -- its DSI is built and then ignored, so it is not built here
    if (n == 3 && !gm_tree4 && (op == 3 || op == 4 || op == 5)) n = 2;
    for (int i = 0; i < n; ++i) np_max = std::max(np_max, batches[i]->n_packets);
    REQUIRE(out->geom.nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", out->geom.nz);
    if (int rc = set_device(ctx)) return rc;
    dsi::BandPlan bp{};
    // every knob of this path (lane mapping, band height, the kernel timer, the experiments flavour's pass size, partition
    // cost and tracing) is read from ONE object, the output mapper; the vote info is recorded on it and on the cameras
    REQUIRE(plan_fused(out, np_max, &bp, n), DSI_ERR_INVALID, "grid rows of %d floats do not fit the fused kernel", out->geom.nx);
    if (bp.interleave < 0) {
        // Which pairs a workgroup takes: a contiguous piece of its XCD's stretch (0), or -- all 32 workgroups of an XCD on
        // consecutive planes of ONE band -- every 32nd pair (1) / the next pair drawn from the XCD's counter (2).  With
        // contiguous pieces an XCD works on bands / 8 + 1 bands at once; when their records (all cameras') exceed its 4 MB of
        // L2 every phase re-reads its band from the Infinity Cache -- four cameras x 2 M events at 1024 x 1024 x 256: 13 MB,
        // 4.6 TB/s; in turn: 6.10 -> 5.76 ms per step (kernel 5.89 -> 5.55), drawn: 5.50 (a workgroup's 74 pairs differ in
        // cost; the draw is one atomic per pair).  A 50 ms stereo window (2.5 MB) measures the same all three ways -- its
        // kernel lasts ceil(2800 pairs / 256 workgroups) = 11 pairs of equal cost however they are dealt -- and keeps the
        // contiguous pieces (one band change per workgroup).
        double records_bytes = 0.0;
        for (int i = 0; i < n; ++i) records_bytes += (double)batches[i]->n_packets * dsi::kPacket * sizeof(dsi::EvRec);
        const double band_bytes = records_bytes * (double)(bp.band_rows + 2) / (double)std::max(1, out->geom.ny);
        const int at_once = std::min(32, bp.bands / 8 + 1);
        bp.interleave = band_bytes * at_once > 3.0e6 ? 2 : 0;
    }
#ifdef DSI_TIMING_EXPERIMENTS
    if (out->fused_solo >= 0) {  // test hook dsi_test_fused_solo: the dealt mode, one workgroup (k_vote_fuse_argmax's body)
        bp.interleave = 2;
        bp.experiment = 310 + out->fused_solo;
    }
#endif
    const dsi::Geom& geom = mappers[0]->geom;
    hipStream_t st = ctx->stream;
    dsi::FusedCameras cams{};
    cams.n = n;
    dsi::PrepCameraArgs prep[dsi::kFusedMaxCameras] = {};
    const int n_pairs = bp.bands * geom.nz;
#ifdef DSI_TIMING_EXPERIMENTS
    const bool balance = n <= 2 && n_pairs <= dsi::fused_max_pairs() && out->fused_fixed_cost >= 0 && out->fused_solo < 0;
    // (dsi_test_fused_grid_blocks may have changed the workgroup count since dsi_test_fused_trace_enable sized the trace)
    REQUIRE(!out->fused_trace_on || out->fused_trace.cap >= dsi::fused_trace_words(), DSI_ERR_INVALID,
            "the trace buffer was sized for another workgroup count: enable tracing again");
#else
    const bool balance = n <= 2 && n_pairs <= dsi::fused_max_pairs() && out->fused_fixed_cost >= 0;
#endif
    for (int i = 0; i < n; ++i) {
        dsi_mapper* m = mappers[i];
        const dsi_batch* b = batches[i];
        const size_t np = b->n_packets;
        // the per-camera tables of the banded vote, built for bands with halo rows
        HIP_TRY(m->centers.reserve(std::max<size_t>(np, 1) * 3));
        HIP_TRY(m->sxy.reserve(np * dsi::kPacket + 1));
        HIP_TRY(m->nvalid.reserve(np + (size_t)geom.nz + 9));
        HIP_TRY(m->rowstart.reserve(np * (size_t)(geom.ny + 2 * bp.row_pad + 3) + 2));
        HIP_TRY(m->coef.reserve(np * geom.nz + 1));
        HIP_TRY(m->cuts.reserve(std::max<size_t>(np * geom.nz * bp.bands, 64)));
        HIP_TRY(m->pair_work.reserve((size_t)n_pairs));
        if (b->ready) HIP_TRY(hipStreamWaitEvent(st, b->ready, 0));  // uploaded on the copy stream
        if (np == 0) {
            // evaluateDSI returns false (mapper_emvs_stereo.cpp:71-75): this camera's DSI is all zero
            HIP_TRY(hipMemsetAsync(m->nvalid.p, 0, ((size_t)geom.nz + 8) * sizeof(uint32_t), st));
            HIP_TRY(hipMemsetAsync(m->pair_work.p, 0, (size_t)n_pairs * sizeof(uint32_t), st));
        }
        prep[i] = dsi::PrepCameraArgs{b->Rt, b->x, b->y, b->first, m->lut_dev.p, m->sensor_w, m->sensor_h, m->centers.p, (int)np,
                                      m->sxy.p, m->nvalid.p, m->rowstart.p, m->planes_dev.p, m->coef.p, m->cuts.p,
                                      balance ? m->pair_work.p : nullptr, m->geom};
        cams.cam[i] = dsi::FusedCamera{m->sxy.p, m->coef.p, m->cuts.p, m->nvalid.p + np, (int)np};
        m->info = dsi_vote_info_t{};
        m->info.algo = DSI_VOTE_FUSED_ARGMAX;
        m->info.n_packets = np;
        m->info.bands = bp.bands;
        m->info.band_rows = bp.band_rows;
        m->info.chunks = 1;
        m->info.block_threads = bp.block_threads;
        m->info.lds_bytes = bp.lds_bytes;
        m->info.packed = bp.packed;
        m->info.group_packets = 1;
    }
    out->info = mappers[0]->info;
    out->info.n_packets = np_max;
    // stage A + packet sort of all cameras in one launch, their coefficient / cut tables in another
    // (a window's ~490 packets per camera do not fill the chip: two launches each would only add latency)
    HIP_TRY(dsi::launch_prepare_cameras(st, prep, n, geom, bp));
    // workgroup -> stretch of (band, plane) pairs, balanced by the records the tables hold per pair
    const uint32_t* splits = nullptr;
    if (balance) {
        HIP_TRY(out->fused_splits.reserve((size_t)dsi::fused_grid_blocks() + 1));
        HIP_TRY(out->fused_prefix.reserve((size_t)n_pairs));
        HIP_TRY(dsi::launch_fused_splits(st, mappers[0]->pair_work.p, n > 1 ? mappers[1]->pair_work.p : nullptr, n_pairs,
                                         (uint32_t)(out->fused_fixed_cost * n), out->fused_prefix.p, out->fused_splits.p));
        splits = out->fused_splits.p;
    }
    const size_t npix = (size_t)geom.nx * geom.ny;
    HIP_TRY(out->conf.reserve(npix));
    HIP_TRY(out->depth.reserve(npix));
    HIP_TRY(out->idx.reserve(npix));
    if (int rc = depth_buffers_acquire(out)) return rc;
    // one key per pixel, zero before the kernel: zeroed once when (re)allocated, then by every unpack
    // (or after a call that failed between the voting kernel and the unpack)
    if (out->fused_keys.cap < npix + dsi::kFusedKeyTail || out->fused_keys_dirty) {
        HIP_TRY(out->fused_keys.reserve(npix + dsi::kFusedKeyTail));  // (+ the pair-dealing counters)
        HIP_TRY(hipMemsetAsync(out->fused_keys.p, 0, out->fused_keys.cap * sizeof(unsigned long long), st));
    }
    out->fused_keys_dirty = true;
    {
        VoteTimer vt(out);
        HIP_TRY(dsi::launch_vote_fuse_argmax(st, cams, geom, bp, op, splits, out->fused_keys.p,
                                             out->fused_trace_on ? out->fused_trace.p : nullptr));
        vt.stop();
    }
    // keys -> confidence, index, depth over the planes the cameras voted (mapper_emvs_stereo.cpp:302-313)
    HIP_TRY(dsi::launch_unpack_argmax(st, out->fused_keys.p, (int)npix, out->planes_dev.p, out->conf.p, out->idx.p,
                                      out->depth.p, /*clear=*/1));
    out->fused_keys_dirty = false;
    return depth_buffers_ready(out);
}

/* ---- Alg. 2 of one window without a DSI (include/dsi_engine.h) ---- */
constexpr size_t kAlg2PlanEventsPerSub = 1250000;  // both cameras' events per sub-interval (dsi_alg2_plan)
int dsi_alg2_subintervals(size_t n_events, int n_sub, int process_method, int camera, size_t* ranges)
{
    REQUIRE(ranges, DSI_ERR_INVALID, "null argument");
    REQUIRE(n_sub >= 1, DSI_ERR_INVALID, "num_subintervals must be >= 1 (got %d)", n_sub);
    REQUIRE(process_method == 2 || process_method == 5, DSI_ERR_INVALID, "process_method 2 or 5 (got %d)", process_method);
    REQUIRE(camera == 0 || camera == 1, DSI_ERR_INVALID, "camera 0 or 1 (got %d)", camera);
    const size_t per = n_events / (size_t)n_sub;  // process2.cpp:46-47 (the tail is dropped)
    // process5.cpp:89-93: the right camera starts at shift * per, shift = N / 2, and wraps around the end of its events
    const bool shuffled = process_method == 5 && camera == 1;
    size_t idx = shuffled ? (size_t)(n_sub / 2) * per : 0;
    for (int k = 0; k < n_sub; ++k) {
        size_t* r = ranges + 4 * (size_t)k;
        if (shuffled && idx + per >= n_events) {  // process5.cpp:135-143 (note the >=)
            r[0] = idx;
            r[1] = n_events;
            r[2] = 0;
            r[3] = idx + per - n_events;
            idx = idx + per - n_events;
        } else {  // process2.cpp:105-107, :132-134; process5.cpp:144-149
            r[0] = idx;
            r[1] = idx + per;
            r[2] = r[3] = 0;
            idx += per;
        }
    }
    return DSI_OK;
}

int dsi_alg2_plan(int n_sub, size_t n_events, int nx, int camera_time)
{
    if (n_sub < 1 || n_sub > dsi::kAlg2MaxSub) return 0;
    // the band of the kernel's smallest register plan (lane mappings 5 / 6) must hold 3 rows: 2 halo + 1 owned
    if (nx < 2 || (size_t)3 * (size_t)nx > std::min(dsi::alg2_max_cells(5, camera_time != 0), dsi::alg2_max_cells(6, camera_time != 0)))
        return 0;
    // measured: the DSI-less kernel's cost grows with the voting phases times the records, the
    // materialising path's with the records plus 2 N volume passes; past ~2.5 M events per sub-interval pair the
    // materialising path wins
    return n_events <= (size_t)kAlg2PlanEventsPerSub * (size_t)n_sub ? 1 : 0;
}

int dsi_mapper_depth_map_of_events_alg2(dsi_mapper_t* out_tc, dsi_mapper_t* out_ct, dsi_mapper_t* const* cams,
                                        const dsi_batch_t* const* batches, int n_sub, int stereo_fusion, int temporal_fusion)
{
    REQUIRE(out_tc && cams && batches && cams[0] && cams[1], DSI_ERR_INVALID, "null argument");
    REQUIRE(n_sub >= 1 && n_sub <= dsi::kAlg2MaxSub, DSI_ERR_INVALID, "num_subintervals must be 1..%d here (got %d)",
            dsi::kAlg2MaxSub, n_sub);
    REQUIRE(stereo_fusion >= 1 && stereo_fusion <= 6, DSI_ERR_BAD_OP, "Improper stereo fusion method %d (expected 1..6)",
            stereo_fusion);
    REQUIRE(out_ct != out_tc, DSI_ERR_INVALID, "time_camera and camera_time need distinct output mappers");
    dsi_context* ctx = out_tc->ctx;
    dsi_mapper* outs[2] = {out_tc, out_ct};
    const int n_out = out_ct ? 2 : 1;
    const int n_batches = 2 * n_sub;
    for (int i = 0; i < n_batches; ++i) {
        REQUIRE(batches[i], DSI_ERR_INVALID, "batch %d: null", i);
        REQUIRE(batches[i]->ctx == ctx, DSI_ERR_CONTEXT, "batches and output mappers must share one context");
    }
    for (int c = 0; c < 2; ++c) {
        REQUIRE(cams[c]->ctx == ctx, DSI_ERR_CONTEXT, "camera mappers and output mappers must share one context");
        REQUIRE(same_shape(out_tc->grid, cams[c]->grid), DSI_ERR_SHAPE, "camera %d: DSI shape differs from the output mapper's", c);
    }
    if (out_ct) {
        REQUIRE(out_ct->ctx == ctx, DSI_ERR_CONTEXT, "the two output mappers must share one context");
        REQUIRE(same_shape(out_tc->grid, out_ct->grid), DSI_ERR_SHAPE, "the two output mappers' DSI shapes differ");
    }
    REQUIRE(out_tc->geom.nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", out_tc->geom.nz);
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const dsi::Geom& geom = cams[0]->geom;
    const size_t npix = (size_t)geom.nx * geom.ny;
    for (int o = 0; o < n_out; ++o) {
        HIP_TRY(outs[o]->conf.reserve(npix));
        HIP_TRY(outs[o]->depth.reserve(npix));
        HIP_TRY(outs[o]->idx.reserve(npix));
    }
    size_t np_max = 0;
    for (int i = 0; i < n_batches; ++i) np_max = std::max(np_max, batches[i]->n_packets);
    if (temporal_fusion != 2 && temporal_fusion != 4) {
        // process2.cpp:213, :227, :240-243: no temporal accumulation -- every grid stays zero, and the depth map is the
        // first maximum of a zero grid: plane 0, confidence 0 (no vote is needed)
        for (int o = 0; o < n_out; ++o) {
            dsi_mapper* m = outs[o];
            if (int rc = depth_buffers_acquire(m)) return rc;
            HIP_TRY(hipMemsetAsync(m->conf.p, 0, npix * sizeof(float), st));
            HIP_TRY(hipMemsetAsync(m->idx.p, 0, npix, st));
            HIP_TRY(dsi::launch_fill(st, m->depth.p, npix, m->planes[0]));
            m->info = dsi_vote_info_t{};
            m->info.algo = DSI_VOTE_FUSED_ARGMAX;
            m->info.n_packets = np_max;
            if (int rc = depth_buffers_ready(m)) return rc;
        }
        return DSI_OK;
    }
    dsi::BandPlan bp{};
    auto cells_ct = [](int mapping) { return dsi::alg2_max_cells(mapping, true); };
    auto cells_tc = [](int mapping) { return dsi::alg2_max_cells(mapping, false); };
    REQUIRE(plan_fused(out_tc, np_max, &bp, 2, out_ct ? +cells_ct : +cells_tc), DSI_ERR_INVALID,
            "grid rows of %d floats do not fit the fused Alg. 2 kernel", geom.nx);
    bp.interleave = 0;  // contiguous pieces of the pair list per workgroup
    if (out_tc->alg2_tables.size() < (size_t)n_batches) out_tc->alg2_tables.resize(n_batches);
    dsi::Alg2Batches bt{};
    bt.n_sub = n_sub;
    dsi::PrepCameraArgs prep[dsi::kFusedMaxCameras] = {};
    int n_prep = 0;
    for (int i = 0; i < n_batches; ++i) {
        dsi_mapper* m = cams[i & 1];  // k-major: (camera 0, camera 1) of sub-interval i / 2
        const dsi_batch* b = batches[i];
        auto& t = out_tc->alg2_tables[i];
        const size_t np = b->n_packets;
        HIP_TRY(t.centers.reserve(std::max<size_t>(np, 1) * 3));
        HIP_TRY(t.sxy.reserve(np * dsi::kPacket + 1));
        HIP_TRY(t.nvalid.reserve(np + (size_t)geom.nz + 9));
        HIP_TRY(t.rowstart.reserve(np * (size_t)(geom.ny + 2 * bp.row_pad + 3) + 2));
        HIP_TRY(t.coef.reserve(np * geom.nz + 1));
        HIP_TRY(t.cuts.reserve(std::max<size_t>(np * geom.nz * bp.bands, 64)));
        if (b->ready) HIP_TRY(hipStreamWaitEvent(st, b->ready, 0));  // uploaded on the copy stream
        // no packets (< 1024 events): evaluateDSI returns false and the sub-interval's DSI stays zero
        if (np == 0) HIP_TRY(hipMemsetAsync(t.nvalid.p, 0, ((size_t)geom.nz + 8) * sizeof(uint32_t), st));
        prep[n_prep++] = dsi::PrepCameraArgs{b->Rt, b->x, b->y, b->first, m->lut_dev.p, m->sensor_w, m->sensor_h, t.centers.p, (int)np,
                                             t.sxy.p, t.nvalid.p, t.rowstart.p, m->planes_dev.p, t.coef.p, t.cuts.p, nullptr, m->geom};
        bt.b[i] = dsi::FusedCamera{t.sxy.p, t.coef.p, t.cuts.p, t.nvalid.p + np, (int)np};
        if (n_prep == dsi::kFusedMaxCameras || i == n_batches - 1) {
            HIP_TRY(dsi::launch_prepare_cameras(st, prep, n_prep, geom, bp));
            n_prep = 0;
        }
    }
    for (int o = 0; o < n_out; ++o) {
        dsi_mapper* m = outs[o];
        m->info = dsi_vote_info_t{};
        m->info.algo = DSI_VOTE_FUSED_ARGMAX;
        m->info.n_packets = np_max;
        m->info.bands = bp.bands;
        m->info.band_rows = bp.band_rows;
        m->info.chunks = 1;
        m->info.block_threads = bp.block_threads;
        m->info.lds_bytes = bp.lds_bytes;
        m->info.packed = bp.packed;
        m->info.group_packets = 1;
        if (int rc = depth_buffers_acquire(m)) return rc;
        if (m->fused_keys.cap < npix + dsi::kFusedKeyTail || m->fused_keys_dirty) {
            HIP_TRY(m->fused_keys.reserve(npix + dsi::kFusedKeyTail));
            HIP_TRY(hipMemsetAsync(m->fused_keys.p, 0, m->fused_keys.cap * sizeof(unsigned long long), st));
        }
        m->fused_keys_dirty = true;
    }
    {
        VoteTimer vt(out_tc);
        HIP_TRY(dsi::launch_vote_alg2_argmax(st, bt, geom, bp, stereo_fusion, temporal_fusion, out_tc->fused_keys.p,
                                             out_ct ? out_ct->fused_keys.p : nullptr));
        vt.stop();
    }
    for (int o = 0; o < n_out; ++o) {
        dsi_mapper* m = outs[o];
        HIP_TRY(dsi::launch_unpack_argmax(st, m->fused_keys.p, (int)npix, m->planes_dev.p, m->conf.p, m->idx.p, m->depth.p,
                                          /*clear=*/1));
        m->fused_keys_dirty = false;
        if (int rc = depth_buffers_ready(m)) return rc;
    }
    return DSI_OK;
}

/* ---- exact tie resolver (include/dsi_engine.h) ---- */
namespace {
constexpr int kTieCounterWords = 24;  // 32-bit words of TieScratch::counters ([16..23]: one bit per plane with a contender)
constexpr int kTieCounterPassWords = 16;  // the words an event pass starts from zero

unsigned bits_for(unsigned long long values)  // bits that hold 0 .. values - 1
{
    unsigned b = 1;
    while (b < 64 && ((unsigned long long)1 << b) < values) ++b;
    return b;
}
}  // namespace

// The values the REFERENCE's summation order gives the voxels ts.cand[0 .. nsv) (linear indices z * npix + p, any order, no
// duplicates) of the DSIs mappers[c] build from batches[c], c < n (1 or 2): ts.exact[c * nsv + i], ts.count[c * nsv + i] on
// the device.  Per camera one inverted event pass (k_tie_hits_binned: the packet's z0 locations binned by tile in LDS,
// every voxel asks which of them the plane transfer can take into its 2 x 2 neighbourhood, those are voted with the
// reference's coordinates, accept test and weights); the recorded votes of all cameras sorted on the device by (camera,
// voxel, event index) and added one by one in fp32 by one thread per (camera, voxel).  grid_stats: also the maxima of
// |grid value - reference-order value| and of the votes per voxel into ts.counters.  Host round trips: ONE read of two
// counters (how many records to sort).
// camera centre + H_z0 of every packet (what the event pass needs besides the raw events).  Depends on no counter: the
// resolver queues it BEFORE it waits for the number of contending voxels, so that the launches behind that wait are not
// held up by it (the dispatch timeline showed ~40 us of idle stream between the wait and the first event pass)
static int tie_packet_geometry(hipStream_t st, dsi_mapper* const* ms, const dsi_batch* const* bs, int n)
{
    for (int c = 0; c < n; ++c) {
        dsi_mapper* m = ms[c];
        const size_t np = bs[c]->n_packets;
        if (!np) continue;
        HIP_TRY(m->H.reserve(np * 9));
        HIP_TRY(m->centers.reserve(np * 3));
        if (bs[c]->ready) HIP_TRY(hipStreamWaitEvent(st, bs[c]->ready, 0));
        // (the events' z0 locations are computed by the event pass itself, packet by packet: no z0 array)
        HIP_TRY(dsi::launch_packet_geometry(st, bs[c]->Rt, (int)np, m->geom, m->centers.p, m->H.p));
    }
    return DSI_OK;
}

static int tie_exact_values_dev(TieScratch& ts, hipStream_t st, dsi_mapper* const* ms, const dsi_batch* const* bs, int n, int nsv,
                                bool grid_stats, long long* votes, bool* table_overflow = nullptr, bool geometry_ready = false)
{
    *votes = 0;
    if (table_overflow) *table_overflow = false;
    if (nsv <= 0) return DSI_OK;
    const dsi::Geom& g0 = ms[0]->geom;
    const int npix = g0.nx * g0.ny;
    size_t np_max = 1;
    for (int c = 0; c < n; ++c) np_max = std::max(np_max, bs[c]->n_packets);
    const unsigned pos_bits = bits_for((unsigned long long)np_max * dsi::kPacket);
    const unsigned rank_bits = bits_for((unsigned long long)n * nsv + 1);  // + 1: the sentinel rank of unused record slots
    REQUIRE(pos_bits + rank_bits <= 64, DSI_ERR_INVALID, "too many voxels x events for a 64-bit sort key");
    const unsigned sentinel = (unsigned)n * (unsigned)nsv;
    const size_t seg = (size_t)dsi::tie_segment_records();
    HIP_TRY(ts.counters.reserve(kTieCounterWords / 2));
    HIP_TRY(ts.desc.reserve((size_t)nsv));
    HIP_TRY(ts.exact.reserve((size_t)n * nsv));
    HIP_TRY(ts.count.reserve((size_t)n * nsv));
    unsigned* cnt = reinterpret_cast<unsigned*>(ts.counters.p);
    HIP_TRY(hipMemsetAsync(cnt + kTieCounterPassWords, 0, (kTieCounterWords - kTieCounterPassWords) * sizeof(unsigned), st));
    HIP_TRY(dsi::launch_tie_desc(st, ts.cand.p, nsv, g0.nx, npix, ts.desc.p, cnt + kTieCounterPassWords));
    if (!geometry_ready)
        if (int rc = tie_packet_geometry(st, ms, bs, n)) return rc;
    // ONE pass per camera into the scratch already held (4 M records to begin with); a pass that runs out of segments only
    // counts what it would have needed, and everything is repeated once with that much room
    size_t cap = std::max<size_t>(ts.keys.cap, (size_t)1 << 22);
    unsigned host_cnt[4] = {0, 0, 0, 0};  // segments, flags, votes (64 bits)
    for (int attempt = 0;; ++attempt) {
        cap = (cap + seg - 1) / seg * seg;
        HIP_TRY(ts.keys.reserve(cap));
        HIP_TRY(ts.keys2.reserve(cap));
        HIP_TRY(ts.w.reserve(cap));
        const unsigned cap_segs = (unsigned)std::min<size_t>(ts.keys.cap / seg, 0x7fffffffu);
        HIP_TRY(hipMemsetAsync(cnt + 2, 0, (kTieCounterPassWords - 2) * sizeof(unsigned), st));
        for (int c = 0; c < n; ++c) {
            dsi_mapper* m = ms[c];
            if (!bs[c]->n_packets) continue;
            HIP_TRY(dsi::launch_tie_hits_binned(st, bs[c]->x, bs[c]->y, bs[c]->first, m->H.p, m->lut_dev.p, m->sensor_w, m->sensor_h,
                                                m->centers.p, m->planes_dev.p, m->geom, (int)bs[c]->n_packets, ts.desc.p, nsv,
                                                (unsigned)c * (unsigned)nsv, pos_bits, sentinel, cnt + 2, cap_segs, cnt + 3,
                                                ts.counters.p + 4, ts.keys.p, ts.w.p));
        }
        unsigned* pinned = nullptr;
        HIP_TRY(ts.host_counters(&pinned));
        HIP_TRY(hipMemcpyAsync(pinned, cnt, kTieCounterPassWords * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        host_cnt[0] = pinned[2];
        host_cnt[1] = pinned[3];
        host_cnt[2] = pinned[8];
        host_cnt[3] = pinned[9];
        if ((host_cnt[1] & 1u) && table_overflow) {  // (a WIDENED pass of the resolver: the caller keeps the last good pass)
            *table_overflow = true;
            return DSI_OK;
        }
        REQUIRE(!(host_cnt[1] & 1u), DSI_ERR_INVALID, "a workgroup recorded more than %d k votes: too many voxels asked for",
                dsi::tie_block_capacity_records() >> 10);
        if (!(host_cnt[1] & 2u)) break;
        REQUIRE(attempt == 0, DSI_ERR_INVALID, "the vote count changed between two passes");
        cap = (size_t)host_cnt[0] * seg;
        REQUIRE(cap < ((size_t)1 << 33), DSI_ERR_INVALID, "%zu votes to re-sum: too many voxels asked for", cap);
    }
    unsigned long long real_votes = 0;
    std::memcpy(&real_votes, host_cnt + 2, sizeof real_votes);
    *votes = (long long)real_votes;
    const size_t n_rec = (size_t)host_cnt[0] * seg;  // with the sentinel tails of the blocks' last segments
    // the votes partitioned by (camera, voxel), each voxel's run put in event order in LDS and added one by one (round 6: no
    // device-wide sort, no library call)
    REQUIRE(pos_bits <= 32 && n_rec < ((size_t)1 << 32), DSI_ERR_INVALID, "%zu votes to re-sum: too many voxels asked for", n_rec);
    if (grid_stats) HIP_TRY(ts.diff.reserve((size_t)n * nsv));
    HIP_TRY(ts.rank_count.reserve((size_t)n * nsv));
    HIP_TRY(ts.rank_start.reserve((size_t)n * nsv + 1));
    HIP_TRY(ts.rank_cursor.reserve(dsi::tie_partition_cursor_words((size_t)n * nsv)));
    HIP_TRY(dsi::launch_tie_partition_sums(st, ts.keys.p, ts.w.p, n_rec, pos_bits, ts.rank_count.p, ts.rank_start.p, ts.rank_cursor.p,
                                           ts.keys2.p, ts.cand.p, nsv, n, grid_stats ? ms[0]->grid->data : nullptr,
                                           grid_stats && n > 1 ? ms[1]->grid->data : nullptr, ts.exact.p, ts.count.p,
                                           grid_stats ? ts.diff.p : nullptr));
    return DSI_OK;
}

// columns of op(a, b) (b == nullptr: of a) with >= 2 planes within rel_gap of the column's maximum: their voxels into
// ts.cand (a column's run contiguous and ascending in z), the columns into ts.cols (k_tie_candidates); counts to the host
static int tie_candidates_dev(TieScratch& ts, hipStream_t st, const float* a, const float* b, int op, int npix, int nz, float rel_gap,
                              unsigned* n_cand, unsigned* n_columns)
{
    const size_t nvox = (size_t)npix * nz;
    unsigned counters[2] = {0, 0};
    HIP_TRY(ts.counters.reserve(kTieCounterWords / 2));
    size_t cap = std::max<size_t>(ts.cand.cap, std::min<size_t>(nvox, (size_t)1 << 20));
    size_t cols_cap = std::max<size_t>(ts.cols.cap, std::min<size_t>((size_t)npix, (size_t)1 << 18));
    for (;;) {
        HIP_TRY(ts.cand.reserve(cap));
        HIP_TRY(ts.cols.reserve(cols_cap));
        HIP_TRY(hipMemsetAsync(ts.counters.p, 0, kTieCounterWords * sizeof(unsigned), st));
        unsigned* d_cnt = reinterpret_cast<unsigned*>(ts.counters.p);
        HIP_TRY(dsi::launch_tie_candidates(st, a, b, op, npix, nz, rel_gap, d_cnt, ts.cand.p, (uint32_t)std::min<size_t>(cap, 0xffffffffu),
                                           ts.cols.p, (uint32_t)std::min<size_t>(cols_cap, 0xffffffffu)));
        unsigned* pinned = nullptr;
        HIP_TRY(ts.host_counters(&pinned));
        HIP_TRY(hipMemcpyAsync(pinned, d_cnt, sizeof counters, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        counters[0] = pinned[0];
        counters[1] = pinned[1];
        if (counters[0] <= cap && counters[1] <= cols_cap) break;
        REQUIRE(cap < nvox || cols_cap < (size_t)npix, DSI_ERR_INVALID, "more contending voxels than voxels");
        cap = std::min<size_t>(nvox, std::max<size_t>(cap, counters[0]));
        cols_cap = std::min<size_t>((size_t)npix, std::max<size_t>(cols_cap, counters[1]));
    }
    *n_cand = counters[0];
    *n_columns = counters[1];
    return DSI_OK;
}

int dsi_mapper_resolve_near_ties(dsi_mapper_t* out, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches, int n,
                                 int op, dsi_resolve_info_t* info)
{
    REQUIRE(out && mappers && batches && info, DSI_ERR_INVALID, "null argument");
    REQUIRE(n == 1 || n == 2, DSI_ERR_INVALID, "1 or 2 cameras (got %d)", n);
    REQUIRE(n == 1 || (op >= 1 && op <= 6), DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    float rel_gap = info->rel_gap > 0.f ? info->rel_gap : 2.5e-4f;
    REQUIRE(rel_gap < 0.5f, DSI_ERR_INVALID, "rel_gap %g is not a rounding-sized gap", (double)rel_gap);
    dsi_context* ctx = out->ctx;
    for (int i = 0; i < n; ++i) {
        REQUIRE(mappers[i] && batches[i], DSI_ERR_INVALID, "camera %d: null mapper or batch", i);
        REQUIRE(mappers[i]->ctx == ctx && batches[i]->ctx == ctx, DSI_ERR_CONTEXT,
                "mappers, batches and the output mapper must share one context");
        REQUIRE(same_shape(out->grid, mappers[i]->grid), DSI_ERR_SHAPE, "camera %d: DSI shape differs from the output mapper's", i);
    }
    REQUIRE(n == 1 || mappers[0] != mappers[1], DSI_ERR_INVALID, "the cameras need distinct mappers");
    REQUIRE(out->depth_valid, DSI_ERR_INVALID, "the output mapper holds no raw depth map to resolve");
    const dsi::Geom& g0 = out->geom;
    const int npix = g0.nx * g0.ny, nz = g0.nz;
    const size_t nvox = (size_t)npix * nz;
    REQUIRE(nvox < ((size_t)1 << 32), DSI_ERR_INVALID, "the resolver addresses voxels with 32 bits");
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const auto t_begin = std::chrono::steady_clock::now();
    *info = dsi_resolve_info_t{};
    TieScratch& ts = out->tie;  // grow-only scratch of the output mapper: a stream of calls allocates nothing
    auto finish = [&]() {
        info->elapsed_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        return DSI_OK;
    };
    // The premise -- the two summation orders differ by far less than the gap whose columns are re-summed -- is CHECKED,
    // not assumed: max_order_diff is measured on the re-summed voxels (the column maxima of the near-tie columns, among
    // them the most-voted voxels of the volume), and a pass that finds it above rel_gap / 8 is repeated with a gap four
    // times as wide (at most three times); premise_ok tells whether the last pass held it.
    // A WIDENED pass can ask for orders of magnitude more voxels than the first; if it overflows a workgroup's segment
    // table (or the 32-bit bookkeeping) the call does not fail: it keeps the last completed pass's patch and statistics
    // and returns DSI_OK with premise_ok = 0 -- "the caller decides", as the header says.
    {
        dsi_mapper* ms0[2] = {mappers[0], n == 2 ? mappers[1] : nullptr};
        const dsi_batch* bs0[2] = {batches[0], n == 2 ? batches[1] : nullptr};
        if (int rc = tie_packet_geometry(st, ms0, bs0, n)) return rc;  // (queued ahead of the first wait below)
    }
    for (int widenings = 0;; ++widenings) {
        const dsi_resolve_info_t last_good = *info;
        info->rel_gap = rel_gap;
        info->gap_widenings = widenings;
        // 1. the contending voxels (device lists)
        unsigned n_cand = 0, n_columns = 0;
        if (int rc = tie_candidates_dev(ts, st, mappers[0]->grid->data, n == 2 ? mappers[1]->grid->data : nullptr, op, npix, nz, rel_gap,
                                        &n_cand, &n_columns))
            return rc;
        info->near_tie_pixels = (int)n_columns;
        info->candidate_voxels = (int)n_cand;
        info->premise_ok = 1;
        if (!n_cand) return finish();
        // 2 + 3. per camera: the contending voxels' values in the reference's summation order (device)
        long long votes = 0;
        dsi_mapper* ms[2] = {mappers[0], n == 2 ? mappers[1] : nullptr};
        const dsi_batch* bs[2] = {batches[0], n == 2 ? batches[1] : nullptr};
        bool overflow = false;
        if (int rc = tie_exact_values_dev(ts, st, ms, bs, n, (int)n_cand, /*grid_stats=*/true, &votes, widenings > 0 ? &overflow : nullptr,
                                          /*geometry_ready=*/true)) {
            if (widenings == 0) return rc;
            overflow = true;  // (too many voxels x events for the sort key, > 2^33 votes: the same verdict)
            g_last_error.clear();
        }
        if (overflow) {
            *info = last_good;  // (premise_ok = 0 there: that is why this pass was tried)
            return finish();
        }
        info->votes = votes;
        // 4. fuse, first maximum per column, patch (device)
        if (int rc = depth_buffers_acquire(out)) return rc;
        unsigned* cnt = reinterpret_cast<unsigned*>(ts.counters.p);
        HIP_TRY(dsi::launch_tie_pick(st, n == 2 ? op : 0, ts.cols.p, (int)n_columns, ts.cand.p, (int)n_cand, npix, ts.exact.p, ts.count.p,
                                     ts.diff.p, out->planes_dev.p, out->conf.p, out->idx.p, out->depth.p, cnt + 4, rel_gap));
        if (int rc = depth_buffers_ready(out)) return rc;
        unsigned stats[4] = {0, 0, 0, 0};
        unsigned* pinned = nullptr;
        HIP_TRY(ts.host_counters(&pinned));
        HIP_TRY(hipMemcpyAsync(pinned, cnt, kTieCounterWords * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(stats, pinned + 4, sizeof stats);
        info->candidate_planes = 0;
        for (int wd = 0; wd < kTieCounterWords - kTieCounterPassWords; ++wd) info->candidate_planes += __builtin_popcount(pinned[kTieCounterPassWords + wd]);
        float diff = 0.f;
        std::memcpy(&diff, &stats[0], sizeof diff);
        info->max_order_diff = (double)diff;  // (of the last pass: what its premise is checked with)
        info->max_rel_bound = stats[1] > 1 ? (double)(stats[1] - 1) * 5.9604644775390625e-8 : 0.0;
        info->changed_pixels += (int)stats[2];
        info->columns_bounded = (int)stats[3];
        info->premise_ok = (8.0 * (double)diff < (double)rel_gap) ? 1 : 0;  // (false for a NaN difference, too)
        if (info->premise_ok || widenings == 3 || rel_gap * 4.f >= 0.5f) return finish();
        rel_gap *= 4.f;
    }
}

int dsi_mapper_prove_near_ties(dsi_mapper_t* out, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches, int n, int op,
                               dsi_prove_info_t* info)
{
    REQUIRE(out && mappers && batches && info, DSI_ERR_INVALID, "null argument");
    REQUIRE(n == 1 || n == 2, DSI_ERR_INVALID, "1 or 2 cameras (got %d)", n);
    REQUIRE(n == 1 || (op >= 1 && op <= 6), DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    const float rel_gap = info->rel_gap > 0.f ? info->rel_gap : 2.5e-4f;
    REQUIRE(rel_gap < 0.5f, DSI_ERR_INVALID, "rel_gap %g is not a rounding-sized gap", (double)rel_gap);
    dsi_context* ctx = out->ctx;
    for (int i = 0; i < n; ++i) {
        REQUIRE(mappers[i] && batches[i], DSI_ERR_INVALID, "camera %d: null mapper or batch", i);
        REQUIRE(mappers[i]->ctx == ctx && batches[i]->ctx == ctx, DSI_ERR_CONTEXT,
                "mappers, batches and the output mapper must share one context");
        REQUIRE(same_shape(out->grid, mappers[i]->grid), DSI_ERR_SHAPE, "camera %d: DSI shape differs from the output mapper's", i);
        // the bounds describe the EXACT sums of the LDS-band mappings (weights truncated to 2^-31, one rounding): a DSI voted
        // with fp32 global atomics or with the paired 32-bit cells (rounded Q.19 weights) is not one
        REQUIRE(batches[i]->n_packets == 0 || (mappers[i]->info.algo == DSI_VOTE_LDS_BANDS && mappers[i]->info.packed != 8),
                DSI_ERR_INVALID, "camera %d: the proof needs a DSI of exact sums (DSI_VOTE_LDS_BANDS, not lane mapping 8)", i);
    }
    REQUIRE(n == 1 || mappers[0] != mappers[1], DSI_ERR_INVALID, "the cameras need distinct mappers");
    const dsi::Geom& g0 = out->geom;
    const size_t nvox = (size_t)g0.nx * g0.ny * g0.nz;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const auto t_begin = std::chrono::steady_clock::now();
    *info = dsi_prove_info_t{};
    info->rel_gap = rel_gap;
    TieScratch& ts = out->tie;
    dsi_mapper* ms[2] = {mappers[0], n == 2 ? mappers[1] : nullptr};
    const dsi_batch* bs[2] = {batches[0], n == 2 ? batches[1] : nullptr};
    if (int rc = tie_packet_geometry(st, ms, bs, n)) return rc;
    for (bool& v : ts.votes_valid) v = false;
    for (int c = 0; c < n; ++c) {
        HIP_TRY(ts.votes[c].reserve(nvox));
        HIP_TRY(hipMemsetAsync(ts.votes[c].p, 0, nvox * sizeof(uint32_t), st));
        dsi_mapper* m = ms[c];
        if (!bs[c]->n_packets) continue;
        HIP_TRY(dsi::launch_count_votes(st, bs[c]->x, bs[c]->y, bs[c]->first, m->H.p, m->lut_dev.p, m->sensor_w, m->sensor_h, m->centers.p,
                                        m->planes_dev.p, m->geom, (int)bs[c]->n_packets, ts.votes[c].p));
    }
    HIP_TRY(ts.counters.reserve(kTieCounterWords / 2));
    unsigned* cnt = reinterpret_cast<unsigned*>(ts.counters.p);
    HIP_TRY(hipMemsetAsync(cnt, 0, 5 * sizeof(unsigned), st));
    HIP_TRY(ts.unproven.reserve((size_t)g0.nx * g0.ny));
    ts.n_unproven = 0;
    HIP_TRY(dsi::launch_tie_prove(st, ms[0]->grid->data, n == 2 ? ms[1]->grid->data : nullptr, ts.votes[0].p, n == 2 ? ts.votes[1].p : nullptr,
                                  op, g0.nx, g0.ny, g0.nz, rel_gap, cnt, ts.unproven.p));
    unsigned* pinned = nullptr;
    HIP_TRY(ts.host_counters(&pinned));
    HIP_TRY(hipMemcpyAsync(pinned, cnt, 5 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int c = 0; c < n; ++c) ts.votes_valid[c] = true;
    ts.n_unproven = pinned[4];
    info->columns = (long long)g0.nx * g0.ny;
    info->columns_proven = pinned[0];
    info->columns_unproven = pinned[1];
    float need = 0.f;
    std::memcpy(&need, &pinned[2], sizeof need);
    info->gap_needed = pinned[1] ? (double)need : 0.0;
    info->max_votes = pinned[3];
    info->elapsed_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return DSI_OK;
}

int dsi_mapper_prove_near_ties_n(dsi_mapper_t* out, dsi_grid_t* fused, dsi_mapper_t* const* mappers, const dsi_batch_t* const* batches,
                                 int n, int mode, dsi_prove_info_t* info)
{
    REQUIRE(out && fused && mappers && batches && info, DSI_ERR_INVALID, "null argument");
    REQUIRE(n >= 1 && n <= 8, DSI_ERR_INVALID, "1 to 8 cameras (got %d)", n);
    REQUIRE(mode == DSI_ACC_GM_TREE || mode == DSI_ACC_MIN || mode == DSI_ACC_MAX || mode == DSI_ACC_SUM, DSI_ERR_BAD_OP,
            "mode %d: the proof covers DSI_ACC_GM_TREE, DSI_ACC_MIN, DSI_ACC_MAX and DSI_ACC_SUM", mode);
    REQUIRE(mode != DSI_ACC_GM_TREE || n == 2 || n == 4 || n == 8, DSI_ERR_BAD_OP, "DSI_ACC_GM_TREE needs 2, 4 or 8 cameras (got %d)", n);
    const float rel_gap = info->rel_gap > 0.f ? info->rel_gap : 2.5e-4f;
    REQUIRE(rel_gap < 0.5f, DSI_ERR_INVALID, "rel_gap %g is not a rounding-sized gap", (double)rel_gap);
    dsi_context* ctx = out->ctx;
    REQUIRE(fused->ctx == ctx && same_shape(out->grid, fused), DSI_ERR_SHAPE, "the fused grid must have the output mapper's shape and context");
    for (int i = 0; i < n; ++i) {
        REQUIRE(mappers[i] && batches[i], DSI_ERR_INVALID, "camera %d: null mapper or batch", i);
        REQUIRE(mappers[i]->ctx == ctx && batches[i]->ctx == ctx, DSI_ERR_CONTEXT,
                "mappers, batches and the output mapper must share one context");
        REQUIRE(same_shape(out->grid, mappers[i]->grid), DSI_ERR_SHAPE, "camera %d: DSI shape differs from the output mapper's", i);
        REQUIRE(batches[i]->n_packets == 0 || (mappers[i]->info.algo == DSI_VOTE_LDS_BANDS && mappers[i]->info.packed != 8),
                DSI_ERR_INVALID, "camera %d: the proof needs a DSI of exact sums (DSI_VOTE_LDS_BANDS, not lane mapping 8)", i);
        for (int k = 0; k < i; ++k) REQUIRE(mappers[i] != mappers[k], DSI_ERR_INVALID, "the cameras need distinct mappers");
    }
    const dsi::Geom& g0 = out->geom;
    const size_t nvox = (size_t)g0.nx * g0.ny * g0.nz;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const auto t_begin = std::chrono::steady_clock::now();
    *info = dsi_prove_info_t{};
    info->rel_gap = rel_gap;
    TieScratch& ts = out->tie;
    for (bool& v : ts.votes_valid) v = false;
    const float* e[8] = {};
    const uint32_t* h[8] = {};
    for (int c = 0; c < n; ++c) {
        dsi_mapper* m = mappers[c];
        const dsi_batch* b = batches[c];
        dsi_mapper* one_m[1] = {m};
        const dsi_batch* one_b[1] = {b};
        if (int rc = tie_packet_geometry(st, one_m, one_b, 1)) return rc;
        HIP_TRY(ts.votes[c].reserve(nvox));
        HIP_TRY(hipMemsetAsync(ts.votes[c].p, 0, nvox * sizeof(uint32_t), st));
        if (b->n_packets)
            HIP_TRY(dsi::launch_count_votes(st, b->x, b->y, b->first, m->H.p, m->lut_dev.p, m->sensor_w, m->sensor_h, m->centers.p,
                                            m->planes_dev.p, m->geom, (int)b->n_packets, ts.votes[c].p));
        e[c] = m->grid->data;
        h[c] = ts.votes[c].p;
    }
    HIP_TRY(ts.counters.reserve(kTieCounterWords / 2));
    unsigned* cnt = reinterpret_cast<unsigned*>(ts.counters.p);
    HIP_TRY(hipMemsetAsync(cnt, 0, 5 * sizeof(unsigned), st));
    HIP_TRY(ts.unproven.reserve((size_t)g0.nx * g0.ny));
    ts.n_unproven = 0;
    HIP_TRY(dsi::launch_tie_prove_n(st, fused->data, e, h, n, mode, g0.nx, g0.ny, g0.nz, rel_gap, cnt, ts.unproven.p));
    unsigned* pinned = nullptr;
    HIP_TRY(ts.host_counters(&pinned));
    HIP_TRY(hipMemcpyAsync(pinned, cnt, 5 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int c = 0; c < n; ++c) ts.votes_valid[c] = true;
    ts.n_unproven = pinned[4];
    info->columns = (long long)g0.nx * g0.ny;
    info->columns_proven = pinned[0];
    info->columns_unproven = pinned[1];
    float need = 0.f;
    std::memcpy(&need, &pinned[2], sizeof need);
    info->gap_needed = pinned[1] ? (double)need : 0.0;
    info->max_votes = pinned[3];
    info->elapsed_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return DSI_OK;
}

int dsi_mapper_reference_interval(dsi_mapper_t* scratch, dsi_mapper_t* m, const dsi_batch_t* batch, dsi_grid_t* lo, dsi_grid_t* hi)
{
    REQUIRE(scratch && m && batch && lo && hi, DSI_ERR_INVALID, "null argument");
    dsi_context* ctx = scratch->ctx;
    REQUIRE(m->ctx == ctx && batch->ctx == ctx && lo->ctx == ctx && hi->ctx == ctx, DSI_ERR_CONTEXT, "everything must share one context");
    REQUIRE(same_shape(scratch->grid, m->grid) && same_shape(m->grid, lo) && same_shape(m->grid, hi), DSI_ERR_SHAPE, "shapes differ");
    REQUIRE(lo != hi && lo != m->grid && hi != m->grid, DSI_ERR_INVALID, "lo, hi and the DSI must be three grids");
    REQUIRE(batch->n_packets == 0 || (m->info.algo == DSI_VOTE_LDS_BANDS && m->info.packed != 8), DSI_ERR_INVALID,
            "the bounds need a DSI of exact sums (DSI_VOTE_LDS_BANDS, not lane mapping 8)");
    const dsi::Geom& g0 = m->geom;
    const size_t nvox = (size_t)g0.nx * g0.ny * g0.nz;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    TieScratch& ts = scratch->tie;
    dsi_mapper* one_m[1] = {m};
    const dsi_batch* one_b[1] = {batch};
    if (int rc = tie_packet_geometry(st, one_m, one_b, 1)) return rc;
    HIP_TRY(ts.votes[7].reserve(nvox));  // (the last counter volume: the cameras' own of a proof stay valid)
    ts.votes_valid[7] = false;
    HIP_TRY(hipMemsetAsync(ts.votes[7].p, 0, nvox * sizeof(uint32_t), st));
    if (batch->n_packets)
        HIP_TRY(dsi::launch_count_votes(st, batch->x, batch->y, batch->first, m->H.p, m->lut_dev.p, m->sensor_w, m->sensor_h, m->centers.p,
                                        m->planes_dev.p, m->geom, (int)batch->n_packets, ts.votes[7].p));
    HIP_TRY(ts.interval_most.reserve(1));
    if (!ts.interval_most_live) {
        HIP_TRY(hipMemsetAsync(ts.interval_most.p, 0, sizeof(unsigned), st));
        ts.interval_most_live = true;
    }
    HIP_TRY(dsi::launch_interval_of_counts(st, m->grid->data, ts.votes[7].p, g0.nx, g0.ny, g0.nz, lo->data, hi->data, ts.interval_most.p));
    return DSI_OK;
}

int dsi_grid_widen_interval(dsi_grid_t* lo, dsi_grid_t* hi, int roundings)
{
    if (int rc = check_pair(lo, hi)) return rc;
    REQUIRE(lo != hi, DSI_ERR_INVALID, "lo and hi must be two grids");
    REQUIRE(roundings >= 1 && roundings <= 4096, DSI_ERR_INVALID, "roundings %d (1 .. 4096)", roundings);
    HIP_TRY(dsi::launch_interval_widen(lo->ctx->stream, lo->data, hi->data, lo->n, roundings));
    return DSI_OK;
}

int dsi_grid_prove_columns(dsi_mapper_t* scratch, dsi_grid_t* fused, dsi_grid_t* lo, dsi_grid_t* hi, dsi_prove_info_t* info)
{
    REQUIRE(scratch && fused && lo && hi && info, DSI_ERR_INVALID, "null argument");
    dsi_context* ctx = scratch->ctx;
    REQUIRE(fused->ctx == ctx && lo->ctx == ctx && hi->ctx == ctx, DSI_ERR_CONTEXT, "everything must share one context");
    REQUIRE(same_shape(scratch->grid, fused) && same_shape(fused, lo) && same_shape(fused, hi), DSI_ERR_SHAPE, "shapes differ");
    const float rel_gap = info->rel_gap > 0.f ? info->rel_gap : 2.5e-4f;
    REQUIRE(rel_gap < 0.5f, DSI_ERR_INVALID, "rel_gap %g is not a rounding-sized gap", (double)rel_gap);
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const auto t_begin = std::chrono::steady_clock::now();
    *info = dsi_prove_info_t{};
    info->rel_gap = rel_gap;
    TieScratch& ts = scratch->tie;
    HIP_TRY(ts.counters.reserve(kTieCounterWords / 2));
    unsigned* cnt = reinterpret_cast<unsigned*>(ts.counters.p);
    HIP_TRY(hipMemsetAsync(cnt, 0, 5 * sizeof(unsigned), st));
    const int npix = fused->nx * fused->ny;
    HIP_TRY(ts.unproven.reserve((size_t)npix));
    ts.n_unproven = 0;
    HIP_TRY(dsi::launch_prove_columns(st, fused->data, lo->data, hi->data, npix, fused->nz, rel_gap, cnt, ts.unproven.p));
    unsigned* pinned = nullptr;
    HIP_TRY(ts.host_counters(&pinned));
    HIP_TRY(hipMemcpyAsync(pinned, cnt, 5 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (ts.interval_most_live) HIP_TRY(hipMemcpyAsync(pinned + 8, ts.interval_most.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ts.votes_valid[0] = true;  // (dsi_mapper_proof_unproven asks whether a proof has run)
    ts.n_unproven = pinned[4];
    info->columns = npix;
    info->columns_proven = pinned[0];
    info->columns_unproven = pinned[1];
    float need = 0.f;
    std::memcpy(&need, &pinned[2], sizeof need);
    info->gap_needed = pinned[1] ? (double)need : 0.0;
    info->max_votes = ts.interval_most_live ? pinned[8] : 0;
    ts.interval_most_live = false;  // (the next composition starts its own maximum)
    info->elapsed_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return DSI_OK;
}

int dsi_mapper_proof_unproven(dsi_mapper_t* out, uint32_t* pixels, float* gaps, size_t capacity, size_t* n)
{
    REQUIRE(out && n && (capacity == 0 || pixels), DSI_ERR_INVALID, "null argument");
    TieScratch& ts = out->tie;
    REQUIRE(ts.votes_valid[0], DSI_ERR_INVALID, "no proof has run on this mapper");
    *n = ts.n_unproven;
    const size_t take = std::min(capacity, ts.n_unproven);
    if (!take) return DSI_OK;
    if (int rc = set_device(out->ctx)) return rc;
    std::vector<uint2> host(take);
    HIP_TRY(hipMemcpyAsync(host.data(), ts.unproven.p, take * sizeof(uint2), hipMemcpyDeviceToHost, out->ctx->stream));
    HIP_TRY(hipStreamSynchronize(out->ctx->stream));
    for (size_t i = 0; i < take; ++i) {
        pixels[i] = host[i].x;
        if (gaps) std::memcpy(&gaps[i], &host[i].y, sizeof(float));
    }
    return DSI_OK;
}

int dsi_mapper_proof_votes(dsi_mapper_t* out, int camera, const uint32_t* voxels, size_t n, uint32_t* votes)
{
    REQUIRE(out && (n == 0 || (voxels && votes)), DSI_ERR_INVALID, "null argument");
    REQUIRE(camera >= 0 && camera < 8, DSI_ERR_INVALID, "camera %d (0 .. 7)", camera);
    const dsi::Geom& g0 = out->geom;
    const size_t nvox = (size_t)g0.nx * g0.ny * g0.nz;
    TieScratch& ts = out->tie;
    REQUIRE(ts.votes[camera].cap >= nvox && ts.votes_valid[camera], DSI_ERR_INVALID, "no proof has counted camera %d's votes on this mapper", camera);
    REQUIRE(n < ((size_t)1 << 31), DSI_ERR_INVALID, "too many voxels");
    for (size_t i = 0; i < n; ++i) REQUIRE(voxels[i] < nvox, DSI_ERR_INVALID, "voxel %zu (%u) is outside the grid", i, voxels[i]);
    if (n == 0) return DSI_OK;
    if (int rc = set_device(out->ctx)) return rc;
    hipStream_t st = out->ctx->stream;
    HIP_TRY(ts.cand.reserve(n));
    HIP_TRY(ts.count.reserve(n));
    HIP_TRY(hipMemcpyAsync(ts.cand.p, voxels, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(dsi::launch_tie_votes_of(st, ts.votes[camera].p, ts.cand.p, (int)n, g0.nx, g0.ny, ts.count.p));
    HIP_TRY(hipMemcpyAsync(votes, ts.count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (pageable host arrays)
    return DSI_OK;
}

int dsi_grid_near_tie_voxels(dsi_mapper_t* scratch, dsi_grid_t* g, float rel_gap, uint32_t* voxels, size_t capacity,
                             size_t* n_voxels, size_t* n_columns)
{
    REQUIRE(scratch && g && n_voxels, DSI_ERR_INVALID, "null argument");
    REQUIRE(capacity == 0 || voxels, DSI_ERR_INVALID, "null output");
    REQUIRE(scratch->ctx == g->ctx, DSI_ERR_CONTEXT, "the scratch mapper must live in the grid's context");
    REQUIRE(same_shape(scratch->grid, g), DSI_ERR_SHAPE, "the scratch mapper's DSI shape differs from the grid's");
    if (!(rel_gap > 0.f)) rel_gap = 2.5e-4f;
    REQUIRE(rel_gap < 0.5f, DSI_ERR_INVALID, "rel_gap %g is not a rounding-sized gap", (double)rel_gap);
    REQUIRE(g->n < ((size_t)1 << 32), DSI_ERR_INVALID, "voxels are addressed with 32 bits");
    REQUIRE(g->nz <= 256, DSI_ERR_SHAPE, "the near-tie search holds a column's planes in four 64-bit masks: dimZ %d > 256", g->nz);
    if (int rc = set_device(g->ctx)) return rc;
    unsigned n_cand = 0, cols = 0;
    if (int rc = tie_candidates_dev(scratch->tie, g->ctx->stream, g->data, nullptr, 0, g->nx * g->ny, g->nz, rel_gap, &n_cand, &cols)) return rc;
    *n_voxels = n_cand;
    if (n_columns) *n_columns = cols;
    if (n_cand <= capacity && n_cand) HIP_TRY(hipMemcpy(voxels, scratch->tie.cand.p, (size_t)n_cand * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DSI_OK;
}

int dsi_mapper_exact_voxels(dsi_mapper_t* m, const dsi_batch_t* batch, const uint32_t* voxels, size_t n, float* values,
                            uint32_t* votes)
{
    REQUIRE(m && batch, DSI_ERR_INVALID, "null argument");
    REQUIRE(n == 0 || (voxels && values), DSI_ERR_INVALID, "null array");
    REQUIRE(m->ctx == batch->ctx, DSI_ERR_CONTEXT, "mapper and batch belong to different contexts");
    const size_t nvox = (size_t)m->geom.nx * m->geom.ny * m->geom.nz;
    REQUIRE(nvox < ((size_t)1 << 32), DSI_ERR_INVALID, "voxels are addressed with 32 bits");
    for (size_t i = 0; i < n; ++i) REQUIRE(voxels[i] < nvox, DSI_ERR_INVALID, "voxel %zu (%u) outside the DSI", i, voxels[i]);
    if (n == 0) return DSI_OK;
    if (int rc = set_device(m->ctx)) return rc;
    hipStream_t st = m->ctx->stream;
    std::vector<uint32_t> sv(voxels, voxels + n);
    std::sort(sv.begin(), sv.end());
    sv.erase(std::unique(sv.begin(), sv.end()), sv.end());
    REQUIRE(sv.size() < ((size_t)1 << 31), DSI_ERR_INVALID, "too many voxels");
    TieScratch& ts = m->tie;
    HIP_TRY(ts.cand.reserve(sv.size()));
    HIP_TRY(hipMemcpyAsync(ts.cand.p, sv.data(), sv.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    long long total = 0;
    dsi_mapper* ms[1] = {m};
    const dsi_batch* bs[1] = {batch};
    if (int rc = tie_exact_values_dev(ts, st, ms, bs, 1, (int)sv.size(), /*grid_stats=*/false, &total)) return rc;
    std::vector<float> exact(sv.size());
    std::vector<uint32_t> count(sv.size());
    HIP_TRY(hipMemcpyAsync(exact.data(), ts.exact.p, sv.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count.data(), ts.count.p, sv.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (sv is pageable: its upload has completed by now, too)
    for (size_t i = 0; i < n; ++i) {
        const size_t c = (size_t)(std::lower_bound(sv.begin(), sv.end(), voxels[i]) - sv.begin());
        values[i] = exact[c];
        if (votes) votes[i] = count[c];
    }
    return DSI_OK;
}

int dsi_reference_fuse2(int op, const float* a, const float* g, size_t n, float* out)
{
    REQUIRE(n == 0 || (a && g && out), DSI_ERR_INVALID, "null array");
    REQUIRE(op >= 1 && op <= 6, DSI_ERR_BAD_OP, "improper fusion method %d (expected 1..6)", op);
    for (size_t i = 0; i < n; ++i) out[i] = dsi::host::fuse2(op, a[i], g[i]);
    return DSI_OK;
}

int dsi_reference_accumulate(int mode, float* acc, const float* g, size_t n)
{
    REQUIRE(n == 0 || (acc && g), DSI_ERR_INVALID, "null array");
    REQUIRE(mode == DSI_ACC_SUM || mode == DSI_ACC_INV_SUM, DSI_ERR_BAD_OP, "the reference accumulates sums (0) or inverse sums (1)");
    for (size_t i = 0; i < n; ++i) acc[i] = dsi::host::accumulate1(mode, acc[i], g[i]);
    return DSI_OK;
}

int dsi_reference_finalize(int mode, float* acc, size_t n, int n_maps)
{
    REQUIRE(n == 0 || acc, DSI_ERR_INVALID, "null array");
    REQUIRE(mode == DSI_ACC_SUM || mode == DSI_ACC_INV_SUM, DSI_ERR_BAD_OP, "the reference accumulates sums (0) or inverse sums (1)");
    REQUIRE(n_maps >= 1, DSI_ERR_INVALID, "number of maps must be >= 1 (got %d)", n_maps);
    for (size_t i = 0; i < n; ++i) acc[i] = dsi::host::finalize1(mode, acc[i], n_maps);
    return DSI_OK;
}

static int patch_depth_map(dsi_mapper_t* m, TieScratch& ts, const uint32_t* pix, const uint8_t* idx, const float* conf, size_t n)
{
    if (n == 0) return DSI_OK;
    hipStream_t st = m->ctx->stream;
    HIP_TRY(ts.count.reserve(n));
    HIP_TRY(ts.exact.reserve(n));
    HIP_TRY(ts.tmp.reserve(n));
    // (the patch lists reuse the resolver's scratch: pix <- count, conf <- exact, idx <- tmp)
    HIP_TRY(hipMemcpyAsync(ts.count.p, pix, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ts.exact.p, conf, n * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ts.tmp.p, idx, n, hipMemcpyHostToDevice, st));
    if (int rc = depth_buffers_acquire(m)) return rc;
    HIP_TRY(dsi::launch_tie_patch(st, ts.count.p, reinterpret_cast<const uint8_t*>(ts.tmp.p), ts.exact.p, (int)n, m->planes_dev.p,
                                  m->conf.p, m->idx.p, m->depth.p));
    if (int rc = depth_buffers_ready(m)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // the host arrays are pageable
    return DSI_OK;
}

int dsi_mapper_patch_depth_map(dsi_mapper_t* m, const uint32_t* pixels, const uint8_t* idx, const float* conf, size_t n)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(n == 0 || (pixels && idx && conf), DSI_ERR_INVALID, "null array");
    REQUIRE(m->depth_valid, DSI_ERR_INVALID, "the mapper holds no raw depth map to patch");
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    for (size_t i = 0; i < n; ++i) {
        REQUIRE(pixels[i] < npix, DSI_ERR_INVALID, "pixel %zu (%u) outside the image", i, pixels[i]);
        REQUIRE((int)idx[i] < m->geom.nz, DSI_ERR_INVALID, "plane index %d outside the depth vector", (int)idx[i]);
    }
    if (int rc = set_device(m->ctx)) return rc;
    return patch_depth_map(m, m->tie, pixels, idx, conf, n);
}

int dsi_mapper_fetch_depth_map(dsi_mapper_t* m, float* depth_host, float* conf_host, uint8_t* idx_host)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(m->depth_valid, DSI_ERR_INVALID, "no depth map has been computed since the last vote");
    if (int rc = set_device(m->ctx)) return rc;
    return depth_buffers_fetch(m, depth_host, conf_host, idx_host, /*wait=*/true);
}

int dsi_mapper_fetch_depth_map_async(dsi_mapper_t* m, float* depth_host, float* conf_host, uint8_t* idx_host)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(m->depth_valid, DSI_ERR_INVALID, "no depth map has been computed since the last vote");
    if (int rc = set_device(m->ctx)) return rc;
    return depth_buffers_fetch(m, depth_host, conf_host, idx_host, /*wait=*/false);
}

int dsi_mapper_fetch_depth_map_in_order(dsi_mapper_t* m, float* depth_host, float* conf_host, uint8_t* idx_host)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(m->depth_valid, DSI_ERR_INVALID, "no depth map has been computed since the last vote");
    if (int rc = set_device(m->ctx)) return rc;
    return depth_buffers_fetch(m, depth_host, conf_host, idx_host, /*wait=*/false, /*in_order=*/true);
}

int dsi_mapper_fetch_wait(dsi_mapper_t* m)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    if (!m->depth_read_pending) return DSI_OK;
    if (int rc = set_device(m->ctx)) return rc;
    HIP_TRY(hipEventSynchronize(m->ev_depth_read));
    return DSI_OK;
}

int dsi_mapper_depth_map(dsi_mapper_t* m, float* depth_host, float* conf_host, uint8_t* idx_host)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    if (int rc = dsi_mapper_depth_map_of(m, m->grid)) return rc;
    return dsi_mapper_fetch_depth_map(m, depth_host, conf_host, idx_host);
}

int dsi_mapper_set_kernel_timing(dsi_mapper_t* m, int enable)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    m->timing = enable != 0;
    return DSI_OK;
}

int dsi_mapper_vote_kernel_time(dsi_mapper_t* m, float* total_ms, int* launches)
{
    REQUIRE(m && total_ms && launches, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(m->ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    float total = 0.f;
    int n = 0;
    for (size_t i = 0; i + 1 < m->timing_pairs.size(); i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->timing_pairs[i], m->timing_pairs[i + 1]) == hipSuccess) {
            total += ms;
            ++n;
        }
    }
    for (Event& e : m->timing_pairs) m->timing_pool.push_back(std::move(e));
    m->timing_pairs.clear();
    *total_ms = total;
    *launches = n;
    return DSI_OK;
}

static int check_depthmap_options(const dsi_depthmap_options_t* opts)
{
    REQUIRE(opts->adaptive_threshold_kernel_size >= 1 && (opts->adaptive_threshold_kernel_size & 1) &&
                opts->adaptive_threshold_kernel_size <= 63,
            DSI_ERR_INVALID, "adaptive_threshold_kernel_size must be odd and in 1..63");
    REQUIRE(opts->median_filter_size >= 1 && (opts->median_filter_size & 1) && opts->median_filter_size <= 31,
            DSI_ERR_INVALID, "median_filter_size must be odd and in 1..31 (median_filtering.cpp:44)");
    return DSI_OK;
}

int dsi_mapper_filter_depth_map(dsi_mapper_t* m, const dsi_depthmap_options_t* opts, float* depth_host,
                                float* conf_host, uint8_t* mask_host, uint8_t* idx_filtered_host)
{
    REQUIRE(m && opts, DSI_ERR_INVALID, "null argument");
    if (int rc = check_depthmap_options(opts)) return rc;
    REQUIRE(m->depth_valid, DSI_ERR_INVALID,
            "no raw depth map on this mapper: call one of dsi_mapper_depth_map_of* first (a filtered map "
            "cannot be filtered again: the confidence image was normalised in place)");
    dsi_context* ctx = m->ctx;
    const int nx = m->geom.nx, ny = m->geom.ny;
    const size_t npix = (size_t)nx * ny;
    if (int rc = set_device(ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;  // an asynchronous fetch of the raw map may be reading them
    HIP_TRY(m->conf8.reserve(npix));
    HIP_TRY(m->mask.reserve(npix));
    HIP_TRY(m->idx_filtered.reserve(npix));
    HIP_TRY(m->minmax.reserve(2));
    HIP_TRY(dsi::launch_depth_map_filters(ctx->stream, m->conf.p, m->idx.p, nx, ny,
                                          opts->adaptive_threshold_kernel_size, opts->adaptive_threshold_c,
                                          opts->median_filter_size, opts->max_confidence, m->planes_dev.p,
                                          m->minmax.p, m->conf8.p, m->mask.p, m->idx_filtered.p, m->depth.p));
    if (depth_host)
        HIP_TRY(hipMemcpyAsync(depth_host, m->depth.p, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (conf_host)
        HIP_TRY(hipMemcpyAsync(conf_host, m->conf.p, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (mask_host) HIP_TRY(hipMemcpyAsync(mask_host, m->mask.p, npix, hipMemcpyDeviceToHost, ctx->stream));
    if (idx_filtered_host)
        HIP_TRY(hipMemcpyAsync(idx_filtered_host, m->idx_filtered.p, npix, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    m->depth_valid = false;  // m->depth now holds the filtered map, m->conf has (0,0) overwritten
    m->filtered_valid = true;
    return DSI_OK;
}

int dsi_mapper_get_depth_map_from_dsi(dsi_mapper_t* m, dsi_grid_t* g, const dsi_depthmap_options_t* opts,
                                      float* depth_host, float* conf_host, uint8_t* mask_host,
                                      uint8_t* idx_filtered_host)
{
    REQUIRE(m && opts, DSI_ERR_INVALID, "null argument");
    if (int rc = check_depthmap_options(opts)) return rc;
    if (!g) g = m->grid;
    if (int rc = dsi_mapper_depth_map_of(m, g)) return rc;  // collapseMaxZSlice, :368 (acquires the buffers)
    return dsi_mapper_filter_depth_map(m, opts, depth_host, conf_host, mask_host, idx_filtered_host);
}

// ---- the point cloud (mapper_emvs_stereo.cpp:440-480) ----

static int check_radius_filter_args(float radius, int min_neighbors)
{
    REQUIRE(std::isfinite(radius) && radius > 0.f, DSI_ERR_INVALID, "radius_search must be finite and > 0 (got %g)", (double)radius);
    REQUIRE(min_neighbors >= 0, DSI_ERR_INVALID, "min_num_neighbors must be >= 0 (got %d): PCL's k = 0 search is undefined",
            min_neighbors);
    return DSI_OK;
}

// keep flags of the first *n_dev of pc.pts (n_max of them at most) on `st`
static int radius_filter_device(hipStream_t st, PcBuffers& pc, const uint32_t* n_dev, size_t n_max, float radius, int min_neighbors)
{
    HIP_TRY(dsi::launch_pc_radius_filter(st, pc.pts.p, n_dev, (uint32_t)n_max, radius, (uint32_t)min_neighbors + 1u, pc.scratch(),
                                         pc.keep.p));
    return DSI_OK;
}

// The cloud of dsi_mapper_get_pointcloud in m->pc.out on the device (dsi_map_integrate_mapper reads it there):
// counts[0] points before the radius filter, counts[1] after it.  Synchronises.
static int pointcloud_device(dsi_mapper_t* m, const float* depth_host, const uint8_t* mask_host, const dsi_pointcloud_options_t* opts,
                             uint32_t counts[2])
{
    if (int rc = check_radius_filter_args(opts->radius_search, opts->min_num_neighbors)) return rc;
    REQUIRE(!depth_host == !mask_host, DSI_ERR_INVALID,
            "depth_host and mask_host must both be given, or both be NULL (the maps left on the device)");
    REQUIRE((size_t)m->geom.nz == m->planes_full.size(), DSI_ERR_INVALID,
            "a plane-sharded mapper holds no whole depth map of its own: the point cloud needs the whole arg-max");
    const int nx = m->geom.nx, ny = m->geom.ny;
    const size_t npix = (size_t)nx * ny;
    REQUIRE(npix <= ((size_t)1 << 30), DSI_ERR_INVALID, "at most 2^30 pixels");
    const bool resident = !depth_host;
    if (resident) {
        REQUIRE(m->filtered_valid, DSI_ERR_INVALID,
                "no filtered depth map on the device: call dsi_mapper_filter_depth_map or dsi_mapper_get_depth_map_from_dsi "
                "after the depth map was computed, or pass the maps");
    } else {
        for (size_t i = 0; i < npix; ++i)
            REQUIRE(!mask_host[i] || std::isfinite(depth_host[i]), DSI_ERR_INVALID,
                    "non-finite depth %g at masked pixel (%zu, %zu)", (double)depth_host[i], i % (size_t)nx, i / (size_t)nx);
    }
    dsi_context* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    if (int rc = set_device(ctx)) return rc;
    PcBuffers& pc = m->pc;
    HIP_TRY(pc.reserve(npix));
    const float* depth = m->depth.p;
    const uint8_t* mask = m->mask.p;
    if (resident) {
        if (int rc = depth_buffers_acquire(m)) return rc;
    } else {
        HIP_TRY(pc.depth.reserve(npix));
        HIP_TRY(pc.mask.reserve(npix));
        HIP_TRY(hipMemcpyAsync(pc.depth.p, depth_host, npix * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(pc.mask.p, mask_host, npix, hipMemcpyHostToDevice, st));
        depth = pc.depth.p;
        mask = pc.mask.p;
    }
    const dsi::Geom& g = m->geom;
    HIP_TRY(dsi::launch_pc_backproject(st, depth, mask, nx, ny, g.vfx, g.vfy, g.vcx, g.vcy, pc.blk.p, pc.tiles.p, pc.pts.p));
    // (the count of the back-projected points stays on the device: the filter's kernels read it, sized for every pixel)
    const uint32_t* n_dev = pc.blk.p + dsi::pc_block_words(npix) - 1;
    counts[0] = counts[1] = 0;
    HIP_TRY(hipMemcpyAsync(&counts[0], n_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (int rc = radius_filter_device(st, pc, n_dev, npix, opts->radius_search, opts->min_num_neighbors)) return rc;
    // (the compaction's block counts go to a buffer of their own: n_dev still lives in pc.blk)
    HIP_TRY(dsi::launch_pc_compact(st, pc.pts.p, pc.keep.p, (uint32_t)npix, pc.blk2.p, pc.tiles.p, pc.out.p));
    HIP_TRY(hipMemcpyAsync(&counts[1], pc.blk2.p + dsi::pc_block_words(npix) - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsi_mapper_get_pointcloud(dsi_mapper_t* m, const float* depth_host, const uint8_t* mask_host,
                              const dsi_pointcloud_options_t* opts, float* xyzi_host, size_t capacity, size_t* n_points,
                              size_t* n_unfiltered)
{
    REQUIRE(m && opts && n_points, DSI_ERR_INVALID, "null argument");
    REQUIRE(xyzi_host || capacity == 0, DSI_ERR_INVALID, "xyzi_host is null");
    uint32_t counts[2];
    if (int rc = pointcloud_device(m, depth_host, mask_host, opts, counts)) return rc;
    if (n_unfiltered) *n_unfiltered = counts[0];
    *n_points = counts[1];
    REQUIRE(capacity >= counts[1], DSI_ERR_INVALID, "capacity of %zu points is too small: %u needed", capacity, counts[1]);
    if (counts[1]) {
        hipStream_t st = m->ctx->stream;
        HIP_TRY(hipMemcpyAsync(xyzi_host, m->pc.out.p, (size_t)counts[1] * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return DSI_OK;
}

// ---- the run's pictures: accumulateEvents and the two images of saveDepthMaps ----

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

static int check_event_image_args(int width, int height, int use_polarity, const void* polarity, size_t n)
{
    REQUIRE(width >= 1 && height >= 1, DSI_ERR_INVALID, "the sensor must be at least 1 x 1 (got %d x %d)", width, height);
    REQUIRE((size_t)width * height <= ((size_t)1 << 30), DSI_ERR_INVALID, "at most 2^30 pixels");
    REQUIRE(n < ((size_t)1 << 31), DSI_ERR_INVALID, "at most 2^31-1 events (the per-pixel counters are int32)");
    REQUIRE(!use_polarity || polarity || n == 0, DSI_ERR_INVALID, "use_polarity needs the polarity bytes");
    return DSI_OK;
}

// x_dev / y_dev: the events on the device (16-byte aligned); pol_dev: n bytes (8-byte aligned; not read when use_polarity == 0);
// out_dev: 4-byte aligned
static int event_image_device(dsi_context* ctx, const uint16_t* x_dev, const uint16_t* y_dev, uint8_t* pol_dev, size_t n, int width,
                              int height, int use_polarity, uint8_t* out_dev, uint32_t* n_dropped_dev)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx->img_words.reserve(dsi::event_image_scratch_words(width, height)));
    HIP_TRY(dsi::launch_event_image(st, x_dev, y_dev, use_polarity ? pol_dev : nullptr, n, width, height, use_polarity,
                                    ctx->img_words.p, out_dev));
    if (n_dropped_dev)
        HIP_TRY(hipMemcpyAsync(n_dropped_dev, ctx->img_words.p + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return DSI_OK;
}

static int event_image_finish(dsi_context* ctx, const uint8_t* out_dev, size_t npix, uint8_t* out_host, size_t* n_dropped)
{
    uint32_t dropped = 0;
    HIP_TRY(hipMemcpyAsync(out_host, out_dev, npix, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&dropped, ctx->img_words.p + 2, sizeof dropped, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_dropped) *n_dropped = dropped;
    return DSI_OK;
}

// uploads the host events into ctx->img_bytes: x | y | polarity | `extra` bytes (256-byte aligned parts)
static int event_image_upload(dsi_context* ctx, const uint16_t* x, const uint16_t* y, const uint8_t* polarity, size_t n,
                              int use_polarity, size_t extra, uint16_t** x_dev, uint16_t** y_dev, uint8_t** pol_dev, uint8_t** extra_dev)
{
    const size_t ev = up256(std::max<size_t>(n, 1) * sizeof(uint16_t)), pb = up256(std::max<size_t>(n, 1));
    HIP_TRY(ctx->img_bytes.reserve(2 * ev + pb + extra));
    uint8_t* base = ctx->img_bytes.p;
    *x_dev = reinterpret_cast<uint16_t*>(base);
    *y_dev = reinterpret_cast<uint16_t*>(base + ev);
    *pol_dev = base + 2 * ev;
    *extra_dev = base + 2 * ev + pb;
    if (n) {
        HIP_TRY(hipMemcpyAsync(*x_dev, x, n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(*y_dev, y, n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
        if (use_polarity) HIP_TRY(hipMemcpyAsync(*pol_dev, polarity, n, hipMemcpyHostToDevice, ctx->stream));
    }
    return DSI_OK;
}

int dsi_event_image_dev(dsi_context_t* ctx, const uint16_t* x, const uint16_t* y, const uint8_t* polarity, size_t n, int width,
                        int height, int use_polarity, uint8_t* out_u8_dev, uint32_t* n_dropped_dev)
{
    REQUIRE(ctx && out_u8_dev, DSI_ERR_INVALID, "null argument");
    REQUIRE(n == 0 || (x && y), DSI_ERR_INVALID, "null event arrays");
    if (int rc = check_event_image_args(width, height, use_polarity, polarity, n)) return rc;
    REQUIRE((reinterpret_cast<uintptr_t>(out_u8_dev) & 3u) == 0, DSI_ERR_INVALID, "the device output must be 4-byte aligned");
    if (int rc = set_device(ctx)) return rc;
    uint16_t *xd, *yd;
    uint8_t *pd, *extra;
    if (int rc = event_image_upload(ctx, x, y, polarity, n, use_polarity, 0, &xd, &yd, &pd, &extra)) return rc;
    return event_image_device(ctx, xd, yd, pd, n, width, height, use_polarity, out_u8_dev, n_dropped_dev);
}

int dsi_event_image(dsi_context_t* ctx, const uint16_t* x, const uint16_t* y, const uint8_t* polarity, size_t n, int width,
                    int height, int use_polarity, uint8_t* out_u8_host, size_t* n_dropped)
{
    REQUIRE(ctx && out_u8_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(n == 0 || (x && y), DSI_ERR_INVALID, "null event arrays");
    if (int rc = check_event_image_args(width, height, use_polarity, polarity, n)) return rc;
    if (int rc = set_device(ctx)) return rc;
    const size_t npix = (size_t)width * height;
    uint16_t *xd, *yd;
    uint8_t *pd, *out;
    if (int rc = event_image_upload(ctx, x, y, polarity, n, use_polarity, npix, &xd, &yd, &pd, &out)) return rc;
    if (int rc = event_image_device(ctx, xd, yd, pd, n, width, height, use_polarity, out, nullptr)) return rc;
    return event_image_finish(ctx, out, npix, out_u8_host, n_dropped);
}

// the batch's x / y stay where they are; only the polarity bytes travel: ctx->img_bytes = polarity | `extra`
static int batch_event_image_prepare(const dsi_batch_t* batch, const uint8_t* polarity_host, int use_polarity, size_t extra,
                                     uint8_t** pol_dev, uint8_t** extra_dev)
{
    dsi_context* ctx = batch->ctx;
    const size_t n = batch->n_events, pb = up256(std::max<size_t>(n, 1));
    HIP_TRY(ctx->img_bytes.reserve(pb + extra));
    *pol_dev = ctx->img_bytes.p;
    *extra_dev = ctx->img_bytes.p + pb;
    if (batch->ready) HIP_TRY(hipStreamWaitEvent(ctx->stream, batch->ready, 0));  // uploaded on the copy stream
    if (n && use_polarity) HIP_TRY(hipMemcpyAsync(*pol_dev, polarity_host, n, hipMemcpyHostToDevice, ctx->stream));
    return DSI_OK;
}

int dsi_batch_event_image_dev(const dsi_batch_t* batch, const uint8_t* polarity_host, int width, int height, int use_polarity,
                              uint8_t* out_u8_dev, uint32_t* n_dropped_dev)
{
    REQUIRE(batch && out_u8_dev, DSI_ERR_INVALID, "null argument");
    if (int rc = check_event_image_args(width, height, use_polarity, polarity_host, batch->n_events)) return rc;
    REQUIRE((reinterpret_cast<uintptr_t>(out_u8_dev) & 3u) == 0, DSI_ERR_INVALID, "the device output must be 4-byte aligned");
    if (int rc = set_device(batch->ctx)) return rc;
    uint8_t *pd, *extra;
    if (int rc = batch_event_image_prepare(batch, polarity_host, use_polarity, 0, &pd, &extra)) return rc;
    return event_image_device(batch->ctx, batch->x, batch->y, pd, batch->n_events, width, height, use_polarity, out_u8_dev,
                              n_dropped_dev);
}

int dsi_batch_event_image(const dsi_batch_t* batch, const uint8_t* polarity_host, int width, int height, int use_polarity,
                          uint8_t* out_u8_host, size_t* n_dropped)
{
    REQUIRE(batch && out_u8_host, DSI_ERR_INVALID, "null argument");
    if (int rc = check_event_image_args(width, height, use_polarity, polarity_host, batch->n_events)) return rc;
    if (int rc = set_device(batch->ctx)) return rc;
    const size_t npix = (size_t)width * height;
    uint8_t *pd, *out;
    if (int rc = batch_event_image_prepare(batch, polarity_host, use_polarity, npix, &pd, &out)) return rc;
    if (int rc = event_image_device(batch->ctx, batch->x, batch->y, pd, batch->n_events, width, height, use_polarity, out, nullptr))
        return rc;
    return event_image_finish(batch->ctx, out, npix, out_u8_host, n_dropped);
}

static int check_depth_image_range(float min_depth, float max_depth)
{
    REQUIRE(std::isfinite(min_depth) && std::isfinite(max_depth) && min_depth > 0.f && max_depth > 0.f && min_depth != max_depth,
            DSI_ERR_INVALID, "min_depth and max_depth must be finite, > 0 and different (got %g, %g)", (double)min_depth,
            (double)max_depth);
    return DSI_OK;
}

// ctx->img_bytes: colour table (1 KiB) | `inputs` bytes for the caller | conf_negated | inv_depth_bgr; runs both kernels on the
// device maps given and brings the images home
static int depth_images_run(dsi_context* ctx, const float* host_maps_depth, const float* host_maps_conf, const uint8_t* host_maps_mask,
                            const float* depth_dev, const float* conf_dev, const uint8_t* mask_dev, int rows, int cols,
                            float min_depth, float max_depth, const uint8_t* lut_bgr, uint8_t* conf_negated_host,
                            uint8_t* inv_depth_bgr_host)
{
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)rows * cols;
    const bool upload = host_maps_depth || host_maps_conf || host_maps_mask;
    const size_t fb = up256(npix * sizeof(float)), mb = up256(npix);
    const size_t inputs = upload ? 2 * fb + mb : 0;
    HIP_TRY(ctx->img_bytes.reserve(1024 + inputs + mb + up256(3 * npix)));
    HIP_TRY(ctx->img_words.reserve(dsi::kEventImageHeadWords));
    uint8_t* base = ctx->img_bytes.p;
    uint8_t* lut_dev = base;
    uint8_t* neg_dev = base + 1024 + inputs;
    uint8_t* bgr_dev = neg_dev + mb;
    if (upload) {
        float* d = reinterpret_cast<float*>(base + 1024);
        float* c = reinterpret_cast<float*>(base + 1024 + fb);
        uint8_t* m = base + 1024 + 2 * fb;
        if (inv_depth_bgr_host) {
            HIP_TRY(hipMemcpyAsync(d, host_maps_depth, npix * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(m, host_maps_mask, npix, hipMemcpyHostToDevice, st));
        }
        if (conf_negated_host) HIP_TRY(hipMemcpyAsync(c, host_maps_conf, npix * sizeof(float), hipMemcpyHostToDevice, st));
        depth_dev = d;
        conf_dev = c;
        mask_dev = m;
    }
    uint8_t jet[768];
    if (inv_depth_bgr_host) {
        if (!lut_bgr) {
            dsi::default_jet_lut(jet);
            lut_bgr = jet;
        }
        HIP_TRY(hipMemcpyAsync(lut_dev, lut_bgr, 768, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(dsi::launch_depth_images(st, depth_dev, conf_dev, mask_dev, rows, cols, min_depth, max_depth, lut_dev, ctx->img_words.p,
                                     conf_negated_host ? neg_dev : nullptr, inv_depth_bgr_host ? bgr_dev : nullptr));
    if (conf_negated_host) HIP_TRY(hipMemcpyAsync(conf_negated_host, neg_dev, npix, hipMemcpyDeviceToHost, st));
    if (inv_depth_bgr_host) HIP_TRY(hipMemcpyAsync(inv_depth_bgr_host, bgr_dev, 3 * npix, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (also: `jet` and the caller's arrays are free again)
    return DSI_OK;
}

int dsi_default_jet_lut(uint8_t* lut_bgr)
{
    REQUIRE(lut_bgr, DSI_ERR_INVALID, "null argument");
    dsi::default_jet_lut(lut_bgr);
    return DSI_OK;
}

int dsi_depth_images(dsi_context_t* ctx, const float* depth_host, const float* conf_host, const uint8_t* mask_host, int rows,
                     int cols, float min_depth, float max_depth, const uint8_t* lut_bgr, uint8_t* conf_negated_host,
                     uint8_t* inv_depth_bgr_host)
{
    REQUIRE(ctx, DSI_ERR_INVALID, "null argument");
    REQUIRE(rows >= 1 && cols >= 1, DSI_ERR_INVALID, "the maps must be at least 1 x 1 (got %d x %d)", rows, cols);
    REQUIRE((size_t)rows * cols <= ((size_t)1 << 29), DSI_ERR_INVALID, "at most 2^29 pixels");
    REQUIRE(!conf_negated_host || conf_host, DSI_ERR_INVALID, "the negated confidence image needs conf_host");
    REQUIRE(!inv_depth_bgr_host || (depth_host && mask_host), DSI_ERR_INVALID,
            "the inverse-depth image needs depth_host and mask_host");
    if (inv_depth_bgr_host)
        if (int rc = check_depth_image_range(min_depth, max_depth)) return rc;
    if (!conf_negated_host && !inv_depth_bgr_host) return DSI_OK;
    if (int rc = set_device(ctx)) return rc;
    return depth_images_run(ctx, depth_host, conf_host, mask_host, nullptr, nullptr, nullptr, rows, cols, min_depth, max_depth,
                            lut_bgr, conf_negated_host, inv_depth_bgr_host);
}

int dsi_mapper_depth_images(dsi_mapper_t* m, float min_depth, float max_depth, const uint8_t* lut_bgr, uint8_t* conf_negated_host,
                            uint8_t* inv_depth_bgr_host)
{
    REQUIRE(m, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->filtered_valid, DSI_ERR_INVALID,
            "no filtered depth map on the device: call dsi_mapper_filter_depth_map or dsi_mapper_get_depth_map_from_dsi "
            "after the depth map was computed, or pass the maps to dsi_depth_images");
    if (inv_depth_bgr_host)
        if (int rc = check_depth_image_range(min_depth, max_depth)) return rc;
    if (!conf_negated_host && !inv_depth_bgr_host) return DSI_OK;
    if (int rc = set_device(m->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    // m->conf is the confidence map as the filter call returned it: element (0,0) = max_confidence, nothing else touched
    return depth_images_run(m->ctx, nullptr, nullptr, nullptr, m->depth.p, m->conf.p, m->mask.p, m->geom.ny, m->geom.nx, min_depth,
                            max_depth, lut_bgr, conf_negated_host, inv_depth_bgr_host);
}

// ---- depth-map scores against ground truth ----

struct dsi_score {
    dsi_context* ctx = nullptr;
    size_t capacity = 0;
    double baseline = 0.0, focal = 0.0, gt_min = 0.0;
    DevBuf<double> buf;  // capacity errors, then kScoreGuardWords words that nothing may touch
    // state | extremes (2) | select work area
    DevBuf<unsigned long long> words;
    DevBuf<double> partials;  // 4 * kScoreMaxBlocks
    DevBuf<float> depth, gt;     // uploaded maps
    DevBuf<uint8_t> mask;
    DevBuf<unsigned long long> counts;
};

namespace {

constexpr size_t kScoreGuardWords = 64;
constexpr unsigned long long kScoreGuardPattern = 0xa5c3a5c3a5c3a5c3ull;
constexpr size_t kScoreStateWords = sizeof(dsi::ScoreState) / sizeof(unsigned long long);
static_assert(sizeof(dsi::ScoreState) % sizeof(unsigned long long) == 0, "ScoreState is made of 64-bit words");

dsi::ScoreState* score_state(dsi_score* s) { return reinterpret_cast<dsi::ScoreState*>(s->words.p); }
unsigned long long* score_mm(dsi_score* s) { return s->words.p + kScoreStateWords; }
unsigned long long* score_select_words(dsi_score* s) { return s->words.p + kScoreStateWords + 2; }

int score_add_device(dsi_score* s, const float* depth_dev, const uint8_t* mask_dev, const float* gt_dev, size_t n)
{
    HIP_TRY(dsi::launch_score_accumulate(s->ctx->stream, depth_dev, mask_dev, gt_dev, n, s->gt_min, s->baseline, s->focal,
                                         score_state(s), s->buf.p, s->capacity, s->partials.p));
    return DSI_OK;
}

int score_check_add(const dsi_score* s, const void* a, const void* b, const void* c, size_t n)
{
    REQUIRE(s && a && b && c, DSI_ERR_INVALID, "null argument");
    REQUIRE(n >= 1 && n <= ((size_t)1 << 40), DSI_ERR_INVALID, "a map holds 1 .. 2^40 pixels (got %zu)", n);
    return DSI_OK;
}

// the state as it stands once the stream has run; synchronises
int score_read_state(dsi_score* s, dsi::ScoreState* st, size_t* n_stored)
{
    HIP_TRY(hipMemcpyAsync(st, s->words.p, sizeof *st, hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    *n_stored = (size_t)std::min<unsigned long long>(st->cursor, s->capacity);
    return DSI_OK;
}

// np.ma.median of the n stored errors; synchronises
int score_median_of(dsi_score* s, size_t n, double* out)
{
    unsigned long long mid[2] = {0, 0};
    unsigned long long* work = score_select_words(s);
    HIP_TRY(dsi::launch_score_select(s->ctx->stream, s->buf.p, n, (n - 1) / 2, n / 2, work));
    HIP_TRY(hipMemcpyAsync(mid, work, sizeof mid, hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    double lo, hi;
    std::memcpy(&lo, &mid[0], sizeof lo);
    std::memcpy(&hi, &mid[1], sizeof hi);
    *out = (n & 1) ? lo : (lo + hi) / 2.0;  // numpy: mid.sum() / 2 of the two middle elements
    return DSI_OK;
}

}  // namespace

int dsi_score_create(dsi_context_t* ctx, size_t capacity_points, double baseline, double focal, double gt_min, dsi_score_t** out)
{
    REQUIRE(ctx && out, DSI_ERR_INVALID, "null argument");
    REQUIRE(capacity_points >= 1 && capacity_points <= ((size_t)1 << 40), DSI_ERR_INVALID,
            "capacity_points must be in 1 .. 2^40 (got %zu)", capacity_points);
    REQUIRE(std::isfinite(baseline) && baseline > 0.0 && std::isfinite(focal) && focal > 0.0, DSI_ERR_INVALID,
            "baseline and focal must be finite and > 0 (got %g, %g)", baseline, focal);
    REQUIRE(std::isfinite(gt_min) && gt_min > 0.0, DSI_ERR_INVALID, "gt_min must be finite and > 0 (got %g)", gt_min);
    if (int rc = set_device(ctx)) return rc;
    dsi_score* s = new (std::nothrow) dsi_score;
    REQUIRE(s, DSI_ERR_INVALID, "out of host memory");
    s->ctx = ctx;
    s->capacity = capacity_points;
    s->baseline = baseline;
    s->focal = focal;
    s->gt_min = gt_min;
    const size_t nwords = kScoreStateWords + 2 + dsi::kScoreSelectWords;
    std::vector<unsigned long long> guard(kScoreGuardWords, kScoreGuardPattern);
    hipError_t e = s->buf.reserve(capacity_points + kScoreGuardWords);
    if (e == hipSuccess) e = s->words.reserve(nwords);
    if (e == hipSuccess) e = s->partials.reserve(4 * (size_t)dsi::kScoreMaxBlocks);
    if (e == hipSuccess) e = hipMemsetAsync(s->words.p, 0, nwords * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->buf.p + capacity_points, guard.data(), kScoreGuardWords * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (`guard` is free again)
    if (e != hipSuccess) {
        delete s;
        return fail(DSI_ERR_HIP, "score allocation of %zu points failed: %s", capacity_points, hipGetErrorString(e));
    }
    ++ctx->children;
    *out = s;
    return DSI_OK;
}

int dsi_score_destroy(dsi_score_t* s)
{
    if (!s) return DSI_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    --s->ctx->children;
    delete s;
    return DSI_OK;
}

int dsi_score_reset(dsi_score_t* s)
{
    REQUIRE(s, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(s->ctx)) return rc;
    HIP_TRY(hipMemsetAsync(s->words.p, 0, kScoreStateWords * sizeof(unsigned long long), s->ctx->stream));
    return DSI_OK;
}

int dsi_score_add(dsi_score_t* s, const float* depth_host, const uint8_t* mask_host, const float* gt_host, size_t n_pixels)
{
    if (int rc = score_check_add(s, depth_host, mask_host, gt_host, n_pixels)) return rc;
    if (int rc = set_device(s->ctx)) return rc;
    hipStream_t st = s->ctx->stream;
    HIP_TRY(s->depth.reserve(n_pixels));
    HIP_TRY(s->gt.reserve(n_pixels));
    HIP_TRY(s->mask.reserve(n_pixels));
    HIP_TRY(hipMemcpyAsync(s->depth.p, depth_host, n_pixels * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->mask.p, mask_host, n_pixels, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->gt.p, gt_host, n_pixels * sizeof(float), hipMemcpyHostToDevice, st));
    return score_add_device(s, s->depth.p, s->mask.p, s->gt.p, n_pixels);
}

int dsi_score_add_dev(dsi_score_t* s, const float* depth_dev, const uint8_t* mask_dev, const float* gt_dev, size_t n_pixels)
{
    if (int rc = score_check_add(s, depth_dev, mask_dev, gt_dev, n_pixels)) return rc;
    if (int rc = set_device(s->ctx)) return rc;
    return score_add_device(s, depth_dev, mask_dev, gt_dev, n_pixels);
}

int dsi_score_add_mapper(dsi_score_t* s, dsi_mapper_t* m, const float* gt_host)
{
    REQUIRE(s && m && gt_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx == s->ctx, DSI_ERR_CONTEXT, "mapper and score belong to different contexts");
    REQUIRE(m->filtered_valid, DSI_ERR_INVALID,
            "no filtered depth map on the device: call dsi_mapper_filter_depth_map or dsi_mapper_get_depth_map_from_dsi "
            "after the depth map was computed, or pass the maps to dsi_score_add");
    if (int rc = set_device(s->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    HIP_TRY(s->gt.reserve(npix));
    HIP_TRY(hipMemcpyAsync(s->gt.p, gt_host, npix * sizeof(float), hipMemcpyHostToDevice, s->ctx->stream));
    return score_add_device(s, m->depth.p, m->mask.p, s->gt.p, npix);
}

int dsi_score_median(dsi_score_t* s, double* median_abs)
{
    REQUIRE(s && median_abs, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(s->ctx)) return rc;
    dsi::ScoreState st;
    size_t n = 0;
    if (int rc = score_read_state(s, &st, &n)) return rc;
    REQUIRE(!st.overflow && st.cursor <= s->capacity, DSI_ERR_INVALID,
            "the error buffer overflowed (%llu joint pixels, capacity %zu): the median needs every error", st.cursor, s->capacity);
    *median_abs = std::nan("");
    if (n == 0) return DSI_OK;
    return score_median_of(s, n, median_abs);
}

int dsi_score_metrics(dsi_score_t* s, dsi_score_metrics_t* out)
{
    REQUIRE(s && out, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(s->ctx)) return rc;
    dsi::ScoreState st;
    size_t n_stored = 0;
    unsigned long long guard[kScoreGuardWords];
    HIP_TRY(hipMemcpyAsync(guard, s->buf.p + s->capacity, sizeof guard, hipMemcpyDeviceToHost, s->ctx->stream));
    if (int rc = score_read_state(s, &st, &n_stored)) return rc;
    dsi_score_metrics_t r{};
    r.n_est = st.count[0];
    r.n_gt = st.count[1];
    r.n_joint = st.count[2];
    for (int k = 0; k < 3; ++k) r.n_delta[k] = st.count[3 + k];
    r.n_bad = st.count[6];
    r.n_stored = n_stored;
    r.overflow = (st.overflow || st.cursor > s->capacity) ? 1 : 0;
    r.guard_intact = 1;
    for (size_t i = 0; i < kScoreGuardWords; ++i)
        if (guard[i] != kScoreGuardPattern) r.guard_intact = 0;
    r.sum_di = st.sum[0];
    r.sum_di2 = st.sum[1];
    r.sum_are = st.sum[2];
    r.sum_abs = st.sum[3];
    const double nan = std::nan("");
    r.max_gt = nan;
    if (st.max_gt_key) std::memcpy(&r.max_gt, &st.max_gt_key, sizeof r.max_gt);
    r.delta[0] = r.delta[1] = r.delta[2] = r.silog = r.are = r.lrmse = r.badp = r.mean_abs = r.median_abs = nan;
    if (r.n_joint) {
        const double n = (double)r.n_joint;
        for (int k = 0; k < 3; ++k) r.delta[k] = (double)r.n_delta[k] / n;                    // depth_metrics.py:10-12
        r.silog = 1.0 / n * r.sum_di2 - 1.0 / (n * n) * (r.sum_di * r.sum_di);                // :17
        r.are = 1.0 / n * r.sum_are;                                                          // :20
        r.lrmse = std::sqrt(1.0 / n * r.sum_di2);                                             // :23
        r.badp = (double)r.n_bad / n;                                                         // :28
        r.mean_abs = r.sum_abs / n;                                                           // np.ma.mean
        if (!r.overflow)
            if (int rc = score_median_of(s, n_stored, &r.median_abs)) return rc;
    }
    *out = r;
    return DSI_OK;
}

int dsi_score_histogram(dsi_score_t* s, double binwidth, uint64_t* counts, size_t cap, size_t* n_bins, double* first_edge,
                        double* last_edge)
{
    REQUIRE(s && n_bins && first_edge && last_edge, DSI_ERR_INVALID, "null argument");
    REQUIRE(std::isfinite(binwidth) && binwidth > 0.0, DSI_ERR_INVALID, "binwidth must be finite and > 0 (got %g)", binwidth);
    if (int rc = set_device(s->ctx)) return rc;
    hipStream_t stream = s->ctx->stream;
    dsi::ScoreState st;
    size_t n = 0;
    if (int rc = score_read_state(s, &st, &n)) return rc;
    REQUIRE(!st.overflow && st.cursor <= s->capacity, DSI_ERR_INVALID,
            "the error buffer overflowed (%llu joint pixels, capacity %zu): the histogram needs every error", st.cursor,
            s->capacity);
    *n_bins = 0;
    *first_edge = *last_edge = std::nan("");
    if (n == 0) return DSI_OK;
    unsigned long long mm[2];
    HIP_TRY(dsi::launch_score_minmax(stream, s->buf.p, n, score_mm(s)));
    HIP_TRY(hipMemcpyAsync(mm, score_mm(s), sizeof mm, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    double lo, hi;
    std::memcpy(&lo, &mm[0], sizeof lo);
    std::memcpy(&hi, &mm[1], sizeof hi);
    const double fbins = hi / binwidth;  // bins = int(np.amax(err) / binwidth)
    REQUIRE(fbins < (double)dsi::kScoreMaxBins + 1.0, DSI_ERR_INVALID, "max(err) / binwidth = %g: more than 2^24 bins", fbins);
    const long long nb = (long long)fbins;
    REQUIRE(nb <= dsi::kScoreMaxBins, DSI_ERR_INVALID, "more than 2^24 bins");
    if (nb < 1) return DSI_OK;  // (numpy raises "`bins` must be positive")
    dsi::ScoreBins B{};
    B.first = lo;
    B.last = hi;
    if (lo == hi) {  // _get_outer_edges
        B.first = lo - 0.5;
        B.last = hi + 0.5;
    }
    B.delta = B.last - B.first;
    B.nb = nb;
    B.step = B.delta / (double)nb;
    B.step_zero = B.step == 0.0;
    *n_bins = (size_t)nb;
    *first_edge = B.first;
    *last_edge = B.last;
    if (!counts) return DSI_OK;
    REQUIRE(cap >= (size_t)nb, DSI_ERR_INVALID, "counts holds %zu bins, the histogram has %lld", cap, nb);
    HIP_TRY(s->counts.reserve((size_t)nb));
    HIP_TRY(dsi::launch_score_histogram(stream, s->buf.p, n, B, s->counts.p));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "64-bit counts");
    HIP_TRY(hipMemcpyAsync(counts, s->counts.p, (size_t)nb * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DSI_OK;
}

// ---- ground-truth depth from disparity images ----

struct dsi_gt {
    dsi_context* ctx = nullptr;
    int width = 0, height = 0, mode = 0;
    dsi::GtCalib calib{};
    // winner table | output map | disparity upload (4 bytes per pixel each), counters
    DevBuf<uint32_t> words;
    DevBuf<unsigned int> counters;
};

namespace {

size_t gt_npix(const dsi_gt* g) { return (size_t)g->width * g->height; }
float* gt_out(const dsi_gt* g) { return reinterpret_cast<float*>(g->words.p + gt_npix(g)); }
void* gt_upload(const dsi_gt* g) { return g->words.p + 2 * gt_npix(g); }

dsi::GtWork gt_work(const dsi_gt* g) { return dsi::GtWork{g->words.p, g->counters.p, gt_out(g)}; }

}  // namespace

int dsi_gt_create(dsi_context_t* ctx, int width, int height, const double* Q, const double* T, const double* K, int mode,
                  dsi_gt_t** out)
{
    REQUIRE(ctx && Q && T && K && out, DSI_ERR_INVALID, "null argument");
    REQUIRE(width >= 1 && height >= 1, DSI_ERR_INVALID, "the image must be at least 1 x 1 (got %d x %d)", width, height);
    REQUIRE((unsigned long long)width * (unsigned long long)height < 0xffffffffull, DSI_ERR_INVALID,
            "width * height must be below 2^32 - 1 (got %d x %d)", width, height);
    REQUIRE(mode == DSI_GT_AS_SCRIPT || mode == DSI_GT_DROP_OUTSIDE, DSI_ERR_INVALID, "unknown mode %d", mode);
    for (int i = 0; i < 16; ++i)
        REQUIRE(std::isfinite(Q[i]) && std::isfinite(T[i]), DSI_ERR_INVALID, "Q and T must be finite (entry %d)", i);
    for (int i = 0; i < 12; ++i) REQUIRE(std::isfinite(K[i]), DSI_ERR_INVALID, "K must be finite (entry %d)", i);
    if (int rc = set_device(ctx)) return rc;
    dsi_gt* g = new (std::nothrow) dsi_gt;
    REQUIRE(g, DSI_ERR_INVALID, "out of host memory");
    g->ctx = ctx;
    g->width = width;
    g->height = height;
    g->mode = mode;
    std::memcpy(g->calib.Q, Q, sizeof g->calib.Q);
    std::memcpy(g->calib.T, T, sizeof g->calib.T);
    std::memcpy(g->calib.K, K, sizeof g->calib.K);
    const size_t n = gt_npix(g);
    hipError_t e = g->words.reserve(3 * n);
    if (e == hipSuccess) e = g->counters.reserve(2);
    if (e == hipSuccess) e = hipMemsetAsync(g->words.p, 0, 2 * n * sizeof(uint32_t), ctx->stream);  // (a fetch before a projection)
    if (e == hipSuccess) e = hipMemsetAsync(g->counters.p, 0, 2 * sizeof(unsigned int), ctx->stream);
    if (e != hipSuccess) {
        delete g;
        return fail(DSI_ERR_HIP, "projector allocation of %d x %d pixels failed: %s", width, height, hipGetErrorString(e));
    }
    ++ctx->children;
    *out = g;
    return DSI_OK;
}

int dsi_gt_destroy(dsi_gt_t* gt)
{
    if (!gt) return DSI_OK;
    (void)hipSetDevice(gt->ctx->device);
    (void)hipStreamSynchronize(gt->ctx->stream);
    --gt->ctx->children;
    delete gt;
    return DSI_OK;
}

int dsi_gt_project(dsi_gt_t* gt, const float* disp_f32_host)
{
    REQUIRE(gt && disp_f32_host, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(gt->ctx)) return rc;
    float* up = static_cast<float*>(gt_upload(gt));
    HIP_TRY(hipMemcpyAsync(up, disp_f32_host, gt_npix(gt) * sizeof(float), hipMemcpyHostToDevice, gt->ctx->stream));
    HIP_TRY(dsi::launch_gt_project(gt->ctx->stream, up, gt->calib, gt->width, gt->height, gt->mode, gt_work(gt)));
    return DSI_OK;
}

int dsi_gt_project_u16(dsi_gt_t* gt, const uint16_t* raw_u16_host)
{
    REQUIRE(gt && raw_u16_host, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(gt->ctx)) return rc;
    uint16_t* up = static_cast<uint16_t*>(gt_upload(gt));
    HIP_TRY(hipMemcpyAsync(up, raw_u16_host, gt_npix(gt) * sizeof(uint16_t), hipMemcpyHostToDevice, gt->ctx->stream));
    HIP_TRY(dsi::launch_gt_project_u16(gt->ctx->stream, up, gt->calib, gt->width, gt->height, gt->mode, gt_work(gt)));
    return DSI_OK;
}

int dsi_gt_fetch(dsi_gt_t* gt, float* depth_host, uint64_t* n_points, uint64_t* n_outside)
{
    REQUIRE(gt, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(gt->ctx)) return rc;
    unsigned int counters[2] = {0, 0};
    hipStream_t st = gt->ctx->stream;
    if (depth_host) HIP_TRY(hipMemcpyAsync(depth_host, gt_out(gt), gt_npix(gt) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counters, gt->counters.p, sizeof counters, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_points) *n_points = counters[0];
    if (n_outside) *n_outside = counters[1];
    return DSI_OK;
}

float* dsi_gt_device_ptr(dsi_gt_t* gt) { return gt ? gt_out(gt) : nullptr; }

int dsi_score_add_gt(dsi_score_t* s, const float* depth_host, const uint8_t* mask_host, size_t n_pixels, dsi_gt_t* gt)
{
    if (int rc = score_check_add(s, depth_host, mask_host, gt, n_pixels)) return rc;
    REQUIRE(gt->ctx == s->ctx, DSI_ERR_CONTEXT, "projector and score belong to different contexts");
    REQUIRE(n_pixels == gt_npix(gt), DSI_ERR_INVALID, "the maps hold %zu pixels, the projector's %d x %d", n_pixels, gt->width,
            gt->height);
    if (int rc = set_device(s->ctx)) return rc;
    hipStream_t st = s->ctx->stream;
    HIP_TRY(s->depth.reserve(n_pixels));
    HIP_TRY(s->mask.reserve(n_pixels));
    HIP_TRY(hipMemcpyAsync(s->depth.p, depth_host, n_pixels * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->mask.p, mask_host, n_pixels, hipMemcpyHostToDevice, st));
    return score_add_device(s, s->depth.p, s->mask.p, gt_out(gt), n_pixels);
}

int dsi_score_add_mapper_gt(dsi_score_t* s, dsi_mapper_t* m, dsi_gt_t* gt)
{
    REQUIRE(s && m && gt, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx == s->ctx, DSI_ERR_CONTEXT, "mapper and score belong to different contexts");
    REQUIRE(gt->ctx == s->ctx, DSI_ERR_CONTEXT, "projector and score belong to different contexts");
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    REQUIRE(npix == gt_npix(gt), DSI_ERR_INVALID, "the mapper's maps hold %zu pixels, the projector's %d x %d", npix, gt->width,
            gt->height);
    REQUIRE(m->filtered_valid, DSI_ERR_INVALID,
            "no filtered depth map on the device: call dsi_mapper_filter_depth_map or dsi_mapper_get_depth_map_from_dsi "
            "after the depth map was computed, or pass the maps to dsi_score_add_gt");
    if (int rc = set_device(s->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    return score_add_device(s, m->depth.p, m->mask.p, gt_out(gt), npix);
}

int dsi_depth_erode(dsi_context_t* ctx, const float* depth_host, const uint8_t* mask_host, int rows, int cols, float no_estimate,
                    float* out_depth_host, uint8_t* out_mask_host)
{
    REQUIRE(ctx && depth_host && mask_host && out_depth_host && out_mask_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(rows >= 1 && cols >= 1, DSI_ERR_INVALID, "the maps must be at least 1 x 1 (got %d x %d)", rows, cols);
    REQUIRE((size_t)rows * cols <= ((size_t)1 << 29), DSI_ERR_INVALID, "at most 2^29 pixels");
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)rows * cols;
    const size_t fb = up256(npix * sizeof(float)), mb = up256(npix);
    HIP_TRY(ctx->img_bytes.reserve(2 * fb + 2 * mb));
    float* d_in = reinterpret_cast<float*>(ctx->img_bytes.p);
    float* d_out = reinterpret_cast<float*>(ctx->img_bytes.p + fb);
    uint8_t* m_in = ctx->img_bytes.p + 2 * fb;
    uint8_t* m_out = m_in + mb;
    HIP_TRY(hipMemcpyAsync(d_in, depth_host, npix * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m_in, mask_host, npix, hipMemcpyHostToDevice, st));
    HIP_TRY(dsi::launch_depth_erode_cross(st, d_in, m_in, rows, cols, no_estimate, d_out, m_out));
    HIP_TRY(hipMemcpyAsync(out_depth_host, d_out, npix * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_mask_host, m_out, npix, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

// ---- lens rectification table ----

int dsi_lens_check(const dsi_lens_t* lens)
{
    REQUIRE(lens, DSI_ERR_INVALID, "null argument");
    REQUIRE(lens->model == DSI_LENS_PLUMB_BOB || lens->model == DSI_LENS_FISHEYE, DSI_ERR_INVALID,
            "unknown lens model %d (DSI_LENS_PLUMB_BOB 0, DSI_LENS_FISHEYE 1)", lens->model);
    const int n = lens->n_dist;
    if (lens->model == DSI_LENS_PLUMB_BOB)
        REQUIRE(n == 0 || n == 4 || n == 5 || n == 8, DSI_ERR_INVALID,
                "plumb_bob takes 0, 4, 5 or 8 distortion coefficients (got %d; thin-prism and tilt terms are not supported)", n);
    else
        REQUIRE(n == 4, DSI_ERR_INVALID, "fisheye takes 4 distortion coefficients (got %d)", n);
    for (int i = 0; i < 9; ++i)
        REQUIRE(std::isfinite(lens->K[i]) && std::isfinite(lens->R[i]), DSI_ERR_INVALID, "K and R must be finite (entry %d)", i);
    for (int i = 0; i < n; ++i) REQUIRE(std::isfinite(lens->D[i]), DSI_ERR_INVALID, "D must be finite (entry %d)", i);
    for (int i = 0; i < 12; ++i) REQUIRE(std::isfinite(lens->P[i]), DSI_ERR_INVALID, "P must be finite (entry %d)", i);
    REQUIRE(lens->K[0] != 0.0 && lens->K[4] != 0.0, DSI_ERR_INVALID, "fx = K[0] and fy = K[4] must not be 0");
    return DSI_OK;
}

int dsi_lens_rr(const dsi_lens_t* lens, double RR[9])
{
    REQUIRE(lens && RR, DSI_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = s + lens->P[4 * i + k] * lens->R[3 * k + j];
            RR[3 * i + j] = s;
        }
    return DSI_OK;
}

namespace {

int lens_coef(const dsi_lens_t* lens, dsi::LensCoef* c)
{
    if (int rc = dsi_lens_check(lens)) return rc;
    *c = dsi::LensCoef{};
    c->fx = lens->K[0];
    c->fy = lens->K[4];
    c->cx = lens->K[2];
    c->cy = lens->K[5];
    for (int i = 0; i < lens->n_dist; ++i) c->k[i] = lens->D[i];
    return dsi_lens_rr(lens, c->RR);
}

int lens_size_check(int width, int height)
{
    REQUIRE(width >= 1 && height >= 1, DSI_ERR_INVALID, "the table must be at least 1 x 1 (got %d x %d)", width, height);
    REQUIRE(width <= 65536 && height <= 65536, DSI_ERR_INVALID, "event coordinates are u16 (got %d x %d)", width, height);
    REQUIRE((unsigned long long)width * (unsigned long long)height < 0xffffffffull, DSI_ERR_INVALID,
            "width * height must be below 2^32 - 1 (got %d x %d)", width, height);
    return DSI_OK;
}

}  // namespace

int dsi_rectify_lut_dev(dsi_context_t* ctx, const dsi_lens_t* lens, int width, int height, float* lut_dev)
{
    REQUIRE(ctx && lens && lut_dev, DSI_ERR_INVALID, "null argument");
    REQUIRE(((uintptr_t)lut_dev & 7u) == 0, DSI_ERR_INVALID, "the table must be 8-byte aligned");
    dsi::LensCoef c;
    if (int rc = lens_coef(lens, &c)) return rc;
    if (int rc = lens_size_check(width, height)) return rc;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(dsi::launch_rectify_lut(ctx->stream, lens->model, c, width, height, reinterpret_cast<float2*>(lut_dev)));
    return DSI_OK;
}

int dsi_rectify_lut(dsi_context_t* ctx, const dsi_lens_t* lens, int width, int height, float* lut_host)
{
    REQUIRE(ctx && lens && lut_host, DSI_ERR_INVALID, "null argument");
    if (int rc = dsi_lens_check(lens)) return rc;
    if (int rc = lens_size_check(width, height)) return rc;
    if (int rc = set_device(ctx)) return rc;
    const size_t bytes = (size_t)width * height * sizeof(float2);
    HIP_TRY(ctx->img_bytes.reserve(bytes));
    float* dev = reinterpret_cast<float*>(ctx->img_bytes.p);
    if (int rc = dsi_rectify_lut_dev(ctx, lens, width, height, dev)) return rc;
    HIP_TRY(hipMemcpyAsync(lut_host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DSI_OK;
}

int dsi_mapper_create_with_lens(dsi_context_t* ctx, const dsi_mapper_config_t* cfg, const dsi_lens_t* lens, dsi_mapper_t** out)
{
    REQUIRE(ctx && cfg && lens && out, DSI_ERR_INVALID, "null argument");
    *out = nullptr;
    REQUIRE(!cfg->lut, DSI_ERR_INVALID, "a table (cfg->lut) and a lens exclude each other");
    dsi::LensCoef c;
    if (int rc = lens_coef(lens, &c)) return rc;
    if (int rc = lens_size_check(cfg->sensor_width, cfg->sensor_height)) return rc;
    dsi_mapper* m = nullptr;
    if (int rc = dsi_mapper_create(ctx, cfg, &m)) return rc;
    // the table goes straight into the mapper's own buffer; the wait makes it visible to every stream that will read it
    // (the mapper's preparation stream does not follow the context's) and brings a failed launch back from here
    hipError_t e = m->lut_dev.reserve((size_t)cfg->sensor_width * cfg->sensor_height);
    if (e == hipSuccess) e = dsi::launch_rectify_lut(ctx->stream, lens->model, c, cfg->sensor_width, cfg->sensor_height, m->lut_dev.p);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        dsi_mapper_destroy(m);  // (a whole mapper by now: its grid is a child of its own)
        return fail(DSI_ERR_HIP, "mapper lens table failed: %s", hipGetErrorString(e));
    }
    *out = m;
    return DSI_OK;
}

int dsi_radius_outlier_removal(dsi_context_t* ctx, const float* xyz_host, size_t stride_floats, size_t n, float radius,
                               int min_neighbors, uint8_t* keep_host)
{
    REQUIRE(ctx, DSI_ERR_INVALID, "ctx is null");
    REQUIRE(stride_floats == 3 || stride_floats == 4, DSI_ERR_INVALID, "stride_floats must be 3 or 4 (got %zu)", stride_floats);
    if (int rc = check_radius_filter_args(radius, min_neighbors)) return rc;
    REQUIRE(n == 0 || (xyz_host && keep_host), DSI_ERR_INVALID, "null array");
    REQUIRE(n <= ((size_t)1 << 30), DSI_ERR_INVALID, "at most 2^30 points");
    if (n == 0) return DSI_OK;
    if ((size_t)min_neighbors + 1 > n) {  // fewer points than a neighbourhood needs: everything is removed
        std::memset(keep_host, 0, n);
        return DSI_OK;
    }
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    PcBuffers& pc = ctx->pc;
    HIP_TRY(pc.reserve(n));
    const uint32_t n32 = (uint32_t)n;
    if (stride_floats == 4) {
        HIP_TRY(hipMemcpyAsync(pc.pts.p, xyz_host, n * sizeof(float4), hipMemcpyHostToDevice, st));
    } else {
        std::vector<float4> packed(n);
        for (size_t i = 0; i < n; ++i) packed[i] = make_float4(xyz_host[3 * i], xyz_host[3 * i + 1], xyz_host[3 * i + 2], 0.f);
        HIP_TRY(hipMemcpyAsync(pc.pts.p, packed.data(), n * sizeof(float4), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // (packed is pageable and goes out of scope)
    }
    HIP_TRY(hipMemcpyAsync(pc.n.p, &n32, sizeof n32, hipMemcpyHostToDevice, st));
    if (int rc = radius_filter_device(st, pc, pc.n.p, n, radius, min_neighbors)) return rc;
    HIP_TRY(hipMemcpyAsync(keep_host, pc.keep.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

// ---- the world map (include/dsi_engine.h "the world map") ----

struct dsi_map {
    dsi_context* ctx = nullptr;
    double leaf = 0.0;
    uint32_t cap_log2 = 0;
    DevBuf<unsigned char> block;         // the table (dsi::map_table_at)
    DevBuf<unsigned long long> ctr;      // device: occupied, accepted, rejected, table-full
    unsigned long long host_ctr[4] = {0, 0, 0, 0};  // as read back by the last integrate call
    uint64_t calls = 0, growths = 0;
    DevBuf<float> upload, xyz;           // a call's host points; the extraction's outputs
    DevBuf<uint32_t> blk, tiles, n_out, w_out;
    DevBuf<unsigned long long> key_out;
    // the last render (dsi_map_render): valid until the map changes
    DevBuf<unsigned long long> zkey, render_ctr;
    DevBuf<uint32_t> hits, render_windows;
    DevBuf<float> render_depth;
    DevBuf<uint8_t> render_mask;
    int render_width = 0, render_height = 0;
    bool render_valid = false;
    // the last compare with this map as the first (dsx_map_compare, include/dsi_map_eval.h): valid until the map changes
    DevBuf<uint8_t> depth_mask;          // dsx_map_integrate_depth's mask upload
    DevBuf<float> cmp_dist, cmp_dist_out;  // per slot; compacted for a fetch
    DevBuf<unsigned long long> cmp_hist, cmp_ctr;
    uint32_t cmp_min_points = 0, cmp_min_windows = 0;
    bool compare_valid = false;
    // the last classification (dsx_map_prune_classify, include/dsi_map_prune.h): valid until the map changes
    DevBuf<uint8_t> prune_first, prune_reason, prune_reason_out;  // per slot: by criteria 1-4, final; compacted for a fetch
    DevBuf<unsigned long long> prune_ctr;
    bool prune_valid = false;
    // dsx_map_export's remaining outputs and dsx_map_merge's counters (include/dsi_map_merge.h)
    DevBuf<unsigned long long> sums_out, merge_ctr;
    DevBuf<uint32_t> stamp_out;
    // the last correspondence pass with this map as the first (dsx_map_align_step, include/dsi_map_align.h): valid until
    // the map changes
    DevBuf<unsigned long long> align_key, align_key_out, align_ctr;  // per slot: the correspondence's key; compacted; the moments
    DevBuf<float> align_dist, align_dist_out;
    uint32_t align_min_points = 0, align_min_windows = 0;
    bool align_valid = false;
    // the last labelling (dsx_map_components, include/dsi_map_components.h): valid until the map changes; the selection
    // (dsx_map_components_select) is valid as long as the labelling it was made on
    DevBuf<uint32_t> comp_parent, comp_cells;           // per slot: the root's slot; at a root, its component's cells
    DevBuf<unsigned long long> comp_label, comp_points; // at a root: the component's label and points
    DevBuf<uint8_t> comp_reason, comp_reason_out;       // per slot: the selection's reason; compacted for a fetch
    DevBuf<unsigned long long> comp_ctr, comp_top, comp_label_out, comp_cells_out, comp_points_out;
    uint32_t comp_min_points = 0, comp_min_windows = 0;
    bool comp_valid = false, comp_select_valid = false;
    // the last self query (dsx_map_knn, include/dsi_map_knn.h): valid until the map changes; the selection
    // (dsx_map_knn_select) is valid as long as the query it was made on
    DevBuf<uint8_t> knn_found, knn_found_out, knn_reason, knn_reason_out;  // per slot; compacted for a fetch
    DevBuf<uint32_t> knn_q, knn_q_out;
    DevBuf<float> knn_mean, knn_mean_out, knn_dist_out;                    // knn_dist_out and the two below: dsx_map_knn_points' rows
    DevBuf<unsigned long long> knn_key_out, knn_ctr;
    DevBuf<uint8_t> knn_pt_found;
    dsx_map_knn_opts_t knn_opts = {};
    unsigned long long knn_moments[4] = {0, 0, 0, 0};  // N, sum_q, sum_q2 low and high
    bool knn_valid = false, knn_select_valid = false;
    // the last local-shape pass (dsx_map_pca, include/dsi_map_pca.h): valid until the map changes; the selection
    // (dsx_map_pca_select) is valid as long as the pass it was made on
    DevBuf<float> pca_normal, pca_tangent, pca_eval, pca_normal_out, pca_tangent_out, pca_eval_out;  // per slot; compacted for a fetch
    DevBuf<uint16_t> pca_members, pca_members_out;
    DevBuf<uint8_t> pca_label, pca_flags, pca_reason, pca_label_out, pca_flags_out, pca_reason_out;
    DevBuf<long long> pca_moments, pca_moments_out;  // with keep_moments only
    DevBuf<unsigned long long> pca_ctr;
    dsx_map_pca_opts_t pca_opts = {};
    bool pca_valid = false, pca_select_valid = false;
    // the visibility tally (dsx_map_observe, include/dsi_map_visibility.h): accumulates over observations until the map
    // changes or dsx_map_visibility_clear; the selection (dsx_map_visibility_select) is valid until the next observation
    DevBuf<uint32_t> vis_seen, vis_agree, vis_through, vis_seen_out, vis_agree_out, vis_through_out;  // per slot; compacted for a fetch
    DevBuf<uint8_t> vis_reason, vis_reason_out, vis_mask;  // vis_mask and vis_depth: dsx_map_observe's staging
    DevBuf<float> vis_depth;
    DevBuf<unsigned long long> vis_ctr;
    uint64_t vis_views = 0;
    bool vis_valid = false, vis_select_valid = false;
};

namespace {

constexpr int kMapMinLog2 = 8, kMapMaxLog2 = 27;
static_assert(dsi::kKnnMaxCells == (uint64_t)1 << kMapMaxLog2, "the threshold's bound on N is the table's");
constexpr int kMapViewMaxLog2 = 26, kMapMaxSplat = 4;

// drops the last render's buffers: a render of another size starts from nothing instead of keeping the larger ones
void map_render_release(dsi_map* mp)
{
    mp->zkey.release();            // early, as are the four below: dsi_map_render of another size
    mp->hits.release();            // per-pixel hit counts
    mp->render_windows.release();  // per-pixel window counts
    mp->render_depth.release();    // the depth image
    mp->render_mask.release();     // its mask
    mp->render_width = mp->render_height = 0;
    mp->render_valid = false;
}

// The map changes (or may change) from here on: every derived result is stale, the selections with the passes they were
// made on.  The render keeps its buffers (map_render_release drops them: a render of another size).  A reader of a
// *_select_valid flag tests the parent flag first and a parent pass clears its selection when it starts, so that clearing
// the selections here is not observable; it keeps the list in one place.
void map_changed(dsi_map* mp)
{
    mp->render_valid = mp->compare_valid = mp->prune_valid = mp->align_valid = false;
    mp->comp_valid = mp->comp_select_valid = mp->knn_valid = mp->knn_select_valid = mp->pca_valid = mp->pca_select_valid = false;
    mp->vis_valid = mp->vis_select_valid = false;
}

// the table doubled until occupied + n <= 3/4 of its slots (the caller checked that 2^27 slots are enough)
int map_grow_for(dsi_map* mp, size_t n)
{
    uint32_t want = mp->cap_log2;
    while ((mp->host_ctr[0] + n) * 4 > ((uint64_t)3 << want)) ++want;
    if (want == mp->cap_log2) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    DevBuf<unsigned char> block;
    HIP_TRY(block.reserve(dsi::map_table_bytes(want)));
    hipError_t e = hipMemsetAsync(block.p, 0, dsi::map_table_bytes(want), st);
    if (e == hipSuccess && mp->host_ctr[0])
        e = dsi::launch_map_rehash(st, dsi::map_table_at(mp->block.p, mp->cap_log2), dsi::map_table_at(block.p, want), mp->ctr.p);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(DSI_ERR_HIP, "growing the map's table to 2^%u slots failed: %s", want, hipGetErrorString(e));
    mp->block = std::move(block);  // (frees the old table)
    mp->growths += want - mp->cap_log2;
    mp->cap_log2 = want;
    return DSI_OK;
}

// one integrate call of at most n points on the map's stream, made by launch(serial, table); synchronises
int map_integrate_call(dsi_map* mp, size_t n, const std::function<hipError_t(uint32_t, const dsi::MapTable&)>& launch, size_t* n_accepted,
                       size_t* n_rejected)
{
    map_changed(mp);
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    REQUIRE(mp->calls < 0xffffffffull, DSI_ERR_INVALID, "at most 2^32 - 1 integrate calls per map");
    REQUIRE((mp->host_ctr[0] + n) * 4 <= ((uint64_t)3 << kMapMaxLog2), DSI_ERR_INVALID,
            "%llu cells + %zu points need more than 2^%d slots: the map is unchanged", mp->host_ctr[0], n, kMapMaxLog2);
    if (int rc = map_grow_for(mp, n)) return rc;
    hipStream_t st = mp->ctx->stream;
    const uint32_t serial = (uint32_t)++mp->calls;
    const unsigned long long accepted_before = mp->host_ctr[1], rejected_before = mp->host_ctr[2];
    HIP_TRY(launch(serial, dsi::map_table_at(mp->block.p, mp->cap_log2)));
    HIP_TRY(hipMemcpyAsync(mp->host_ctr, mp->ctr.p, sizeof mp->host_ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_HIP, "the map's table ran full (%llu points lost): an engine bug, the map is unusable",
            mp->host_ctr[3]);
    if (n_accepted) *n_accepted = (size_t)(mp->host_ctr[1] - accepted_before);
    if (n_rejected) *n_rejected = (size_t)(mp->host_ctr[2] - rejected_before);
    return DSI_OK;
}

// one integrate call of n device points (stride floats each)
int map_integrate_device(dsi_map* mp, const float* pts_dev, size_t stride, size_t n, const double T_w_rv[12], size_t* n_rejected)
{
    return map_integrate_call(
        mp, n,
        [&](uint32_t serial, const dsi::MapTable& t) {
            return dsi::launch_map_integrate(mp->ctx->stream, pts_dev, (uint32_t)stride, (uint32_t)n, T_w_rv, mp->leaf, serial, t, mp->ctr.p);
        },
        nullptr, n_rejected);
}

int check_map_pose(const double T[12])
{
    REQUIRE(T, DSI_ERR_INVALID, "T_w_rv is null");
    return DSI_OK;
}

// the filtered cells counted and scanned into mp->blk; *total their number.  Synchronises.
int map_count_device(dsi_map* mp, uint32_t min_points, uint32_t min_windows, size_t* total)
{
    const size_t cap = (size_t)1 << mp->cap_log2, words = dsi::pc_block_words(cap);
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->blk.reserve(words));
    HIP_TRY(mp->tiles.reserve(dsi::pc_scan_tile_words(words)));
    HIP_TRY(dsi::launch_map_count(st, dsi::map_table_at(mp->block.p, mp->cap_log2), min_points, min_windows, mp->blk.p, mp->tiles.p));
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, mp->blk.p + words - 1, sizeof n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *total = n;
    return DSI_OK;
}

// what every dsx_map_*_fetch does before its gather: the cells under the pass's filter counted and scanned into mp->blk,
// *n and *total their number, refused when `capacity` is smaller.  *total == 0: there is nothing to gather.  Synchronises.
int map_fetch_count(dsi_map* mp, uint32_t min_points, uint32_t min_windows, size_t capacity, size_t* n, size_t* total)
{
    if (int rc = map_count_device(mp, min_points, min_windows, total)) return rc;
    *n = *total;
    REQUIRE(capacity >= *total, DSI_ERR_INVALID, "capacity of %zu cells is too small: %zu needed", capacity, *total);
    return DSI_OK;
}

}  // namespace

int dsi_invert_pose(const double T[12], double out[12])
{
    REQUIRE(T && out, DSI_ERR_INVALID, "null argument");
    double r[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r[4 * i + j] = T[4 * j + i];
        r[4 * i + 3] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
    }
    std::memcpy(out, r, sizeof r);
    return DSI_OK;
}

int dsi_map_create(dsi_context_t* ctx, double leaf, int capacity_log2, dsi_map_t** out)
{
    REQUIRE(ctx && out, DSI_ERR_INVALID, "null argument");
    REQUIRE(std::isfinite(leaf) && leaf > 0.0, DSI_ERR_INVALID, "leaf must be finite and > 0 (got %g)", leaf);
    REQUIRE(capacity_log2 >= kMapMinLog2 && capacity_log2 <= kMapMaxLog2, DSI_ERR_INVALID, "capacity_log2 must be in %d..%d (got %d)",
            kMapMinLog2, kMapMaxLog2, capacity_log2);
    if (int rc = set_device(ctx)) return rc;
    dsi_map* mp = new (std::nothrow) dsi_map;
    REQUIRE(mp, DSI_ERR_INVALID, "out of host memory");
    mp->ctx = ctx;
    mp->leaf = leaf;
    mp->cap_log2 = (uint32_t)capacity_log2;
    const size_t bytes = dsi::map_table_bytes(mp->cap_log2);
    hipError_t e = mp->block.reserve(bytes);
    if (e == hipSuccess) e = mp->ctr.reserve(sizeof mp->host_ctr / sizeof mp->host_ctr[0]);
    if (e == hipSuccess) e = hipMemsetAsync(mp->block.p, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(mp->ctr.p, 0, sizeof mp->host_ctr, ctx->stream);
    if (e != hipSuccess) {
        delete mp;
        return fail(DSI_ERR_HIP, "map allocation of 2^%d slots failed: %s", capacity_log2, hipGetErrorString(e));
    }
    ++ctx->children;
    *out = mp;
    return DSI_OK;
}

int dsi_map_destroy(dsi_map_t* mp)
{
    if (!mp) return DSI_OK;
    (void)hipSetDevice(mp->ctx->device);
    (void)hipStreamSynchronize(mp->ctx->stream);
    --mp->ctx->children;
    delete mp;
    return DSI_OK;
}

int dsi_map_reset(dsi_map_t* mp)
{
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    map_changed(mp);
    if (int rc = set_device(mp->ctx)) return rc;
    HIP_TRY(hipMemsetAsync(mp->block.p, 0, dsi::map_table_bytes(mp->cap_log2), mp->ctx->stream));
    HIP_TRY(hipMemsetAsync(mp->ctr.p, 0, sizeof mp->host_ctr, mp->ctx->stream));
    std::memset(mp->host_ctr, 0, sizeof mp->host_ctr);
    mp->calls = mp->growths = 0;
    return DSI_OK;
}

int dsi_map_integrate(dsi_map_t* mp, const float* xyz_host, size_t stride_floats, size_t n, const double T_w_rv[12], size_t* n_rejected)
{
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(stride_floats == 3 || stride_floats == 4, DSI_ERR_INVALID, "stride_floats must be 3 or 4 (got %zu)", stride_floats);
    REQUIRE(n == 0 || xyz_host, DSI_ERR_INVALID, "xyz_host is null");
    if (int rc = check_map_pose(T_w_rv)) return rc;
    REQUIRE(n <= ((size_t)1 << kMapMaxLog2), DSI_ERR_INVALID, "at most 2^%d points per call (got %zu)", kMapMaxLog2, n);
    if (int rc = set_device(mp->ctx)) return rc;
    if (n) {
        HIP_TRY(mp->upload.reserve(n * stride_floats));
        HIP_TRY(hipMemcpyAsync(mp->upload.p, xyz_host, n * stride_floats * sizeof(float), hipMemcpyHostToDevice, mp->ctx->stream));
    }
    return map_integrate_device(mp, mp->upload.p, stride_floats, n, T_w_rv, n_rejected);
}

int dsi_map_integrate_mapper(dsi_map_t* mp, dsi_mapper_t* m, const dsi_pointcloud_options_t* opts_pc, const double T_w_rv[12],
                             size_t* n_points, size_t* n_rejected)
{
    REQUIRE(mp && m && opts_pc, DSI_ERR_INVALID, "null argument");
    if (int rc = check_map_pose(T_w_rv)) return rc;
    REQUIRE(mp->ctx == m->ctx, DSI_ERR_CONTEXT, "the map and the mapper live on different contexts");
    uint32_t counts[2];
    if (int rc = pointcloud_device(m, nullptr, nullptr, opts_pc, counts)) return rc;
    if (n_points) *n_points = counts[1];
    return map_integrate_device(mp, reinterpret_cast<const float*>(m->pc.out.p), 4, counts[1], T_w_rv, n_rejected);
}

int dsi_map_info(dsi_map_t* mp, dsi_map_info_t* info)
{
    REQUIRE(mp && info, DSI_ERR_INVALID, "null argument");
    info->leaf = mp->leaf;
    info->capacity = (uint64_t)1 << mp->cap_log2;
    info->occupied = mp->host_ctr[0];
    info->calls = mp->calls;
    info->accepted = mp->host_ctr[1];
    info->rejected = mp->host_ctr[2];
    info->growths = mp->growths;
    return DSI_OK;
}

int dsi_map_count(dsi_map_t* mp, uint32_t min_points, uint32_t min_windows, size_t* n)
{
    REQUIRE(mp && n, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(mp->ctx)) return rc;
    return map_count_device(mp, min_points, min_windows, n);
}

int dsi_map_extract(dsi_map_t* mp, uint32_t min_points, uint32_t min_windows, float* xyz_host, uint32_t* n_points_host,
                    uint32_t* n_windows_host, uint64_t* keys_host, size_t capacity, size_t* n)
{
    REQUIRE(mp && n, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_count_device(mp, min_points, min_windows, &total)) return rc;
    *n = total;
    REQUIRE(capacity >= total, DSI_ERR_INVALID, "capacity of %zu cells is too small: %zu needed", capacity, total);
    if (!total) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->xyz.reserve(3 * total));
    HIP_TRY(mp->n_out.reserve(total));
    HIP_TRY(mp->w_out.reserve(total));
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(dsi::launch_map_extract(st, dsi::map_table_at(mp->block.p, mp->cap_log2), min_points, min_windows, mp->leaf, mp->blk.p, mp->xyz.p,
                                    mp->n_out.p, mp->w_out.p, mp->key_out.p));
    if (xyz_host) HIP_TRY(hipMemcpyAsync(xyz_host, mp->xyz.p, 3 * total * sizeof(float), hipMemcpyDeviceToHost, st));
    if (n_points_host) HIP_TRY(hipMemcpyAsync(n_points_host, mp->n_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (n_windows_host) HIP_TRY(hipMemcpyAsync(n_windows_host, mp->w_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsi_map_render(dsi_map_t* mp, const dsi_map_view_t* view, dsi_map_render_info_t* info)
{
    // (the view first: its bounds can then be exercised without a device, with no map at hand)
    REQUIRE(view, DSI_ERR_INVALID, "view is null");
    REQUIRE(view->width >= 1 && view->height >= 1, DSI_ERR_INVALID, "the view must be at least 1 x 1 (got %d x %d)", view->width,
            view->height);
    REQUIRE((uint64_t)view->width * (uint64_t)view->height <= ((uint64_t)1 << kMapViewMaxLog2), DSI_ERR_INVALID,
            "a view holds at most 2^%d pixels (got %d x %d)", kMapViewMaxLog2, view->width, view->height);
    REQUIRE(view->splat >= 0 && view->splat <= kMapMaxSplat, DSI_ERR_INVALID, "splat must be in 0..%d (got %d)", kMapMaxSplat,
            view->splat);
    REQUIRE(std::isfinite(view->fx) && std::isfinite(view->fy) && view->fx != 0.0 && view->fy != 0.0, DSI_ERR_INVALID,
            "fx and fy must be finite and not 0 (got %g, %g)", view->fx, view->fy);
    REQUIRE(std::isfinite(view->cx) && std::isfinite(view->cy), DSI_ERR_INVALID, "cx and cy must be finite (got %g, %g)", view->cx,
            view->cy);
    REQUIRE(std::isfinite(view->min_depth) && std::isfinite(view->max_depth) && view->min_depth >= (double)FLT_MIN &&
                view->min_depth < view->max_depth && view->max_depth <= (double)FLT_MAX,
            DSI_ERR_INVALID, "the depth range must satisfy FLT_MIN <= min_depth < max_depth <= FLT_MAX (got %g, %g)", view->min_depth,
            view->max_depth);
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = set_device(mp->ctx)) return rc;
    hipStream_t st = mp->ctx->stream;
    const size_t npix = (size_t)view->width * (size_t)view->height;
    mp->render_valid = false;
    if (npix != (size_t)mp->render_width * (size_t)mp->render_height) {
        HIP_TRY(hipStreamSynchronize(st));
        map_render_release(mp);
    }
    HIP_TRY(mp->zkey.reserve(npix));
    HIP_TRY(mp->hits.reserve(npix));
    HIP_TRY(mp->render_windows.reserve(npix));
    HIP_TRY(mp->render_depth.reserve(npix));
    HIP_TRY(mp->render_mask.reserve(npix));
    HIP_TRY(mp->render_ctr.reserve(dsi::kMapRenderCounters));
    mp->render_width = view->width;
    mp->render_height = view->height;
    dsi::MapView v;
    std::memcpy(v.T, view->T_v_w, sizeof v.T);
    v.fx = view->fx, v.fy = view->fy, v.cx = view->cx, v.cy = view->cy;
    v.min_depth = view->min_depth, v.max_depth = view->max_depth;
    v.width = view->width, v.height = view->height, v.splat = view->splat;
    v.min_points = view->min_points, v.min_windows = view->min_windows;
    const dsi::MapImage img{mp->zkey.p, mp->hits.p, mp->render_windows.p, mp->render_depth.p, mp->render_mask.p};
    unsigned long long ctr[dsi::kMapRenderCounters] = {0, 0, 0, 0, 0};
    HIP_TRY(dsi::launch_map_render(st, dsi::map_table_at(mp->block.p, mp->cap_log2), v, mp->leaf, img, mp->render_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->render_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mp->render_valid = true;
    if (info) {
        info->width = view->width;
        info->height = view->height;
        info->n_cells = ctr[0];
        info->n_clipped = ctr[1];
        info->n_outside = ctr[2];
        info->n_drawn = ctr[3];
        info->n_pixels = ctr[4];
    }
    return DSI_OK;
}

namespace {

int map_render_check(const dsi_map* mp)
{
    REQUIRE(mp->render_valid, DSI_ERR_INVALID,
            "no render of the map as it stands: call dsi_map_render (after the last dsi_map_reset or integrate call)");
    return DSI_OK;
}

}  // namespace

int dsi_map_render_fetch(dsi_map_t* mp, float* depth_host, uint32_t* windows_host, uint32_t* hits_host, uint8_t* mask_host)
{
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = map_render_check(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    hipStream_t st = mp->ctx->stream;
    const size_t npix = (size_t)mp->render_width * (size_t)mp->render_height;
    if (depth_host) HIP_TRY(hipMemcpyAsync(depth_host, mp->render_depth.p, npix * sizeof(float), hipMemcpyDeviceToHost, st));
    if (windows_host) HIP_TRY(hipMemcpyAsync(windows_host, mp->render_windows.p, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (hits_host) HIP_TRY(hipMemcpyAsync(hits_host, mp->hits.p, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (mask_host) HIP_TRY(hipMemcpyAsync(mask_host, mp->render_mask.p, npix, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsi_score_add_map_render(dsi_score_t* s, dsi_map_t* mp, const float* gt_host)
{
    REQUIRE(s && mp && gt_host, DSI_ERR_INVALID, "null argument");
    REQUIRE(mp->ctx == s->ctx, DSI_ERR_CONTEXT, "map and score belong to different contexts");
    if (int rc = map_render_check(mp)) return rc;
    if (int rc = set_device(s->ctx)) return rc;
    const size_t npix = (size_t)mp->render_width * (size_t)mp->render_height;
    HIP_TRY(s->gt.reserve(npix));
    HIP_TRY(hipMemcpyAsync(s->gt.p, gt_host, npix * sizeof(float), hipMemcpyHostToDevice, s->ctx->stream));
    return score_add_device(s, mp->render_depth.p, mp->render_mask.p, s->gt.p, npix);
}

int dsi_score_add_map_render_gt(dsi_score_t* s, dsi_map_t* mp, dsi_gt_t* gt)
{
    REQUIRE(s && mp && gt, DSI_ERR_INVALID, "null argument");
    REQUIRE(mp->ctx == s->ctx, DSI_ERR_CONTEXT, "map and score belong to different contexts");
    REQUIRE(gt->ctx == s->ctx, DSI_ERR_CONTEXT, "projector and score belong to different contexts");
    if (int rc = map_render_check(mp)) return rc;
    const size_t npix = (size_t)mp->render_width * (size_t)mp->render_height;
    REQUIRE(npix == gt_npix(gt), DSI_ERR_INVALID, "the render holds %d x %d pixels, the projector's map %d x %d", mp->render_width,
            mp->render_height, gt->width, gt->height);
    if (int rc = set_device(s->ctx)) return rc;
    return score_add_device(s, mp->render_depth.p, mp->render_mask.p, gt_out(gt), npix);
}

// ---- the map scored in 3-D (include/dsi_map_eval.h; DESIGN.md 7j "Scoring the map in 3-D") ----

namespace {

// dsi_map_view_t's bounds on a depth image and its pinhole: decided without a device, before any handle is looked at
int check_depth_image(int32_t width, int32_t height, double fx, double fy, double cx, double cy, double min_depth, double max_depth)
{
    REQUIRE(width >= 1 && height >= 1, DSI_ERR_INVALID, "the image must be at least 1 x 1 (got %d x %d)", width, height);
    REQUIRE((uint64_t)width * (uint64_t)height <= ((uint64_t)1 << kMapViewMaxLog2), DSI_ERR_INVALID,
            "an image holds at most 2^%d pixels (got %d x %d)", kMapViewMaxLog2, width, height);
    REQUIRE(std::isfinite(fx) && std::isfinite(fy) && fx != 0.0 && fy != 0.0, DSI_ERR_INVALID,
            "fx and fy must be finite and not 0 (got %g, %g)", fx, fy);
    REQUIRE(std::isfinite(cx) && std::isfinite(cy), DSI_ERR_INVALID, "cx and cy must be finite (got %g, %g)", cx, cy);
    REQUIRE(std::isfinite(min_depth) && std::isfinite(max_depth) && min_depth >= (double)FLT_MIN && min_depth < max_depth &&
                max_depth <= (double)FLT_MAX,
            DSI_ERR_INVALID, "the depth range must satisfy FLT_MIN <= min_depth < max_depth <= FLT_MAX (got %g, %g)", min_depth,
            max_depth);
    return DSI_OK;
}

// one integrate call of a device depth image (mask_dev may be null); the table grows for width * height points
int map_integrate_depth_device(dsi_map* mp, const float* depth_dev, const uint8_t* mask_dev, int32_t width, int32_t height, double fx,
                               double fy, double cx, double cy, double min_depth, double max_depth, const double T_w_c[12],
                               uint64_t* n_points, uint64_t* n_rejected)
{
    const dsi::MapDepthImage g{(uint32_t)width, (uint32_t)width * (uint32_t)height, fx, fy, cx, cy, min_depth, max_depth};
    size_t accepted = 0, rejected = 0;
    if (int rc = map_integrate_call(
            mp, g.npix,
            [&](uint32_t serial, const dsi::MapTable& t) {
                return dsi::launch_map_integrate_depth(mp->ctx->stream, depth_dev, mask_dev, g, T_w_c, mp->leaf, serial, t, mp->ctr.p);
            },
            &accepted, &rejected))
        return rc;
    if (n_points) *n_points = (uint64_t)accepted + (uint64_t)rejected;
    if (n_rejected) *n_rejected = rejected;
    return DSI_OK;
}

}  // namespace

int dsx_map_integrate_depth(dsi_map_t* mp, const float* depth_host, const uint8_t* mask_host, int32_t width, int32_t height, double fx,
                            double fy, double cx, double cy, double min_depth, double max_depth, const double T_w_c[12],
                            uint64_t* n_points, uint64_t* n_rejected)
{
    if (int rc = check_depth_image(width, height, fx, fy, cx, cy, min_depth, max_depth)) return rc;
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(depth_host, DSI_ERR_INVALID, "depth_host is null");
    REQUIRE(T_w_c, DSI_ERR_INVALID, "T_w_c is null");
    if (int rc = set_device(mp->ctx)) return rc;
    const size_t npix = (size_t)width * (size_t)height;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->upload.reserve(npix));
    HIP_TRY(hipMemcpyAsync(mp->upload.p, depth_host, npix * sizeof(float), hipMemcpyHostToDevice, st));
    if (mask_host) {
        HIP_TRY(mp->depth_mask.reserve(npix));
        HIP_TRY(hipMemcpyAsync(mp->depth_mask.p, mask_host, npix, hipMemcpyHostToDevice, st));
    }
    return map_integrate_depth_device(mp, mp->upload.p, mask_host ? mp->depth_mask.p : nullptr, width, height, fx, fy, cx, cy, min_depth,
                                      max_depth, T_w_c, n_points, n_rejected);
}

int dsx_map_integrate_depth_gt(dsi_map_t* mp, dsi_gt_t* gt, double fx, double fy, double cx, double cy, double min_depth, double max_depth,
                               const double T_w_c[12], uint64_t* n_points, uint64_t* n_rejected)
{
    if (int rc = check_depth_image(1, 1, fx, fy, cx, cy, min_depth, max_depth)) return rc;  // (the pinhole, with no handle at hand)
    REQUIRE(mp && gt, DSI_ERR_INVALID, "null argument");
    REQUIRE(T_w_c, DSI_ERR_INVALID, "T_w_c is null");
    REQUIRE(mp->ctx == gt->ctx, DSI_ERR_CONTEXT, "the map and the projector live on different contexts");
    if (int rc = check_depth_image(gt->width, gt->height, fx, fy, cx, cy, min_depth, max_depth)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    return map_integrate_depth_device(mp, gt_out(gt), nullptr, gt->width, gt->height, fx, fy, cx, cy, min_depth, max_depth, T_w_c,
                                      n_points, n_rejected);
}

int dsx_map_compare(dsi_map_t* a, dsi_map_t* b, const dsx_map_compare_opts_t* opts, uint64_t* hist_host, dsx_map_compare_info_t* info)
{
    // (the options first: radius and n_bins can then be exercised without a device, with no map at hand)
    REQUIRE(opts, DSI_ERR_INVALID, "opts is null");
    REQUIRE(std::isfinite(opts->radius) && opts->radius > 0.0, DSI_ERR_INVALID, "radius must be finite and > 0 (got %g)", opts->radius);
    REQUIRE(opts->n_bins >= 1 && opts->n_bins <= dsi::kMapCompareMaxBins, DSI_ERR_INVALID, "n_bins must be in 1..%d (got %d)",
            dsi::kMapCompareMaxBins, opts->n_bins);
    const double bin_width = opts->radius / (double)opts->n_bins;
    REQUIRE(bin_width > 0.0, DSI_ERR_INVALID, "radius / n_bins underflows to 0 (radius %g, n_bins %d)", opts->radius, opts->n_bins);
    REQUIRE(a && b, DSI_ERR_INVALID, "map is null");
    REQUIRE(a->ctx == b->ctx, DSI_ERR_CONTEXT, "the maps live on different contexts");
    const double reach_d = std::ceil(opts->radius / b->leaf);
    REQUIRE(reach_d >= 1.0 && reach_d <= (double)dsi::kMapCompareMaxReach, DSI_ERR_INVALID,
            "reach = ceil(radius / leaf_b) must be in 1..%d (radius %g, leaf_b %g)", dsi::kMapCompareMaxReach, opts->radius, b->leaf);
    if (int rc = set_device(a->ctx)) return rc;
    hipStream_t st = a->ctx->stream;
    a->compare_valid = false;
    HIP_TRY(a->cmp_dist.reserve((size_t)1 << a->cap_log2));
    HIP_TRY(a->cmp_hist.reserve(dsi::kMapCompareMaxBins));
    HIP_TRY(a->cmp_ctr.reserve(dsi::kMapCompareCounters));
    dsi::MapCompare o;
    o.leaf_a = a->leaf, o.leaf_b = b->leaf, o.radius = opts->radius, o.bin_width = bin_width;
    o.min_points_a = opts->min_points_a, o.min_windows_a = opts->min_windows_a;
    o.min_points_b = opts->min_points_b, o.min_windows_b = opts->min_windows_b;
    o.reach = (int)reach_d, o.n_bins = opts->n_bins;
    unsigned long long ctr[dsi::kMapCompareCounters] = {0, 0, 0};
    HIP_TRY(dsi::launch_map_compare(st, dsi::map_table_at(a->block.p, a->cap_log2), dsi::map_table_at(b->block.p, b->cap_log2), o,
                                    a->cmp_dist.p, a->cmp_hist.p, a->cmp_ctr.p));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "64-bit counts");
    if (hist_host)
        HIP_TRY(hipMemcpyAsync(hist_host, a->cmp_hist.p, (size_t)opts->n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ctr, a->cmp_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    a->cmp_min_points = opts->min_points_a;
    a->cmp_min_windows = opts->min_windows_a;
    a->compare_valid = true;
    if (info) {
        info->n_cells = ctr[0] + ctr[1];
        info->n_matched = ctr[0];
        info->n_unmatched = ctr[1];
        info->sum_q = ctr[2];
        info->reach = o.reach;
    }
    return DSI_OK;
}

int dsx_map_compare_fetch(dsi_map_t* a, float* dist_host, uint64_t* keys_host, size_t capacity, size_t* n)
{
    REQUIRE(a && n, DSI_ERR_INVALID, "null argument");
    REQUIRE(a->compare_valid, DSI_ERR_INVALID,
            "no compare of the map as it stands: call dsx_map_compare (after the last dsi_map_reset or integrate call)");
    if (int rc = set_device(a->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(a, a->cmp_min_points, a->cmp_min_windows, capacity, n, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = a->ctx->stream;
    HIP_TRY(a->cmp_dist_out.reserve(total));
    HIP_TRY(a->key_out.reserve(total));
    HIP_TRY(dsi::launch_map_compare_gather(st, dsi::map_table_at(a->block.p, a->cap_log2), a->cmp_min_points, a->cmp_min_windows,
                                           a->cmp_dist.p, a->blk.p, a->cmp_dist_out.p, a->key_out.p));
    if (dist_host) HIP_TRY(hipMemcpyAsync(dist_host, a->cmp_dist_out.p, total * sizeof(float), hipMemcpyDeviceToHost, st));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, a->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

// ---- pruning the map (include/dsi_map_prune.h; DESIGN.md 7j "Pruning") ----

namespace {

// the bounds of the options: decided without a device, before any handle is looked at
int check_prune_opts(const dsx_map_prune_opts_t* o)
{
    REQUIRE(o, DSI_ERR_INVALID, "opts is null");
    REQUIRE(o->use_box == 0 || o->use_box == 1, DSI_ERR_INVALID, "use_box must be 0 or 1 (got %d)", o->use_box);
    if (o->use_box)
        for (int a = 0; a < 3; ++a)
            REQUIRE(o->box_lo[a] <= o->box_hi[a], DSI_ERR_INVALID, "the box needs box_lo <= box_hi without NaN on axis %d (got %g, %g)",
                    a, o->box_lo[a], o->box_hi[a]);  // (NaN compares false)
    REQUIRE(o->reach >= 0 && o->reach <= dsi::kMapPruneMaxReach, DSI_ERR_INVALID, "reach must be in 0..%d (got %d)",
            dsi::kMapPruneMaxReach, o->reach);
    const uint32_t most = (uint32_t)((2 * o->reach + 1) * (2 * o->reach + 1) * (2 * o->reach + 1) - 1);
    if (o->reach > 0)
        REQUIRE(o->min_neighbors >= 1 && o->min_neighbors <= most, DSI_ERR_INVALID, "min_neighbors must be in 1..%u at reach %d (got %u)",
                most, o->reach, o->min_neighbors);
    else
        REQUIRE(o->min_neighbors == 0, DSI_ERR_INVALID, "min_neighbors must be 0 at reach 0 (got %u)", o->min_neighbors);
    REQUIRE(o->shrink == 0 || o->shrink == 1, DSI_ERR_INVALID, "shrink must be 0 or 1 (got %d)", o->shrink);
    return DSI_OK;
}

// every cell classified into mp->prune_first / prune_reason and counted into ctr (kMapPruneCounters); synchronises
int map_prune_classify_device(dsi_map* mp, const dsx_map_prune_opts_t* opts, unsigned long long* ctr)
{
    hipStream_t st = mp->ctx->stream;
    const size_t cap = (size_t)1 << mp->cap_log2;
    HIP_TRY(mp->prune_first.reserve(cap));
    HIP_TRY(mp->prune_reason.reserve(cap));
    HIP_TRY(mp->prune_ctr.reserve(dsi::kMapPruneCounters));
    dsi::MapPrune o;
    o.leaf = mp->leaf;
    for (int a = 0; a < 3; ++a) o.box_lo[a] = opts->box_lo[a], o.box_hi[a] = opts->box_hi[a];
    o.max_age = opts->max_age;
    o.min_points = opts->min_points, o.min_windows = opts->min_windows;
    o.calls = (uint32_t)mp->calls;  // (< 2^32: map_integrate_call)
    o.min_neighbors = opts->min_neighbors;
    o.use_box = opts->use_box, o.reach = opts->reach;
    HIP_TRY(dsi::launch_map_prune_classify(st, dsi::map_table_at(mp->block.p, mp->cap_log2), o, mp->prune_first.p, mp->prune_reason.p,
                                           mp->prune_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->prune_ctr.p, dsi::kMapPruneCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

void map_prune_info(const dsi_map* mp, const unsigned long long* ctr, dsx_map_prune_info_t* info)
{
    if (!info) return;
    info->n_kept = ctr[0];
    info->n_cells = ctr[0];
    for (int r = 0; r < 5; ++r) {
        info->n_removed[r] = ctr[1 + r];
        info->n_cells += ctr[1 + r];
    }
    info->capacity = (uint64_t)1 << mp->cap_log2;
}

// The rebuild that every prune ends with: the `kept` cells with reason_dev[slot] == 0 into a fresh table, of the smallest
// size that holds them at 3/4 when `shrink`, else of the present size.  Nothing leaves (!removed_any) and the size stays:
// the table is the result already.  The new table is allocated before anything is touched -- when that fails the map and
// its derived results are as the caller left them --, then map_changed, then the rebuild on the map's stream; synchronises.
int map_rebuild_kept(dsi_map* mp, const uint8_t* reason_dev, unsigned long long kept, bool removed_any, int shrink)
{
    hipStream_t st = mp->ctx->stream;
    uint32_t want = mp->cap_log2;
    if (shrink)
        for (want = kMapMinLog2; kept * 4 > ((uint64_t)3 << want); ++want) {
        }
    DevBuf<unsigned char> block;
    const bool rebuild = removed_any || want != mp->cap_log2;
    if (rebuild) {
        const hipError_t e = block.reserve(dsi::map_table_bytes(want));
        if (e != hipSuccess)
            return fail(DSI_ERR_HIP, "a pruned table of 2^%u slots could not be allocated (%s): the map is unchanged", want,
                        hipGetErrorString(e));
    }
    map_changed(mp);
    if (!rebuild) return DSI_OK;
    HIP_TRY(hipMemsetAsync(block.p, 0, dsi::map_table_bytes(want), st));
    HIP_TRY(hipMemsetAsync(mp->ctr.p, 0, sizeof(unsigned long long), st));  // occupied: the rebuild counts the cells it moves
    if (kept)
        HIP_TRY(dsi::launch_map_prune_rehash(st, dsi::map_table_at(mp->block.p, mp->cap_log2), dsi::map_table_at(block.p, want), reason_dev,
                                             mp->ctr.p));
    HIP_TRY(hipMemcpyAsync(mp->host_ctr, mp->ctr.p, sizeof mp->host_ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mp->block = std::move(block);  // (frees the old table)
    mp->cap_log2 = want;
    REQUIRE(mp->host_ctr[3] == 0 && mp->host_ctr[0] == kept, DSI_ERR_HIP,
            "the pruned table holds %llu of %llu kept cells (%llu found it full): an engine bug, the map is unusable", mp->host_ctr[0], kept,
            mp->host_ctr[3]);
    return DSI_OK;
}

}  // namespace

int dsx_map_prune_classify(dsi_map_t* mp, const dsx_map_prune_opts_t* opts, dsx_map_prune_info_t* info)
{
    if (int rc = check_prune_opts(opts)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    if (int rc = set_device(mp->ctx)) return rc;
    mp->prune_valid = false;
    unsigned long long ctr[dsi::kMapPruneCounters] = {0, 0, 0, 0, 0, 0};
    if (int rc = map_prune_classify_device(mp, opts, ctr)) return rc;
    mp->prune_valid = true;
    map_prune_info(mp, ctr, info);
    return DSI_OK;
}

int dsx_map_prune_fetch(dsi_map_t* mp, uint8_t* reason_host, uint64_t* keys_host, size_t capacity, size_t* n)
{
    REQUIRE(mp && n, DSI_ERR_INVALID, "null argument");
    REQUIRE(mp->prune_valid, DSI_ERR_INVALID,
            "no classification of the map as it stands: call dsx_map_prune_classify (after the last reset, integrate call or prune)");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(mp, 1, 1, capacity, n, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->prune_reason_out.reserve(total));
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(dsi::launch_map_prune_gather(st, dsi::map_table_at(mp->block.p, mp->cap_log2), mp->prune_reason.p, mp->blk.p,
                                         mp->prune_reason_out.p, mp->key_out.p));
    if (reason_host) HIP_TRY(hipMemcpyAsync(reason_host, mp->prune_reason_out.p, total, hipMemcpyDeviceToHost, st));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_prune(dsi_map_t* mp, const dsx_map_prune_opts_t* opts, dsx_map_prune_info_t* info)
{
    if (int rc = check_prune_opts(opts)) return rc;
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    if (int rc = set_device(mp->ctx)) return rc;
    map_changed(mp);  // (before the classification: this prune's results are stale even when the rebuild cannot allocate)
    unsigned long long ctr[dsi::kMapPruneCounters] = {0, 0, 0, 0, 0, 0};
    if (int rc = map_prune_classify_device(mp, opts, ctr)) return rc;
    const bool removed_any = ctr[1] + ctr[2] + ctr[3] + ctr[4] + ctr[5] != 0;
    if (int rc = map_rebuild_kept(mp, mp->prune_reason.p, ctr[0], removed_any, opts->shrink)) return rc;
    map_prune_info(mp, ctr, info);
    return DSI_OK;
}

// ---- the map's connected components (include/dsi_map_components.h; DESIGN.md 7j "Components") ----

namespace {

// the bounds of the options: decided without a device, before any handle is looked at
int check_components_opts(const dsx_map_components_opts_t* o)
{
    REQUIRE(o, DSI_ERR_INVALID, "opts is null");
    REQUIRE(o->connectivity == 6 || o->connectivity == 18 || o->connectivity == 26 || o->connectivity == 124, DSI_ERR_INVALID,
            "connectivity must be 6, 18, 26 or 124 (got %d)", o->connectivity);
    return DSI_OK;
}

int check_components_selection(const dsx_map_components_selection_t* s)
{
    REQUIRE(s, DSI_ERR_INVALID, "sel is null");
    REQUIRE(s->keep_largest >= 0 && s->keep_largest <= dsi::kMapCompMaxKeep, DSI_ERR_INVALID, "keep_largest must be in 0..%d (got %d)",
            dsi::kMapCompMaxKeep, s->keep_largest);
    REQUIRE(s->shrink == 0 || s->shrink == 1, DSI_ERR_INVALID, "shrink must be 0 or 1 (got %d)", s->shrink);
    return DSI_OK;
}

dsi::MapComponents map_components_of(const dsi_map* mp)
{
    return dsi::MapComponents{mp->comp_parent.p, mp->comp_label.p, mp->comp_cells.p, mp->comp_points.p};
}

// what every entry point that reads the labelling asks of the map
int check_labelling(const dsi_map* mp)
{
    REQUIRE(mp->comp_valid, DSI_ERR_INVALID,
            "no labelling of the map as it stands: call dsx_map_components (after the last reset, integrate call, merge, import or prune)");
    return DSI_OK;
}

// every cell's reason into mp->comp_reason and the counts into ctr (kMapCompSelectCounters); synchronises
int map_components_select_device(dsi_map* mp, const dsx_map_components_selection_t* sel, unsigned long long* ctr)
{
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->comp_reason.reserve((size_t)1 << mp->cap_log2));
    const dsi::MapCompSelect o{sel->min_cells, sel->min_component_points, sel->keep_largest};
    HIP_TRY(dsi::launch_map_components_select(st, dsi::map_table_at(mp->block.p, mp->cap_log2), map_components_of(mp), o, mp->comp_reason.p,
                                              mp->comp_top.p, mp->comp_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->comp_ctr.p, dsi::kMapCompSelectCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

void map_components_select_info(const dsi_map* mp, const unsigned long long* ctr, dsx_map_components_select_info_t* info)
{
    if (!info) return;
    info->n_kept = ctr[0];
    info->n_cells = ctr[0];
    for (int r = 0; r < 4; ++r) {
        info->n_removed[r] = ctr[1 + r];
        info->n_cells += ctr[1 + r];
    }
    info->n_components_kept = ctr[5];
    info->capacity = (uint64_t)1 << mp->cap_log2;
}

}  // namespace

int dsx_map_components(dsi_map_t* mp, const dsx_map_components_opts_t* opts, dsx_map_components_info_t* info)
{
    if (int rc = check_components_opts(opts)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    if (int rc = set_device(mp->ctx)) return rc;
    mp->comp_valid = mp->comp_select_valid = false;
    hipStream_t st = mp->ctx->stream;
    const size_t cap = (size_t)1 << mp->cap_log2;
    HIP_TRY(mp->comp_parent.reserve(cap));
    HIP_TRY(mp->comp_label.reserve(cap));
    HIP_TRY(mp->comp_cells.reserve(cap));
    HIP_TRY(mp->comp_points.reserve(cap));
    HIP_TRY(mp->comp_ctr.reserve(std::max(dsi::kMapCompCounters, dsi::kMapCompSelectCounters)));
    HIP_TRY(mp->comp_top.reserve(dsi::kMapCompTopWords));
    unsigned long long ctr[dsi::kMapCompCounters] = {0, 0, 0, 0, 0}, top[2] = {0, 0};
    HIP_TRY(dsi::launch_map_components(st, dsi::map_table_at(mp->block.p, mp->cap_log2), opts->min_points, opts->min_windows,
                                       opts->connectivity, map_components_of(mp), mp->comp_top.p, mp->comp_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->comp_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(top, mp->comp_top.p, sizeof top, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mp->comp_min_points = opts->min_points, mp->comp_min_windows = opts->min_windows;
    mp->comp_valid = true;
    if (info) {
        info->n_cells = ctr[0];
        info->n_unlabelled = ctr[1];
        info->n_components = ctr[2];
        info->n_singletons = ctr[3];
        info->largest_cells = top[0];
        info->largest_label = top[0] ? top[1] : 0;
        info->largest_points = top[0] ? ctr[4] : 0;
    }
    return DSI_OK;
}

int dsx_map_components_fetch(dsi_map_t* mp, uint64_t* keys_host, uint64_t* labels_host, uint8_t* reasons_host, size_t capacity, size_t* count)
{
    REQUIRE(mp && count, DSI_ERR_INVALID, "null argument");
    if (int rc = check_labelling(mp)) return rc;
    REQUIRE(!reasons_host || mp->comp_select_valid, DSI_ERR_INVALID,
            "no selection on this labelling: call dsx_map_components_select before asking for reasons");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(mp, mp->comp_min_points, mp->comp_min_windows, capacity, count, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(mp->comp_label_out.reserve(total));
    if (reasons_host) HIP_TRY(mp->comp_reason_out.reserve(total));
    HIP_TRY(dsi::launch_map_components_gather(st, dsi::map_table_at(mp->block.p, mp->cap_log2), mp->comp_min_points, mp->comp_min_windows,
                                              map_components_of(mp), reasons_host ? mp->comp_reason.p : nullptr, mp->blk.p, mp->key_out.p,
                                              mp->comp_label_out.p, reasons_host ? mp->comp_reason_out.p : nullptr));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (labels_host) HIP_TRY(hipMemcpyAsync(labels_host, mp->comp_label_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (reasons_host) HIP_TRY(hipMemcpyAsync(reasons_host, mp->comp_reason_out.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_components_list(dsi_map_t* mp, uint64_t* labels_host, uint64_t* cells_host, uint64_t* points_host, size_t capacity, size_t* count)
{
    REQUIRE(mp && count, DSI_ERR_INVALID, "null argument");
    if (int rc = check_labelling(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    hipStream_t st = mp->ctx->stream;
    const size_t words = dsi::pc_block_words((size_t)1 << mp->cap_log2);
    HIP_TRY(mp->blk.reserve(words));
    HIP_TRY(mp->tiles.reserve(dsi::pc_scan_tile_words(words)));
    const dsi::MapTable t = dsi::map_table_at(mp->block.p, mp->cap_log2);
    HIP_TRY(dsi::launch_map_components_count_roots(st, t, map_components_of(mp), mp->blk.p, mp->tiles.p));
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, mp->blk.p + words - 1, sizeof n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t total = n;
    *count = total;
    REQUIRE(capacity >= total, DSI_ERR_INVALID, "capacity of %zu components is too small: %zu needed", capacity, total);
    if (!total) return DSI_OK;
    HIP_TRY(mp->comp_label_out.reserve(total));
    HIP_TRY(mp->comp_cells_out.reserve(total));
    HIP_TRY(mp->comp_points_out.reserve(total));
    HIP_TRY(dsi::launch_map_components_list(st, t, map_components_of(mp), mp->blk.p, mp->comp_label_out.p, mp->comp_cells_out.p,
                                            mp->comp_points_out.p));
    if (labels_host) HIP_TRY(hipMemcpyAsync(labels_host, mp->comp_label_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (cells_host) HIP_TRY(hipMemcpyAsync(cells_host, mp->comp_cells_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (points_host) HIP_TRY(hipMemcpyAsync(points_host, mp->comp_points_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_components_select(dsi_map_t* mp, const dsx_map_components_selection_t* sel, dsx_map_components_select_info_t* info)
{
    if (int rc = check_components_selection(sel)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_labelling(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->comp_select_valid = false;
    unsigned long long ctr[dsi::kMapCompSelectCounters] = {0, 0, 0, 0, 0, 0};
    if (int rc = map_components_select_device(mp, sel, ctr)) return rc;
    mp->comp_select_valid = true;
    map_components_select_info(mp, ctr, info);
    return DSI_OK;
}

int dsx_map_prune_components(dsi_map_t* mp, const dsx_map_components_selection_t* sel, dsx_map_components_select_info_t* info)
{
    if (int rc = check_components_selection(sel)) return rc;
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_labelling(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->comp_select_valid = false;
    unsigned long long ctr[dsi::kMapCompSelectCounters] = {0, 0, 0, 0, 0, 0};
    if (int rc = map_components_select_device(mp, sel, ctr)) return rc;
    mp->comp_select_valid = true;  // (the reasons are those of the map as it stands, should the rebuild fail to allocate)
    if (int rc = map_rebuild_kept(mp, mp->comp_reason.p, ctr[0], ctr[1] + ctr[2] + ctr[3] + ctr[4] != 0, sel->shrink)) return rc;
    map_components_select_info(mp, ctr, info);
    return DSI_OK;
}

// ---- the map's k nearest cells (include/dsi_map_knn.h; DESIGN.md 7j "Neighbours and statistical outliers") ----

namespace {

// the bounds of the options that need no map: decided without a device, before any handle is looked at
int check_knn_opts(const dsx_map_knn_opts_t* o)
{
    REQUIRE(o, DSI_ERR_INVALID, "opts is null");
    REQUIRE(o->k >= 1 && o->k <= dsi::kMapKnnMaxK, DSI_ERR_INVALID, "k must be in 1..%d (got %d)", dsi::kMapKnnMaxK, o->k);
    REQUIRE(o->min_found >= 1 && o->min_found <= o->k, DSI_ERR_INVALID, "min_found must be in 1..k = %d (got %d)", o->k, o->min_found);
    REQUIRE(std::isfinite(o->radius) && o->radius > 0.0, DSI_ERR_INVALID, "radius must be finite and > 0 (got %g)", o->radius);
    return DSI_OK;
}

int check_knn_selection(const dsx_map_knn_selection_t* s)
{
    REQUIRE(s, DSI_ERR_INVALID, "sel is null");
    REQUIRE(std::isfinite(s->std_mult), DSI_ERR_INVALID, "std_mult must be finite (got %g)", s->std_mult);
    REQUIRE(s->shrink == 0 || s->shrink == 1, DSI_ERR_INVALID, "shrink must be 0 or 1 (got %d)", s->shrink);
    return DSI_OK;
}

// the kernels' view of the options; reach = ceil(radius / leaf) is judged here, with the map at hand
int map_knn_of(const dsi_map* mp, const dsx_map_knn_opts_t* opts, dsi::MapKnn* o)
{
    const double reach_d = std::ceil(opts->radius / mp->leaf);
    REQUIRE(reach_d >= 1.0 && reach_d <= (double)dsi::kMapKnnMaxReach, DSI_ERR_INVALID,
            "reach = ceil(radius / leaf) must be in 1..%d (radius %g, leaf %g)", dsi::kMapKnnMaxReach, opts->radius, mp->leaf);
    o->leaf = mp->leaf, o->radius = opts->radius;
    o->min_points = opts->min_points, o->min_windows = opts->min_windows;
    o->k = opts->k, o->min_found = opts->min_found, o->reach = (int)reach_d;
    return DSI_OK;
}

dsi::MapKnnCells map_knn_cells_of(const dsi_map* mp) { return dsi::MapKnnCells{mp->knn_found.p, mp->knn_q.p, mp->knn_mean.p}; }

// what every entry point that reads the self query asks of the map
int check_self_query(const dsi_map* mp)
{
    REQUIRE(mp->knn_valid, DSI_ERR_INVALID,
            "no self query of the map as it stands: call dsx_map_knn (after the last reset, integrate call, merge, import or prune)");
    return DSI_OK;
}

// the threshold of the map's self query, then every cell's reason into mp->knn_reason and the counts into ctr
// (kMapKnnSelectCounters); synchronises
int map_knn_select_device(dsi_map* mp, const dsx_map_knn_selection_t* sel, unsigned long long* ctr, dsx_map_knn_select_info_t* thr)
{
    if (int rc = dsx_map_knn_threshold(mp->knn_moments[0], mp->knn_moments[1], reinterpret_cast<const uint64_t*>(&mp->knn_moments[2]),
                                       sel->std_mult, &thr->mu, &thr->sigma, &thr->T_q))
        return rc;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->knn_reason.reserve((size_t)1 << mp->cap_log2));
    dsi::MapKnn o;
    if (int rc = map_knn_of(mp, &mp->knn_opts, &o)) return rc;
    HIP_TRY(dsi::launch_map_knn_select(st, dsi::map_table_at(mp->block.p, mp->cap_log2), o, map_knn_cells_of(mp), sel->std_mult >= 0.0,
                                       (uint32_t)thr->T_q, mp->knn_reason.p, mp->knn_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->knn_ctr.p, dsi::kMapKnnSelectCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

void map_knn_select_info(const dsi_map* mp, const unsigned long long* ctr, const dsx_map_knn_select_info_t& thr, dsx_map_knn_select_info_t* info)
{
    if (!info) return;
    info->n_kept = ctr[0];
    info->n_cells = ctr[0];
    for (int r = 0; r < 3; ++r) {
        info->n_removed[r] = ctr[1 + r];
        info->n_cells += ctr[1 + r];
    }
    info->T_q = thr.T_q, info->mu = thr.mu, info->sigma = thr.sigma;
    info->capacity = (uint64_t)1 << mp->cap_log2;
}

}  // namespace

int dsx_map_knn_points(dsi_map_t* mp, const float* xyz_host, size_t stride_floats, size_t n, const dsx_map_knn_opts_t* opts,
                       uint64_t* keys_host, float* dist_host, uint8_t* found_host)
{
    if (int rc = check_knn_opts(opts)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(stride_floats == 3 || stride_floats == 4, DSI_ERR_INVALID, "stride_floats must be 3 or 4 (got %zu)", stride_floats);
    REQUIRE(n == 0 || xyz_host, DSI_ERR_INVALID, "xyz_host is null");
    REQUIRE(n <= ((size_t)1 << kMapMaxLog2), DSI_ERR_INVALID, "at most 2^%d points per call (got %zu)", kMapMaxLog2, n);
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    dsi::MapKnn o;
    if (int rc = map_knn_of(mp, opts, &o)) return rc;
    if (!n) return DSI_OK;
    if (int rc = set_device(mp->ctx)) return rc;
    hipStream_t st = mp->ctx->stream;
    const size_t rows = n * (size_t)o.k;
    HIP_TRY(mp->upload.reserve(n * stride_floats));
    if (keys_host) HIP_TRY(mp->knn_key_out.reserve(rows));
    if (dist_host) HIP_TRY(mp->knn_dist_out.reserve(rows));
    if (found_host) HIP_TRY(mp->knn_pt_found.reserve(n));
    HIP_TRY(hipMemcpyAsync(mp->upload.p, xyz_host, n * stride_floats * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(dsi::launch_map_knn_points(st, dsi::map_table_at(mp->block.p, mp->cap_log2), o, mp->upload.p, (uint32_t)stride_floats, (uint32_t)n,
                                       keys_host ? mp->knn_key_out.p : nullptr, dist_host ? mp->knn_dist_out.p : nullptr,
                                       found_host ? mp->knn_pt_found.p : nullptr));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "64-bit keys");
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->knn_key_out.p, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (dist_host) HIP_TRY(hipMemcpyAsync(dist_host, mp->knn_dist_out.p, rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (found_host) HIP_TRY(hipMemcpyAsync(found_host, mp->knn_pt_found.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_knn(dsi_map_t* mp, const dsx_map_knn_opts_t* opts, dsx_map_knn_info_t* info)
{
    if (int rc = check_knn_opts(opts)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    dsi::MapKnn o;
    if (int rc = map_knn_of(mp, opts, &o)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->knn_valid = mp->knn_select_valid = false;
    hipStream_t st = mp->ctx->stream;
    const size_t cap = (size_t)1 << mp->cap_log2;
    HIP_TRY(mp->knn_found.reserve(cap));
    HIP_TRY(mp->knn_q.reserve(cap));
    HIP_TRY(mp->knn_mean.reserve(cap));
    HIP_TRY(mp->knn_ctr.reserve(std::max(dsi::kMapKnnCounters, dsi::kMapKnnSelectCounters)));
    unsigned long long ctr[dsi::kMapKnnCounters] = {0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(dsi::launch_map_knn_self(st, dsi::map_table_at(mp->block.p, mp->cap_log2), o, map_knn_cells_of(mp), mp->knn_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->knn_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t sum_q2[2];
    dsi::knn_sum_q2(ctr[5], ctr[6], sum_q2);
    mp->knn_opts = *opts;
    mp->knn_moments[0] = ctr[2], mp->knn_moments[1] = ctr[4];
    mp->knn_moments[2] = sum_q2[0], mp->knn_moments[3] = sum_q2[1];
    mp->knn_valid = true;
    if (info) {
        info->n_cells = ctr[0];
        info->n_unqueried = ctr[1];
        info->n_scored = ctr[2];
        info->n_isolated = ctr[3];
        info->sum_q = ctr[4];
        info->sum_q2[0] = mp->knn_moments[2], info->sum_q2[1] = mp->knn_moments[3];
        info->reach = o.reach;
    }
    return DSI_OK;
}

int dsx_map_knn_threshold(uint64_t N, uint64_t sum_q, const uint64_t sum_q2[2], double std_mult, double* mu, double* sigma, uint64_t* T_q)
{
    REQUIRE(sum_q2, DSI_ERR_INVALID, "sum_q2 is null");
    REQUIRE(std::isfinite(std_mult), DSI_ERR_INVALID, "std_mult must be finite (got %g)", std_mult);
    double m = 0.0, sd = 0.0;
    uint64_t tq = 0;
    const dsi::KnnThresholdError e = dsi::knn_threshold_host(N, sum_q, sum_q2, std_mult, &m, &sd, &tq);
    REQUIRE(e != dsi::kKnnTooManyCells, DSI_ERR_INVALID, "N must be at most 2^%d (got %llu)", kMapMaxLog2, (unsigned long long)N);
    REQUIRE(e != dsi::kKnnMomentsTooLarge, DSI_ERR_INVALID, "moments too large for N = %llu cells with q <= 2^30", (unsigned long long)N);
    REQUIRE(e != dsi::kKnnNegativeVariance, DSI_ERR_INVALID, "N * sum_q2 < sum_q^2: no set of N values has these moments");
    if (mu) *mu = m;
    if (sigma) *sigma = sd;
    if (T_q) *T_q = tq;
    return DSI_OK;
}

int dsx_map_knn_select(dsi_map_t* mp, const dsx_map_knn_selection_t* sel, dsx_map_knn_select_info_t* info)
{
    if (int rc = check_knn_selection(sel)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_self_query(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->knn_select_valid = false;
    unsigned long long ctr[dsi::kMapKnnSelectCounters] = {0, 0, 0, 0};
    dsx_map_knn_select_info_t thr = {};
    if (int rc = map_knn_select_device(mp, sel, ctr, &thr)) return rc;
    mp->knn_select_valid = true;
    map_knn_select_info(mp, ctr, thr, info);
    return DSI_OK;
}

int dsx_map_knn_fetch(dsi_map_t* mp, uint64_t* keys_host, uint8_t* found_host, float* mean_host, uint32_t* q_host, uint8_t* reasons_host,
                      size_t capacity, size_t* count)
{
    REQUIRE(mp && count, DSI_ERR_INVALID, "null argument");
    if (int rc = check_self_query(mp)) return rc;
    REQUIRE(!reasons_host || mp->knn_select_valid, DSI_ERR_INVALID,
            "no selection on this self query: call dsx_map_knn_select before asking for reasons");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(mp, mp->knn_opts.min_points, mp->knn_opts.min_windows, capacity, count, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(mp->knn_found_out.reserve(total));
    HIP_TRY(mp->knn_mean_out.reserve(total));
    HIP_TRY(mp->knn_q_out.reserve(total));
    if (reasons_host) HIP_TRY(mp->knn_reason_out.reserve(total));
    HIP_TRY(dsi::launch_map_knn_gather(st, dsi::map_table_at(mp->block.p, mp->cap_log2), mp->knn_opts.min_points, mp->knn_opts.min_windows,
                                       map_knn_cells_of(mp), reasons_host ? mp->knn_reason.p : nullptr, mp->blk.p, mp->key_out.p,
                                       mp->knn_found_out.p, mp->knn_mean_out.p, mp->knn_q_out.p,
                                       reasons_host ? mp->knn_reason_out.p : nullptr));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (found_host) HIP_TRY(hipMemcpyAsync(found_host, mp->knn_found_out.p, total, hipMemcpyDeviceToHost, st));
    if (mean_host) HIP_TRY(hipMemcpyAsync(mean_host, mp->knn_mean_out.p, total * sizeof(float), hipMemcpyDeviceToHost, st));
    if (q_host) HIP_TRY(hipMemcpyAsync(q_host, mp->knn_q_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (reasons_host) HIP_TRY(hipMemcpyAsync(reasons_host, mp->knn_reason_out.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_prune_knn(dsi_map_t* mp, const dsx_map_knn_selection_t* sel, dsx_map_knn_select_info_t* info)
{
    if (int rc = check_knn_selection(sel)) return rc;
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_self_query(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->knn_select_valid = false;
    unsigned long long ctr[dsi::kMapKnnSelectCounters] = {0, 0, 0, 0};
    dsx_map_knn_select_info_t thr = {};
    if (int rc = map_knn_select_device(mp, sel, ctr, &thr)) return rc;
    mp->knn_select_valid = true;  // (the reasons are those of the map as it stands, should the rebuild fail to allocate)
    if (int rc = map_rebuild_kept(mp, mp->knn_reason.p, ctr[0], ctr[1] + ctr[2] + ctr[3] != 0, sel->shrink)) return rc;
    map_knn_select_info(mp, ctr, thr, info);
    return DSI_OK;
}

// ---- the map's local shape (include/dsi_map_pca.h; DESIGN.md 7j "Local shape") ----

namespace {

constexpr int kMapPcaMaxFound = 342;  // (2 * kMapKnnMaxReach + 1)^3 - 1
static_assert(dsi::kPcaMaxMembers == (uint32_t)kMapPcaMaxFound + 1, "the solver's bound on m is the largest neighbourhood's");

// the bounds of the options that need no map: decided without a device, before any handle is looked at
int check_pca_opts(const dsx_map_pca_opts_t* o)
{
    REQUIRE(o, DSI_ERR_INVALID, "opts is null");
    REQUIRE(o->k >= 0 && o->k <= dsi::kMapKnnMaxK, DSI_ERR_INVALID, "k must be in 0..%d (got %d)", dsi::kMapKnnMaxK, o->k);
    const int top = o->k == 0 ? kMapPcaMaxFound : std::max(o->k, 2);
    REQUIRE(o->min_found >= 2 && o->min_found <= top, DSI_ERR_INVALID, "min_found must be in 2..%d for k = %d (got %d)", top, o->k,
            o->min_found);
    REQUIRE(std::isfinite(o->radius) && o->radius > 0.0, DSI_ERR_INVALID, "radius must be finite and > 0 (got %g)", o->radius);
    REQUIRE(o->orient == 0 || o->orient == 1, DSI_ERR_INVALID, "orient must be 0 or 1 (got %d)", o->orient);
    REQUIRE(o->keep_moments == 0 || o->keep_moments == 1, DSI_ERR_INVALID, "keep_moments must be 0 or 1 (got %d)", o->keep_moments);
    REQUIRE(std::isfinite(o->viewpoint[0]) && std::isfinite(o->viewpoint[1]) && std::isfinite(o->viewpoint[2]), DSI_ERR_INVALID,
            "viewpoint must be finite (got %g %g %g)", o->viewpoint[0], o->viewpoint[1], o->viewpoint[2]);
    return DSI_OK;
}

int check_pca_selection(const dsx_map_pca_selection_t* s)
{
    REQUIRE(s, DSI_ERR_INVALID, "sel is null");
    REQUIRE(s->keep_labels >= 1u && s->keep_labels <= 7u, DSI_ERR_INVALID, "keep_labels must be a non-zero mask over the labels 1..3 (got %u)",
            s->keep_labels);
    REQUIRE(s->remove_sparse == 0 || s->remove_sparse == 1, DSI_ERR_INVALID, "remove_sparse must be 0 or 1 (got %d)", s->remove_sparse);
    REQUIRE(s->shrink == 0 || s->shrink == 1, DSI_ERR_INVALID, "shrink must be 0 or 1 (got %d)", s->shrink);
    return DSI_OK;
}

dsi::MapPcaCells map_pca_cells_of(const dsi_map* mp)
{
    return dsi::MapPcaCells{mp->pca_normal.p, mp->pca_tangent.p, mp->pca_eval.p, mp->pca_members.p,
                            mp->pca_label.p,  mp->pca_flags.p,   mp->pca_opts.keep_moments ? mp->pca_moments.p : nullptr};
}

// what every entry point that reads the pass asks of the map
int check_pca_pass(const dsi_map* mp)
{
    REQUIRE(mp->pca_valid, DSI_ERR_INVALID,
            "no local-shape pass of the map as it stands: call dsx_map_pca (after the last reset, integrate call, merge, import or prune)");
    return DSI_OK;
}

// every cell's reason into mp->pca_reason and the counts into ctr (kMapPcaSelectCounters); synchronises
int map_pca_select_device(dsi_map* mp, const dsx_map_pca_selection_t* sel, unsigned long long* ctr)
{
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->pca_reason.reserve((size_t)1 << mp->cap_log2));
    HIP_TRY(dsi::launch_map_pca_select(st, dsi::map_table_at(mp->block.p, mp->cap_log2), mp->pca_opts.min_points, mp->pca_opts.min_windows,
                                       mp->pca_label.p, sel->keep_labels, sel->remove_sparse, mp->pca_reason.p, mp->pca_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->pca_ctr.p, dsi::kMapPcaSelectCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

void map_pca_select_info(const dsi_map* mp, const unsigned long long* ctr, dsx_map_pca_select_info_t* info)
{
    if (!info) return;
    info->n_kept = ctr[0];
    info->n_cells = ctr[0];
    for (int r = 0; r < 3; ++r) {
        info->n_removed[r] = ctr[1 + r];
        info->n_cells += ctr[1 + r];
    }
    info->capacity = (uint64_t)1 << mp->cap_log2;
}

}  // namespace

int dsx_map_pca(dsi_map_t* mp, const dsx_map_pca_opts_t* opts, dsx_map_pca_info_t* info)
{
    if (int rc = check_pca_opts(opts)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    dsi::MapPca o;
    {
        dsx_map_knn_opts_t q = {};
        q.min_points = opts->min_points, q.min_windows = opts->min_windows;
        q.k = opts->k, q.min_found = opts->min_found, q.radius = opts->radius;
        if (int rc = map_knn_of(mp, &q, &o.q)) return rc;
    }
    o.quantum = mp->leaf * dsi::kPcaQuantumPerLeaf;
    for (int a = 0; a < 3; ++a) o.viewpoint[a] = opts->viewpoint[a];
    o.orient = opts->orient;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->pca_valid = mp->pca_select_valid = false;
    hipStream_t st = mp->ctx->stream;
    const size_t cap = (size_t)1 << mp->cap_log2;
    HIP_TRY(mp->pca_normal.reserve(3 * cap));
    HIP_TRY(mp->pca_tangent.reserve(3 * cap));
    HIP_TRY(mp->pca_eval.reserve(3 * cap));
    HIP_TRY(mp->pca_members.reserve(cap));
    HIP_TRY(mp->pca_label.reserve(cap));
    HIP_TRY(mp->pca_flags.reserve(cap));
    if (opts->keep_moments) HIP_TRY(mp->pca_moments.reserve(9 * cap));
    HIP_TRY(mp->pca_ctr.reserve(std::max(dsi::kMapPcaCounters, dsi::kMapPcaSelectCounters)));
    mp->pca_opts = *opts;
    unsigned long long ctr[dsi::kMapPcaCounters] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(dsi::launch_map_pca(st, dsi::map_table_at(mp->block.p, mp->cap_log2), o, map_pca_cells_of(mp), mp->pca_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->pca_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mp->pca_valid = true;
    if (info) {
        info->n_cells = ctr[0];
        info->n_unqueried = ctr[1];
        info->n_sparse = ctr[2];
        for (int l = 0; l < 3; ++l) info->n_label[l] = ctr[3 + l];
        info->n_normal_determined = ctr[6];
        info->n_tangent_determined = ctr[7];
        info->sum_members = ctr[8];
        info->reach = o.q.reach;
    }
    return DSI_OK;
}

int dsx_map_pca_fetch(dsi_map_t* mp, uint64_t* keys_host, float* normal_host, float* tangent_host, float* eval_host, uint16_t* members_host,
                      uint8_t* label_host, uint8_t* flags_host, int64_t* moments_host, uint8_t* reasons_host, size_t capacity, size_t* count)
{
    REQUIRE(mp && count, DSI_ERR_INVALID, "null argument");
    if (int rc = check_pca_pass(mp)) return rc;
    REQUIRE(!moments_host || mp->pca_opts.keep_moments, DSI_ERR_INVALID, "the pass kept no moments: call dsx_map_pca with keep_moments = 1");
    REQUIRE(!reasons_host || mp->pca_select_valid, DSI_ERR_INVALID,
            "no selection on this pass: call dsx_map_pca_select before asking for reasons");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(mp, mp->pca_opts.min_points, mp->pca_opts.min_windows, capacity, count, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(mp->pca_normal_out.reserve(3 * total));
    HIP_TRY(mp->pca_tangent_out.reserve(3 * total));
    HIP_TRY(mp->pca_eval_out.reserve(3 * total));
    HIP_TRY(mp->pca_members_out.reserve(total));
    HIP_TRY(mp->pca_label_out.reserve(total));
    HIP_TRY(mp->pca_flags_out.reserve(total));
    if (moments_host) HIP_TRY(mp->pca_moments_out.reserve(9 * total));
    if (reasons_host) HIP_TRY(mp->pca_reason_out.reserve(total));
    const dsi::MapPcaCells out{mp->pca_normal_out.p, mp->pca_tangent_out.p, mp->pca_eval_out.p, mp->pca_members_out.p,
                               mp->pca_label_out.p,  mp->pca_flags_out.p,   moments_host ? mp->pca_moments_out.p : nullptr};
    HIP_TRY(dsi::launch_map_pca_gather(st, dsi::map_table_at(mp->block.p, mp->cap_log2), mp->pca_opts.min_points, mp->pca_opts.min_windows,
                                       map_pca_cells_of(mp), reasons_host ? mp->pca_reason.p : nullptr, mp->blk.p, mp->key_out.p, out,
                                       reasons_host ? mp->pca_reason_out.p : nullptr));
    static_assert(sizeof(int64_t) == sizeof(long long), "64-bit moments");
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (normal_host) HIP_TRY(hipMemcpyAsync(normal_host, out.normal, 3 * total * sizeof(float), hipMemcpyDeviceToHost, st));
    if (tangent_host) HIP_TRY(hipMemcpyAsync(tangent_host, out.tangent, 3 * total * sizeof(float), hipMemcpyDeviceToHost, st));
    if (eval_host) HIP_TRY(hipMemcpyAsync(eval_host, out.eval, 3 * total * sizeof(float), hipMemcpyDeviceToHost, st));
    if (members_host) HIP_TRY(hipMemcpyAsync(members_host, out.members, total * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    if (label_host) HIP_TRY(hipMemcpyAsync(label_host, out.label, total, hipMemcpyDeviceToHost, st));
    if (flags_host) HIP_TRY(hipMemcpyAsync(flags_host, out.flags, total, hipMemcpyDeviceToHost, st));
    if (moments_host) HIP_TRY(hipMemcpyAsync(moments_host, out.moments, 9 * total * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (reasons_host) HIP_TRY(hipMemcpyAsync(reasons_host, mp->pca_reason_out.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_pca_solve(uint32_t m, const int64_t s[3], const int64_t ss[6], double quantum, int32_t orient, const double viewpoint[3],
                  const double p[3], dsx_pca_row_t* out)
{
    REQUIRE(s && ss && out, DSI_ERR_INVALID, "null argument");
    REQUIRE(std::isfinite(quantum) && quantum > 0.0, DSI_ERR_INVALID, "quantum must be finite and > 0 (got %g)", quantum);
    REQUIRE(orient == 0 || orient == 1, DSI_ERR_INVALID, "orient must be 0 or 1 (got %d)", orient);
    if (orient) {
        REQUIRE(viewpoint && p, DSI_ERR_INVALID, "orient needs viewpoint and p");
        for (int a = 0; a < 3; ++a)
            REQUIRE(std::isfinite(viewpoint[a]) && std::isfinite(p[a]), DSI_ERR_INVALID, "viewpoint and p must be finite");
    }
    dsi::PcaSolved r;
    const dsi::PcaSolveError e = dsi::pca_solve_host(m, s, ss, quantum, orient, viewpoint, p, &r);
    REQUIRE(e != dsi::kPcaBadMembers, DSI_ERR_INVALID, "m must be in 1..%u (got %u)", dsi::kPcaMaxMembers, m);
    REQUIRE(e != dsi::kPcaMomentsTooLarge, DSI_ERR_INVALID, "moments beyond what m = %u members with |D| <= %lld can sum to", m,
            (long long)dsi::kPcaMaxOffset);
    REQUIRE(e != dsi::kPcaNegativeVariance, DSI_ERR_INVALID, "m * ss < s^2 on an axis: no set of m offsets has these moments");
    for (int a = 0; a < 3; ++a) {
        out->normal_d[a] = r.normal[a], out->tangent_d[a] = r.tangent[a], out->lambda[a] = r.lambda[a];
        out->normal[a] = r.normal_f[a], out->tangent[a] = r.tangent_f[a], out->eval[a] = r.eval[a];
    }
    out->label = r.label, out->flags = r.flags;
    return DSI_OK;
}

int dsx_map_pca_select(dsi_map_t* mp, const dsx_map_pca_selection_t* sel, dsx_map_pca_select_info_t* info)
{
    if (int rc = check_pca_selection(sel)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_pca_pass(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->pca_select_valid = false;
    unsigned long long ctr[dsi::kMapPcaSelectCounters] = {0, 0, 0, 0};
    if (int rc = map_pca_select_device(mp, sel, ctr)) return rc;
    mp->pca_select_valid = true;
    map_pca_select_info(mp, ctr, info);
    return DSI_OK;
}

int dsx_map_prune_pca(dsi_map_t* mp, const dsx_map_pca_selection_t* sel, dsx_map_pca_select_info_t* info)
{
    if (int rc = check_pca_selection(sel)) return rc;
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_pca_pass(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->pca_select_valid = false;
    unsigned long long ctr[dsi::kMapPcaSelectCounters] = {0, 0, 0, 0};
    if (int rc = map_pca_select_device(mp, sel, ctr)) return rc;
    mp->pca_select_valid = true;  // (the reasons are those of the map as it stands, should the rebuild fail to allocate)
    if (int rc = map_rebuild_kept(mp, mp->pca_reason.p, ctr[0], ctr[1] + ctr[2] + ctr[3] != 0, sel->shrink)) return rc;
    map_pca_select_info(mp, ctr, info);
    return DSI_OK;
}

// ---- the map carved by free space (include/dsi_map_visibility.h; DESIGN.md 7j "Visibility") ----

namespace {

// the bounds of an observation: decided without a device, before any handle is looked at
int check_observation(const dsx_map_observation_t* o)
{
    REQUIRE(o, DSI_ERR_INVALID, "obs is null");
    if (int rc = check_depth_image(o->width, o->height, o->fx, o->fy, o->cx, o->cy, o->min_depth, o->max_depth)) return rc;
    REQUIRE(o->window >= 0 && o->window <= dsi::kMapObserveMaxWindow, DSI_ERR_INVALID, "window must be in 0..%d (got %d)",
            dsi::kMapObserveMaxWindow, o->window);
    REQUIRE(std::isfinite(o->abs_tol) && o->abs_tol >= 0.0 && std::isfinite(o->rel_tol) && o->rel_tol >= 0.0, DSI_ERR_INVALID,
            "abs_tol and rel_tol must be finite and >= 0 (got %g, %g)", o->abs_tol, o->rel_tol);
    return DSI_OK;
}

int check_visibility_selection(const dsx_map_visibility_selection_t* s)
{
    REQUIRE(s, DSI_ERR_INVALID, "sel is null");
    REQUIRE(s->min_through >= 1u, DSI_ERR_INVALID, "min_through must be >= 1 (got %u)", s->min_through);
    REQUIRE(s->shrink == 0 || s->shrink == 1, DSI_ERR_INVALID, "shrink must be 0 or 1 (got %d)", s->shrink);
    return DSI_OK;
}

dsi::MapTally map_tally_of(const dsi_map* mp) { return dsi::MapTally{mp->vis_seen.p, mp->vis_agree.p, mp->vis_through.p}; }

// what every entry point that reads the tally asks of the map
int check_visibility_tally(const dsi_map* mp)
{
    REQUIRE(mp->vis_valid, DSI_ERR_INVALID,
            "no visibility tally of the map as it stands: call dsx_map_observe (after the last reset, integrate call, merge, import, prune "
            "or dsx_map_visibility_clear)");
    return DSI_OK;
}

// one observation of a device depth image (mask_dev may be null) into the tally, which starts zeroed when there is none;
// the caller checked obs and set the device.  Synchronises.
int map_observe_device(dsi_map* mp, const float* depth_dev, const uint8_t* mask_dev, const dsx_map_observation_t* obs,
                       dsx_map_observe_info_t* info)
{
    REQUIRE(mp->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    REQUIRE(!mp->vis_valid || mp->vis_views < 0xffffffffull, DSI_ERR_INVALID, "at most 2^32 - 1 views per tally: clear it");
    hipStream_t st = mp->ctx->stream;
    const size_t cap = (size_t)1 << mp->cap_log2;
    mp->vis_select_valid = false;
    if (!mp->vis_valid) {
        HIP_TRY(mp->vis_seen.reserve(cap));
        HIP_TRY(mp->vis_agree.reserve(cap));
        HIP_TRY(mp->vis_through.reserve(cap));
        HIP_TRY(hipMemsetAsync(mp->vis_seen.p, 0, cap * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(mp->vis_agree.p, 0, cap * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(mp->vis_through.p, 0, cap * sizeof(uint32_t), st));
        mp->vis_views = 0;
    }
    mp->vis_valid = false;  // (until the kernel went through: a tally that a failed launch may have half written is none)
    HIP_TRY(mp->vis_ctr.reserve(std::max(dsi::kMapObserveCounters, dsi::kMapVisibilitySelectCounters)));
    dsi::MapObserve o;
    std::memcpy(o.T, obs->T_v_w, sizeof o.T);
    o.fx = obs->fx, o.fy = obs->fy, o.cx = obs->cx, o.cy = obs->cy;
    o.min_depth = obs->min_depth, o.max_depth = obs->max_depth;
    o.abs_tol = obs->abs_tol, o.rel_tol = obs->rel_tol;
    o.width = obs->width, o.height = obs->height, o.window = obs->window;
    unsigned long long ctr[dsi::kMapObserveCounters] = {0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(dsi::launch_map_observe(st, dsi::map_table_at(mp->block.p, mp->cap_log2), o, mp->leaf, depth_dev, mask_dev, map_tally_of(mp),
                                    mp->vis_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->vis_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mp->vis_valid = true;
    ++mp->vis_views;
    if (info) {
        info->n_clipped = ctr[0], info->n_outside = ctr[1], info->n_unseen = ctr[2];
        info->n_agree = ctr[3], info->n_through = ctr[4], info->n_behind = ctr[5];
        info->n_cells = ((ctr[0] + ctr[1]) + (ctr[2] + ctr[3])) + (ctr[4] + ctr[5]);
        info->n_valid_pixels = ctr[6];
        info->views = mp->vis_views;
    }
    return DSI_OK;
}

// every cell's reason into mp->vis_reason and the counts into ctr (kMapVisibilitySelectCounters); synchronises
int map_visibility_select_device(dsi_map* mp, const dsx_map_visibility_selection_t* sel, unsigned long long* ctr)
{
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->vis_reason.reserve((size_t)1 << mp->cap_log2));
    HIP_TRY(dsi::launch_map_visibility_select(st, dsi::map_table_at(mp->block.p, mp->cap_log2), map_tally_of(mp), sel->min_through,
                                              sel->agree_weight, mp->vis_reason.p, mp->vis_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, mp->vis_ctr.p, dsi::kMapVisibilitySelectCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

void map_visibility_select_info(const dsi_map* mp, const unsigned long long* ctr, dsx_map_visibility_select_info_t* info)
{
    if (!info) return;
    info->n_kept = ctr[0];
    info->n_removed = ctr[1];
    info->n_cells = ctr[0] + ctr[1];
    info->capacity = (uint64_t)1 << mp->cap_log2;
}

}  // namespace

int dsx_map_observe(dsi_map_t* mp, const float* depth_host, const uint8_t* mask_host, const dsx_map_observation_t* obs,
                    dsx_map_observe_info_t* info)
{
    if (int rc = check_observation(obs)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    REQUIRE(depth_host, DSI_ERR_INVALID, "depth_host is null");
    if (int rc = set_device(mp->ctx)) return rc;
    const size_t npix = (size_t)obs->width * (size_t)obs->height;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->vis_depth.reserve(npix));
    HIP_TRY(hipMemcpyAsync(mp->vis_depth.p, depth_host, npix * sizeof(float), hipMemcpyHostToDevice, st));
    if (mask_host) {
        HIP_TRY(mp->vis_mask.reserve(npix));
        HIP_TRY(hipMemcpyAsync(mp->vis_mask.p, mask_host, npix, hipMemcpyHostToDevice, st));
    }
    return map_observe_device(mp, mp->vis_depth.p, mask_host ? mp->vis_mask.p : nullptr, obs, info);
}

int dsx_map_observe_mapper(dsi_map_t* mp, dsi_mapper_t* m, const dsx_map_observation_t* obs, dsx_map_observe_info_t* info)
{
    if (int rc = check_observation(obs)) return rc;
    REQUIRE(mp && m, DSI_ERR_INVALID, "null argument");
    REQUIRE(mp->ctx == m->ctx, DSI_ERR_CONTEXT, "the map and the mapper live on different contexts");
    REQUIRE((size_t)m->geom.nz == m->planes_full.size(), DSI_ERR_INVALID,
            "a plane-sharded mapper holds no whole depth map of its own: the observation needs the whole arg-max");
    REQUIRE(m->filtered_valid, DSI_ERR_INVALID,
            "no filtered depth map on the device: call dsi_mapper_filter_depth_map or dsi_mapper_get_depth_map_from_dsi "
            "after the depth map was computed, or pass the maps to dsx_map_observe");
    REQUIRE(obs->width == m->geom.nx && obs->height == m->geom.ny, DSI_ERR_INVALID, "the observation is %d x %d, the mapper's depth map %d x %d",
            obs->width, obs->height, m->geom.nx, m->geom.ny);
    if (int rc = set_device(mp->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    return map_observe_device(mp, m->depth.p, m->mask.p, obs, info);
}

int dsx_map_visibility_clear(dsi_map_t* mp)
{
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    mp->vis_valid = mp->vis_select_valid = false;  // (the next observation zeroes the words)
    return DSI_OK;
}

int dsx_map_visibility_fetch(dsi_map_t* mp, uint64_t* keys_host, uint32_t* seen_host, uint32_t* agree_host, uint32_t* through_host,
                             uint8_t* reasons_host, size_t capacity, size_t* count)
{
    REQUIRE(mp && count, DSI_ERR_INVALID, "null argument");
    if (int rc = check_visibility_tally(mp)) return rc;
    REQUIRE(!reasons_host || mp->vis_select_valid, DSI_ERR_INVALID,
            "no selection on this tally: call dsx_map_visibility_select before asking for reasons");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(mp, 1, 1, capacity, count, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(mp->vis_seen_out.reserve(total));
    HIP_TRY(mp->vis_agree_out.reserve(total));
    HIP_TRY(mp->vis_through_out.reserve(total));
    if (reasons_host) HIP_TRY(mp->vis_reason_out.reserve(total));
    const dsi::MapTally out{mp->vis_seen_out.p, mp->vis_agree_out.p, mp->vis_through_out.p};
    HIP_TRY(dsi::launch_map_visibility_gather(st, dsi::map_table_at(mp->block.p, mp->cap_log2), map_tally_of(mp),
                                              reasons_host ? mp->vis_reason.p : nullptr, mp->blk.p, mp->key_out.p, out,
                                              reasons_host ? mp->vis_reason_out.p : nullptr));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (seen_host) HIP_TRY(hipMemcpyAsync(seen_host, out.seen, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (agree_host) HIP_TRY(hipMemcpyAsync(agree_host, out.agree, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (through_host) HIP_TRY(hipMemcpyAsync(through_host, out.through, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (reasons_host) HIP_TRY(hipMemcpyAsync(reasons_host, mp->vis_reason_out.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_visibility_select(dsi_map_t* mp, const dsx_map_visibility_selection_t* sel, dsx_map_visibility_select_info_t* info)
{
    if (int rc = check_visibility_selection(sel)) return rc;  // (first: the bounds can be exercised with no map at hand)
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_visibility_tally(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->vis_select_valid = false;
    unsigned long long ctr[dsi::kMapVisibilitySelectCounters] = {0, 0};
    if (int rc = map_visibility_select_device(mp, sel, ctr)) return rc;
    mp->vis_select_valid = true;
    map_visibility_select_info(mp, ctr, info);
    return DSI_OK;
}

int dsx_map_prune_visibility(dsi_map_t* mp, const dsx_map_visibility_selection_t* sel, dsx_map_visibility_select_info_t* info)
{
    if (int rc = check_visibility_selection(sel)) return rc;
    REQUIRE(mp, DSI_ERR_INVALID, "map is null");
    if (int rc = check_visibility_tally(mp)) return rc;
    if (int rc = set_device(mp->ctx)) return rc;
    mp->vis_select_valid = false;
    unsigned long long ctr[dsi::kMapVisibilitySelectCounters] = {0, 0};
    if (int rc = map_visibility_select_device(mp, sel, ctr)) return rc;
    mp->vis_select_valid = true;  // (the reasons are those of the map as it stands, should the rebuild fail to allocate)
    if (int rc = map_rebuild_kept(mp, mp->vis_reason.p, ctr[0], ctr[1] != 0, sel->shrink)) return rc;
    map_visibility_select_info(mp, ctr, info);
    return DSI_OK;
}

// ---- merging maps and moving their state (include/dsi_map_merge.h; DESIGN.md 7j "Merging") ----

namespace {

// the source of a merge, whichever table holds it: another map's, or the scratch table an import built
struct MapMergeSource {
    dsi::MapTable t;
    uint64_t cells, calls, accepted, rejected;
};

// the bounds that the two maps' states must meet together: judged on the host, before dst is touched
int map_merge_check(const dsi_map* dst, uint64_t cells, uint64_t calls, uint64_t accepted)
{
    REQUIRE(dst->host_ctr[3] == 0, DSI_ERR_INVALID, "dst's table overflowed in an earlier call: reset the map");
    REQUIRE(calls <= 0xffffffffull && dst->calls + calls <= 0xffffffffull, DSI_ERR_INVALID,
            "calls: %llu + %llu integrate calls exceed 2^32 - 1 (stamps are 32 bits wide): dst is unchanged",
            (unsigned long long)dst->calls, (unsigned long long)calls);
    REQUIRE(accepted <= 0xffffffffull && dst->host_ctr[1] + accepted <= 0xffffffffull, DSI_ERR_INVALID,
            "accepted: %llu + %llu accepted points exceed 2^32 - 1 (a cell's n is 32 bits wide): dst is unchanged", dst->host_ctr[1],
            (unsigned long long)accepted);
    REQUIRE(cells <= ((uint64_t)1 << kMapMaxLog2) && (dst->host_ctr[0] + cells) * 4 <= ((uint64_t)3 << kMapMaxLog2), DSI_ERR_INVALID,
            "%llu cells + %llu cells need more than 2^%d slots: dst is unchanged", dst->host_ctr[0], (unsigned long long)cells, kMapMaxLog2);
    return DSI_OK;
}

// the one routine behind dsx_map_merge and dsx_map_import: dst grown for src's cells, then src appended; synchronises
int map_merge_apply(dsi_map* dst, const MapMergeSource& src, dsx_map_merge_info_t* info)
{
    hipStream_t st = dst->ctx->stream;
    HIP_TRY(dst->merge_ctr.reserve(dsi::kMapMergeCounters));
    const uint64_t growths_before = dst->growths;
    if (int rc = map_grow_for(dst, (size_t)src.cells)) return rc;                 // (a failed allocation leaves dst as it is)
    map_changed(dst);
    unsigned long long mctr[dsi::kMapMergeCounters] = {0, 0};
    HIP_TRY(dsi::launch_map_merge(st, src.t, dsi::map_table_at(dst->block.p, dst->cap_log2), (uint32_t)dst->calls, src.accepted,
                                  src.rejected, dst->ctr.p, dst->merge_ctr.p));
    HIP_TRY(hipMemcpyAsync(dst->host_ctr, dst->ctr.p, sizeof dst->host_ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mctr, dst->merge_ctr.p, sizeof mctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    dst->calls += src.calls;
    REQUIRE(dst->host_ctr[3] == 0 && mctr[0] + mctr[1] == src.cells, DSI_ERR_HIP,
            "the merge placed %llu of %llu cells (%llu found the table full): an engine bug, the map is unusable", mctr[0] + mctr[1],
            (unsigned long long)src.cells, dst->host_ctr[3]);
    if (info) {
        info->n_src_cells = src.cells;
        info->n_new = mctr[0];
        info->n_common = mctr[1];
        info->capacity = (uint64_t)1 << dst->cap_log2;
        info->growths = dst->growths - growths_before;
    }
    return DSI_OK;
}

}  // namespace

int dsx_map_export(dsi_map_t* mp, dsx_map_state_t* state, uint64_t* keys_host, uint32_t* n_host, uint64_t* sums_host,
                   uint32_t* windows_host, uint32_t* stamp_host, size_t capacity, size_t* count)
{
    REQUIRE(mp && count, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(mp->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_count_device(mp, 0, 0, &total)) return rc;
    if (state) {
        state->leaf = mp->leaf;
        state->n_cells = total;
        state->calls = mp->calls;
        state->accepted = mp->host_ctr[1];
        state->rejected = mp->host_ctr[2];
    }
    *count = total;
    REQUIRE(capacity >= total, DSI_ERR_INVALID, "capacity of %zu cells is too small: %zu needed", capacity, total);
    if (!total || !(keys_host || n_host || sums_host || windows_host || stamp_host)) return DSI_OK;
    hipStream_t st = mp->ctx->stream;
    HIP_TRY(mp->key_out.reserve(total));
    HIP_TRY(mp->n_out.reserve(total));
    HIP_TRY(mp->sums_out.reserve(3 * total));
    HIP_TRY(mp->w_out.reserve(total));
    HIP_TRY(mp->stamp_out.reserve(total));
    HIP_TRY(dsi::launch_map_export(st, dsi::map_table_at(mp->block.p, mp->cap_log2), mp->blk.p, mp->key_out.p, mp->n_out.p, mp->sums_out.p,
                                   mp->w_out.p, mp->stamp_out.p));
    if (keys_host) HIP_TRY(hipMemcpyAsync(keys_host, mp->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (n_host) HIP_TRY(hipMemcpyAsync(n_host, mp->n_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (sums_host) HIP_TRY(hipMemcpyAsync(sums_host, mp->sums_out.p, 3 * total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (windows_host) HIP_TRY(hipMemcpyAsync(windows_host, mp->w_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (stamp_host) HIP_TRY(hipMemcpyAsync(stamp_host, mp->stamp_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_map_merge(dsi_map_t* dst, dsi_map_t* src, dsx_map_merge_info_t* info)
{
    REQUIRE(dst, DSI_ERR_INVALID, "dst is null");
    REQUIRE(src, DSI_ERR_INVALID, "src is null");
    REQUIRE(dst != src, DSI_ERR_INVALID, "same map: dst and src are one map");
    REQUIRE(dst->ctx == src->ctx, DSI_ERR_CONTEXT, "contexts: dst and src live on different contexts, export and import instead");
    REQUIRE(std::memcmp(&dst->leaf, &src->leaf, sizeof(double)) == 0, DSI_ERR_INVALID, "leaf: dst has %.17g, src has %.17g", dst->leaf,
            src->leaf);
    REQUIRE(src->host_ctr[3] == 0, DSI_ERR_INVALID, "src's table overflowed in an earlier call");
    if (int rc = map_merge_check(dst, src->host_ctr[0], src->calls, src->host_ctr[1])) return rc;
    if (int rc = set_device(dst->ctx)) return rc;
    const MapMergeSource s{dsi::map_table_at(src->block.p, src->cap_log2), src->host_ctr[0], src->calls, src->host_ctr[1], src->host_ctr[2]};
    return map_merge_apply(dst, s, info);
}

int dsx_map_import(dsi_map_t* dst, const dsx_map_state_t* state, const uint64_t* keys_host, const uint32_t* n_host,
                   const uint64_t* sums_host, const uint32_t* windows_host, const uint32_t* stamp_host, dsx_map_merge_info_t* info)
{
    REQUIRE(dst, DSI_ERR_INVALID, "dst is null");
    REQUIRE(state, DSI_ERR_INVALID, "state is null");
    REQUIRE(std::isfinite(state->leaf) && state->leaf > 0.0, DSI_ERR_INVALID, "leaf: must be finite and > 0 (got %g)", state->leaf);
    const uint64_t m = state->n_cells;
    REQUIRE(m <= ((uint64_t)1 << kMapMaxLog2), DSI_ERR_INVALID, "n_cells: at most 2^%d cells (got %llu)", kMapMaxLog2, (unsigned long long)m);
    if (m) {
        REQUIRE(keys_host, DSI_ERR_INVALID, "keys is null");
        REQUIRE(n_host, DSI_ERR_INVALID, "n is null");
        REQUIRE(sums_host, DSI_ERR_INVALID, "sums is null");
        REQUIRE(windows_host, DSI_ERR_INVALID, "windows is null");
        REQUIRE(stamp_host, DSI_ERR_INVALID, "stamp is null");
    }
    REQUIRE(std::memcmp(&dst->leaf, &state->leaf, sizeof(double)) == 0, DSI_ERR_INVALID, "leaf: dst has %.17g, the state has %.17g",
            dst->leaf, state->leaf);
    if (int rc = map_merge_check(dst, m, state->calls, state->accepted)) return rc;
    if (int rc = set_device(dst->ctx)) return rc;
    hipStream_t st = dst->ctx->stream;
    // the scratch table: the smallest that holds m cells at 3/4 load; it and the uploads live for this call
    uint32_t want = kMapMinLog2;
    while (m * 4 > ((uint64_t)3 << want)) ++want;
    DevBuf<unsigned char> scratch;
    DevBuf<unsigned long long> keys, sums, ctr;
    DevBuf<uint32_t> n, windows, stamp;
    hipError_t e = scratch.reserve(dsi::map_table_bytes(want));
    if (e == hipSuccess) e = ctr.reserve(dsi::kMapImportCounters);
    if (e == hipSuccess && m) e = keys.reserve(m);
    if (e == hipSuccess && m) e = sums.reserve(3 * m);
    if (e == hipSuccess && m) e = n.reserve(m);
    if (e == hipSuccess && m) e = windows.reserve(m);
    if (e == hipSuccess && m) e = stamp.reserve(m);
    if (e != hipSuccess)
        return fail(DSI_ERR_HIP, "a scratch table of 2^%u slots for %llu cells could not be allocated (%s): dst is unchanged", want,
                    (unsigned long long)m, hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(scratch.p, 0, dsi::map_table_bytes(want), st));
    if (m) {
        HIP_TRY(hipMemcpyAsync(keys.p, keys_host, m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sums.p, sums_host, 3 * m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(n.p, n_host, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(windows.p, windows_host, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(stamp.p, stamp_host, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    const dsi::MapTable table = dsi::map_table_at(scratch.p, want);
    unsigned long long c[dsi::kMapImportCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(dsi::launch_map_import_build(st, keys.p, n.p, sums.p, windows.p, stamp.p, (uint32_t)m, (uint32_t)state->calls, table, ctr.p));
    HIP_TRY(hipMemcpyAsync(c, ctr.p, sizeof c, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    REQUIRE(c[0] == 0, DSI_ERR_INVALID, "keys: %llu cells have the key 0 or a packed coordinate outside [1, 2^21 - 3]", c[0]);
    REQUIRE(c[1] == 0, DSI_ERR_INVALID, "keys: %llu duplicate keys", c[1]);
    REQUIRE(c[2] == 0, DSI_ERR_INVALID, "n: %llu cells have n == 0", c[2]);
    REQUIRE(c[3] == 0, DSI_ERR_INVALID, "windows: %llu cells have windows == 0, windows > n or windows > stamp", c[3]);
    REQUIRE(c[4] == 0, DSI_ERR_INVALID, "stamp: %llu cells have stamp == 0 or stamp > calls (%llu)", c[4], (unsigned long long)state->calls);
    REQUIRE(c[5] == 0, DSI_ERR_INVALID, "sums: %llu cells have a sum above n * 2^32", c[5]);
    REQUIRE(c[6] == 0, DSI_ERR_HIP, "the scratch table ran full (%llu cells lost): an engine bug; dst is unchanged", c[6]);
    REQUIRE(state->accepted >= c[7], DSI_ERR_INVALID, "accepted: the state names %llu accepted points, its cells hold %llu",
            (unsigned long long)state->accepted, c[7]);
    const MapMergeSource s{table, m, state->calls, state->accepted, state->rejected};
    return map_merge_apply(dst, s, info);
}

// ---- aligning maps (include/dsi_map_align.h; DESIGN.md 7j "Aligning") ----

namespace {

int check_finite_pose(const double T[12], const char* name)
{
    REQUIRE(T, DSI_ERR_INVALID, "%s is null", name);
    for (int k = 0; k < 12; ++k) REQUIRE(std::isfinite(T[k]), DSI_ERR_INVALID, "%s[%d] is not finite (%g)", name, k, T[k]);
    return DSI_OK;
}

// what a step needs of its arguments, in the order the header gives: opts and T without a map at hand, then the maps
int check_align_step(const dsi_map* a, const dsi_map* b, const dsx_map_align_opts_t* opts, const double T[12], const char* T_name)
{
    REQUIRE(opts, DSI_ERR_INVALID, "opts is null");
    REQUIRE(std::isfinite(opts->radius) && opts->radius > 0.0, DSI_ERR_INVALID, "radius must be finite and > 0 (got %g)", opts->radius);
    if (int rc = check_finite_pose(T, T_name)) return rc;
    REQUIRE(a && b, DSI_ERR_INVALID, "map is null");
    REQUIRE(a->ctx == b->ctx, DSI_ERR_CONTEXT, "the maps live on different contexts");
    const double reach_d = std::ceil(opts->radius / b->leaf);
    REQUIRE(reach_d >= 1.0 && reach_d <= (double)dsi::kMapCompareMaxReach, DSI_ERR_INVALID,
            "reach = ceil(radius / leaf_b) must be in 1..%d (radius %g, leaf_b %g)", dsi::kMapCompareMaxReach, opts->radius, b->leaf);
    REQUIRE(a->host_ctr[3] == 0 && b->host_ctr[3] == 0, DSI_ERR_INVALID, "a map's table overflowed in an earlier call: reset the map");
    return DSI_OK;
}

int check_align_loop(const dsx_map_align_opts_t* opts)
{
    REQUIRE(opts, DSI_ERR_INVALID, "opts is null");
    REQUIRE(opts->max_iterations >= 1 && opts->max_iterations <= 64, DSI_ERR_INVALID, "max_iterations must be in 1..64 (got %d)",
            opts->max_iterations);
    REQUIRE(std::isfinite(opts->eps_rot) && opts->eps_rot >= 0.0, DSI_ERR_INVALID, "eps_rot must be finite and >= 0 (got %g)", opts->eps_rot);
    REQUIRE(std::isfinite(opts->eps_trans) && opts->eps_trans >= 0.0, DSI_ERR_INVALID, "eps_trans must be finite and >= 0 (got %g)",
            opts->eps_trans);
    return DSI_OK;
}

// one pass on the device (the arguments are checked, the device is set); synchronises for the moment block
int map_align_step_device(dsi_map* a, dsi_map* b, const dsx_map_align_opts_t* opts, const double T[12], dsx_map_align_moments_t* m)
{
    hipStream_t st = a->ctx->stream;
    a->align_valid = false;
    HIP_TRY(a->align_key.reserve((size_t)1 << a->cap_log2));
    HIP_TRY(a->align_dist.reserve((size_t)1 << a->cap_log2));
    HIP_TRY(a->align_ctr.reserve(dsi::kMapAlignCounters));
    dsi::MapAlign o;
    std::memcpy(o.T, T, sizeof o.T);
    o.leaf_a = a->leaf, o.leaf_b = b->leaf, o.radius = opts->radius, o.quantum = b->leaf * 0x1p-10;
    o.min_points_a = opts->min_points_a, o.min_windows_a = opts->min_windows_a;
    o.min_points_b = opts->min_points_b, o.min_windows_b = opts->min_windows_b;
    o.reach = (int)std::ceil(opts->radius / b->leaf);
    unsigned long long ctr[dsi::kMapAlignCounters];
    HIP_TRY(dsi::launch_map_align_step(st, dsi::map_table_at(a->block.p, a->cap_log2), dsi::map_table_at(b->block.p, b->cap_log2), o,
                                       a->align_key.p, a->align_dist.p, a->align_ctr.p));
    HIP_TRY(hipMemcpyAsync(ctr, a->align_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    a->align_min_points = opts->min_points_a;
    a->align_min_windows = opts->min_windows_a;
    a->align_valid = true;
    m->n_cells = ctr[0] + ctr[1];
    m->n_matched = ctr[0];
    m->n_unmatched = ctr[1];
    for (int k = 0; k < 3; ++k) m->su[k] = (int64_t)ctr[2 + k], m->sv[k] = (int64_t)ctr[5 + k];
    for (int k = 0; k < 9; ++k) m->suv_hi[k] = (int64_t)ctr[8 + k], m->suv_lo[k] = ctr[17 + k];
    m->e2 = ctr[26];
    m->quantum = o.quantum;
    m->reach = o.reach;
    m->reserved = 0;
    return DSI_OK;
}

}  // namespace

int dsx_map_align_step(dsi_map_t* a, dsi_map_t* b, const dsx_map_align_opts_t* opts, const double T[12], dsx_map_align_moments_t* moments)
{
    if (int rc = check_align_step(a, b, opts, T, "T")) return rc;
    REQUIRE(moments, DSI_ERR_INVALID, "moments is null");
    if (int rc = set_device(a->ctx)) return rc;
    return map_align_step_device(a, b, opts, T, moments);
}

int dsx_map_align_fetch(dsi_map_t* a, uint64_t* keys_a, uint64_t* keys_b, float* dist, size_t capacity, size_t* n)
{
    REQUIRE(a && n, DSI_ERR_INVALID, "null argument");
    REQUIRE(a->align_valid, DSI_ERR_INVALID,
            "no alignment step of the map as it stands: call dsx_map_align_step (after the last dsi_map_reset, integrate call, merge or prune)");
    if (int rc = set_device(a->ctx)) return rc;
    size_t total = 0;
    if (int rc = map_fetch_count(a, a->align_min_points, a->align_min_windows, capacity, n, &total)) return rc;
    if (!total) return DSI_OK;
    hipStream_t st = a->ctx->stream;
    HIP_TRY(a->key_out.reserve(total));
    HIP_TRY(a->align_key_out.reserve(total));
    HIP_TRY(a->align_dist_out.reserve(total));
    HIP_TRY(dsi::launch_map_align_gather(st, dsi::map_table_at(a->block.p, a->cap_log2), a->align_min_points, a->align_min_windows,
                                         a->align_key.p, a->align_dist.p, a->blk.p, a->key_out.p, a->align_key_out.p, a->align_dist_out.p));
    if (keys_a) HIP_TRY(hipMemcpyAsync(keys_a, a->key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (keys_b) HIP_TRY(hipMemcpyAsync(keys_b, a->align_key_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (dist) HIP_TRY(hipMemcpyAsync(dist, a->align_dist_out.p, total * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DSI_OK;
}

int dsx_pose_compose(const double A[12], const double B[12], double out[12])
{
    REQUIRE(A && B && out, DSI_ERR_INVALID, "null argument");
    double r[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
        r[4 * i + 3] = ((A[4 * i] * B[3] + A[4 * i + 1] * B[7]) + A[4 * i + 2] * B[11]) + A[4 * i + 3];
    }
    std::memcpy(out, r, sizeof r);
    return DSI_OK;
}

int dsx_map_align_solve(const dsx_map_align_moments_t* m, double T_delta[12], dsx_map_align_solve_info_t* info)
{
    REQUIRE(m && T_delta, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->n_matched >= 3, DSI_ERR_INVALID, "n_matched: %llu matched pairs, a rigid motion needs at least 3",
            (unsigned long long)m->n_matched);
    REQUIRE(std::isfinite(m->quantum) && m->quantum > 0.0, DSI_ERR_INVALID, "quantum must be finite and > 0 (got %g)", m->quantum);
    const double nd = (double)m->n_matched;
    const double scale = (m->quantum * m->quantum) / (nd * nd);
    double S[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const __int128 sum_p = (__int128)m->suv_hi[3 * r + c] * ((__int128)1 << 32) + (__int128)m->suv_lo[3 * r + c];
            const __int128 centred = (__int128)m->n_matched * sum_p - (__int128)m->su[r] * (__int128)m->sv[c];
            S[3 * r + c] = (double)centred * scale;
        }
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 16; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    int i0 = 0;
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > A[i0][i0]) i0 = k;
    int i1 = i0 == 0 ? 1 : 0;
    for (int k = 0; k < 4; ++k)
        if (k != i0 && A[k][k] > A[i1][i1]) i1 = k;
    const double l0 = A[i0][i0], l1 = A[i1][i1];
    const double size = ((std::fabs(A[0][0]) + std::fabs(A[1][1])) + std::fabs(A[2][2])) + std::fabs(A[3][3]);
    const double rms = std::sqrt(((double)m->e2 * (m->quantum * m->quantum)) / nd);
    if (!(l0 - l1 > 0x1p-26 * size)) {
        if (info) {
            info->n_matched = m->n_matched;
            info->rms = rms;
            info->angle = info->trans = 0.0;
            info->lambda[0] = l0, info->lambda[1] = l1;
        }
        return fail(DSI_ERR_INVALID,
                    "degenerate: the largest eigenvalue %.17g is not separated from the second %.17g (collinear or coincident pairs)", l0, l1);
    }
    double w = V[0][i0], x = V[1][i0], y = V[2][i0], z = V[3][i0];
    const double norm = std::sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / norm, x = x / norm, y = y / norm, z = z / norm;
    if (w < 0.0) w = -w, x = -x, y = -y, z = -z;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    double mu[3], mv[3], t[3];
    for (int r = 0; r < 3; ++r) mu[r] = ((double)m->su[r] / nd) * m->quantum, mv[r] = ((double)m->sv[r] / nd) * m->quantum;
    for (int r = 0; r < 3; ++r) t[r] = mv[r] - ((R[3 * r] * mu[0] + R[3 * r + 1] * mu[1]) + R[3 * r + 2] * mu[2]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T_delta[4 * r + c] = R[3 * r + c];
        T_delta[4 * r + 3] = t[r];
    }
    if (info) {
        info->n_matched = m->n_matched;
        info->rms = rms;
        info->angle = 2.0 * std::atan2(std::sqrt((x * x + y * y) + z * z), w);
        info->trans = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        info->lambda[0] = l0, info->lambda[1] = l1;
    }
    return DSI_OK;
}

int dsx_map_align(dsi_map_t* a, dsi_map_t* b, const dsx_map_align_opts_t* opts, const double T_init[12], double T_out[12],
                  dsx_map_align_info_t* info)
{
    if (int rc = check_align_loop(opts)) return rc;
    REQUIRE(T_out, DSI_ERR_INVALID, "T_out is null");
    if (int rc = check_align_step(a, b, opts, T_init, "T_init")) return rc;
    if (int rc = set_device(a->ctx)) return rc;
    double T[12];
    std::memcpy(T, T_init, sizeof T);
    dsx_map_align_info_t out{};
    int rc = DSI_OK;
    for (int it = 0; it < opts->max_iterations; ++it) {
        dsx_map_align_moments_t m;
        if ((rc = map_align_step_device(a, b, opts, T, &m)) != DSI_OK) break;
        out.iterations = it + 1;
        out.reach = m.reach;
        out.n_cells = m.n_cells;
        if (it == 0) out.n_matched_first = m.n_matched;
        out.n_matched_last = m.n_matched;
        if (m.n_matched < opts->min_matched) {
            out.stopped = 1;
            rc = fail(DSI_ERR_INVALID, "round %d matched %llu cells, fewer than min_matched = %llu: T_out is the last good pose", it + 1,
                      (unsigned long long)m.n_matched, (unsigned long long)opts->min_matched);
            break;
        }
        double T_delta[12];
        dsx_map_align_solve_info_t si;
        if ((rc = dsx_map_align_solve(&m, T_delta, &si)) != DSI_OK) {
            out.stopped = 2;
            break;
        }
        if (it == 0) out.rms_first = si.rms;
        out.rms_last = si.rms;
        out.angle_last = si.angle, out.trans_last = si.trans;
        dsx_pose_compose(T_delta, T, T);
        if (si.angle <= opts->eps_rot && si.trans <= opts->eps_trans) {
            out.converged = 1;
            break;
        }
    }
    std::memcpy(T_out, T, sizeof T);
    if (info) *info = out;
    return rc;
}

int dsx_map_integrate_map(dsi_map_t* dst, dsi_map_t* src, const double T[12], uint32_t min_points, uint32_t min_windows,
                          uint64_t* n_points, uint64_t* n_rejected)
{
    REQUIRE(dst, DSI_ERR_INVALID, "dst is null");
    REQUIRE(src, DSI_ERR_INVALID, "src is null");
    if (int rc = check_finite_pose(T, "T")) return rc;
    REQUIRE(dst != src, DSI_ERR_INVALID, "same map: dst and src are one map");
    REQUIRE(dst->ctx == src->ctx, DSI_ERR_CONTEXT, "contexts: dst and src live on different contexts");
    REQUIRE(src->host_ctr[3] == 0, DSI_ERR_INVALID, "src's table overflowed in an earlier call");
    REQUIRE(dst->host_ctr[3] == 0, DSI_ERR_INVALID, "the map's table overflowed in an earlier call: reset the map");
    if (int rc = set_device(dst->ctx)) return rc;
    size_t accepted = 0, rejected = 0;
    if (int rc = map_integrate_call(
            dst, (size_t)src->host_ctr[0],
            [&](uint32_t serial, const dsi::MapTable& t) {
                return dsi::launch_map_integrate_map(dst->ctx->stream, dsi::map_table_at(src->block.p, src->cap_log2), min_points,
                                                     min_windows, src->leaf, T, dst->leaf, serial, t, dst->ctr.p);
            },
            &accepted, &rejected))
        return rc;
    if (n_points) *n_points = (uint64_t)accepted + (uint64_t)rejected;
    if (n_rejected) *n_rejected = rejected;
    return DSI_OK;
}

int dsi_mapper_last_vote_info(const dsi_mapper_t* m, dsi_vote_info_t* info)
{
    REQUIRE(m && info, DSI_ERR_INVALID, "null argument");
    *info = m->info;
    return DSI_OK;
}

/* Diagnostics of the voting kernel's work on one batch (bench.py: roofline.achieved / frac_issued).  Votes the batch
 * twice: once with every merged record counted once -- the sum of that DSI is the number of RECORDS the voting kernel
 * accepted, a quarter of the LDS atomics it issues -- and once as dsi_mapper_evaluate_batch does, whose DSI sums to the
 * accepted event-planes (the four bilinear weights of a vote sum to 1) and is what the mapper's grid holds afterwards.
 * The switch that makes the first pass is internal: no caller can leave it on.  Synchronises. */
int dsi_mapper_vote_statistics(dsi_mapper_t* m, const dsi_batch_t* batch, double* accepted_event_planes, double* accepted_records)
{
    REQUIRE(m && batch && accepted_event_planes && accepted_records, DSI_ERR_INVALID, "null argument");
    std::vector<float> host(m->grid->n);
    double sums[2] = {0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass) {
        m->unit_multiplicity = pass == 0 ? 1 : 0;
        const int rc = dsi_mapper_evaluate_batch(m, batch);
        m->unit_multiplicity = 0;
        if (rc != DSI_OK) return rc;
        if (int rc2 = dsi_grid_download(m->grid, host.data())) return rc2;
        double t = 0.0;
        for (float v : host) t += (double)v;
        sums[pass] = t;
    }
    *accepted_records = sums[0];
    *accepted_event_planes = sums[1];
    return DSI_OK;
}

int dsi_build_flavour(void)
{
#ifdef DSI_TIMING_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

#ifdef DSI_TIMING_EXPERIMENTS
/* Everything from here to the #endif exists only in the EXPERIMENTS flavour of the library
 * (libdsi_engine_experiments.so, `python -m dvs_mcemvs_amd.build --experiments`): hooks of the timing experiments and
 * development tools quoted in NOTEBOOK.md.  The production library exports no dsi_test_* symbol (tests/test_abi.py). */
/* test hook (not in the public header): packets per pass of the voting streams, as a power of two (0 = automatic) */
DSI_API int dsi_test_pass_lg(dsi_mapper_t* m, int lg)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    m->want_pass_lg = lg;
    return DSI_OK;
}

/* test hook (not in the public header): the fixed cost of one phase of the fused kernel in record units (the
 * balanced partition's only tunable); < 0 switches the balancing off (equal pair counts per workgroup) */
DSI_API int dsi_test_fused_fixed_cost(dsi_mapper_t* m, int records)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    m->fused_fixed_cost = records;
    return DSI_OK;
}

/* test hook (not in the public header): the workgroup count of the fused kernels (k_vote_fuse_argmax, its two-per-CU
 * sibling at twice the count, k_vote_fuse_argmax_alg2), of the balanced partition and of the trace, for every later call of
 * this process: a multiple of 8 that is >= 8 -- a CPX / QPX partition of the device has 32 / 64 CUs --, 0 = the device's own */
DSI_API int dsi_test_fused_grid_blocks(int blocks)
{
    REQUIRE(dsi::fused_grid_blocks_force(blocks), DSI_ERR_INVALID, "a multiple of 8 in [8, 4096], or 0 (got %d)", blocks);
    return DSI_OK;
}

/* test hook (not in the public header): what the last launch of a DSI-less kernel in this process was -- its grid size,
 * bp.interleave (0 pieces, 1 in turn, 2 dealt), the kernel (1 k_vote_fuse_argmax, 2 k_vote_fuse_argmax_2cu, 3 the
 * instantiation that defers camera 1's arg-max update, 4 four cameras, 5 k_vote_fuse_argmax_alg2) and whether it read a
 * balanced partition: lets a test observe that a forced count or mode took effect and which kernel a shape reaches */
DSI_API int dsi_test_fused_last_launch(int* blocks, int* interleave, int* kernel, int* splits)
{
    REQUIRE(blocks && interleave && kernel && splits, DSI_ERR_INVALID, "null argument");
    dsi::fused_last_launch(blocks, interleave, kernel, splits);
    return DSI_OK;
}

/* test hook (not in the public header): the next fused vote kernels that mapper m leads run in the dealt mode as ONE
 * workgroup that acts as workgroup 0 of XCD `xcd` (0..7): it votes every (band, plane) pair, beginning at pair P xcd / 8 and
 * wrapping round to P xcd / 8 - 1 -- a fixed draw order that descends within a band.  -1 switches it off */
DSI_API int dsi_test_fused_solo(dsi_mapper_t* m, int xcd)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    REQUIRE(xcd >= -1 && xcd <= 7, DSI_ERR_INVALID, "XCD 0..7, or -1 (got %d)", xcd);
    m->fused_solo = xcd;
    return DSI_OK;
}

/* test hooks (not in the public header): time stamps of the phases of the next fused vote kernels that
 * mapper m leads (dsi_mapper_depth_map_of_events with mappers[0] == m): [workgroup][64 phases][16 waves][4]
 * ticks of the 100 MHz clock; *_read synchronises, copies and switches tracing off */
DSI_API int dsi_test_fused_trace_enable(dsi_mapper_t* m, size_t* n_words)
{
    REQUIRE(m && n_words, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(m->ctx)) return rc;
    *n_words = dsi::fused_trace_words();
    HIP_TRY(m->fused_trace.reserve(*n_words));
    HIP_TRY(hipMemsetAsync(m->fused_trace.p, 0, *n_words * sizeof(unsigned long long), m->ctx->stream));
    m->fused_trace_on = true;
    return DSI_OK;
}

DSI_API int dsi_test_fused_trace_read(dsi_mapper_t* m, unsigned long long* host, size_t n_words)
{
    REQUIRE(m && host, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->fused_trace_on && n_words <= m->fused_trace.cap, DSI_ERR_INVALID, "tracing is not enabled");
    if (int rc = set_device(m->ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    HIP_TRY(hipMemcpy(host, m->fused_trace.p, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    m->fused_trace_on = false;
    return DSI_OK;
}

/* test hook (not in the public header): total length of all runs [lo,hi) of the last banded
 * vote, i.e. the number of event-planes the voting kernel looked at (>= the number accepted) */
DSI_API int dsi_test_run_length_total(dsi_mapper_t* m, unsigned long long* total, unsigned long long* entries)
{
    REQUIRE(m && total && entries, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(m->ctx)) return rc;
    size_t units = m->info.n_packets;
    REQUIRE(!m->info_cuts_inline, DSI_ERR_INVALID, "the last vote derived its runs in the kernel: there is no cut table to add up");
    const uint32_t* src = m->cuts.p;
    if (m->info.packed == 2 || m->info.packed == 4) {  // grouped mapping: one run per group of packets
        units = (m->info.n_packets + m->info.group_packets - 1) / m->info.group_packets;
        src = m->gcuts.p;
    }
    const size_t n = units * (size_t)m->geom.nz * (size_t)m->info.bands;
    std::vector<uint32_t> h(n);
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    if (n) HIP_TRY(hipMemcpy(h.data(), src, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    unsigned long long t = 0;
    for (uint32_t c : h) t += (c >> 16) - (c & 0xffffu);
    *total = t;
    *entries = n;
    return DSI_OK;
}

/* test hook (not in the public header): residual-corrected division vs IEEE divide */
DSI_API int dsi_test_div_probe(dsi_context_t* ctx, const float* n, const float* d, size_t count, float* q, float* ref)
{
    REQUIRE(ctx && n && d && q && ref, DSI_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    DevBuf<float> dn, dd, dq, dr;
    const size_t bytes = count * sizeof(float);
    hipError_t e = dn.reserve(count);
    if (e == hipSuccess) e = dd.reserve(count);
    if (e == hipSuccess) e = dq.reserve(count);
    if (e == hipSuccess) e = dr.reserve(count);
    if (e == hipSuccess) e = hipMemcpy(dn.p, n, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dd.p, d, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsi::launch_div_probe(ctx->stream, dn.p, dd.p, count, dq.p, dr.p);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(q, dq.p, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ref, dr.p, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(DSI_ERR_HIP, "div probe failed: %s", hipGetErrorString(e));
    return DSI_OK;
}

// one axis (0 x, 1 y, 2 z) of dsi_grid_smooth_iir on its own, for tools/volume_filters_bench.py; with_post: the z kernel's
// folded post-scale
DSI_API int dsi_test_iir_axis(dsi_grid_t* g, int axis, float sigma, int numsteps, int with_post)
{
    REQUIRE(g && axis >= 0 && axis <= 2 && sigma > 0 && numsteps >= 1 && numsteps <= 16, DSI_ERR_INVALID, "bad argument");
    if (int rc = set_device(g->ctx)) return rc;
    const IirAxis ax = iir_axis(sigma, numsteps);
    HIP_TRY(dsi::launch_iir_axis(g->ctx->stream, g->data, g->nx, g->ny, g->nz, axis, ax.nu, ax.boundaryscale, numsteps,
                                 with_post != 0, ax.postscale));
    return DSI_OK;
}
#endif  // DSI_TIMING_EXPERIMENTS

}  // extern "C"

/* ---------------------------------------------------------- multi-GPU (RCCL) */
struct dsi_comm {
    ncclComm_t comm = nullptr;
    int device = 0, rank = 0, size = 1;
};

namespace {

// librccl entry points, resolved once (see load_rccl for which copy).
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                              hipStream_t) = nullptr;
    ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                                  hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;     // what RCCL itself says about a communicator
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;  // (bench.py prints it: proof of the rank count)
    ncclResult_t (*CommCuDevice)(const ncclComm_t, int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

Rccl* load_rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // The RCCL that belongs to the HIP runtime this process runs on: the librccl next to the loaded
        // libamdhip64 (/opt/rocm/lib, or torch's lib directory when torch brought its own runtime in
        // first).  Opening by soname instead could hand back an RCCL built for another runtime that
        // some other package loaded (seen: torch's librccl on /opt/rocm's libamdhip64 fails in
        // ncclCommInitAll).
        std::vector<std::string> names;
        Dl_info di;
        if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &di) && di.dli_fname) {
            std::string dir(di.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash);
                names.push_back(dir + "/librccl.so.1");
                names.push_back(dir + "/librccl.so");
            }
        }
        names.push_back("/opt/rocm/lib/librccl.so.1");
        names.push_back("librccl.so.1");
        names.push_back("librccl.so");
        for (const std::string& n : names) {
            r.lib = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
        if (!r.lib) {
            r.error = std::string("librccl could not be loaded: ") + (dlerror() ? dlerror() : "?");
            return;
        }
        auto sym = [&](const char* name) -> void* {
            void* p = dlsym(r.lib, name);
            if (!p && r.error.empty()) r.error = std::string("librccl lacks ") + name;
            return p;
        };
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(sym("ncclCommInitAll"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
        r.ReduceScatter = reinterpret_cast<decltype(r.ReduceScatter)>(sym("ncclReduceScatter"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
        r.CommCount = reinterpret_cast<decltype(r.CommCount)>(sym("ncclCommCount"));
        r.CommUserRank = reinterpret_cast<decltype(r.CommUserRank)>(sym("ncclCommUserRank"));
        r.CommCuDevice = reinterpret_cast<decltype(r.CommCuDevice)>(sym("ncclCommCuDevice"));
    });
    return &r;
}

#define RCCL_TRY(R, expr)                                                                          \
    do {                                                                                           \
        ncclResult_t e_ = (expr);                                                                  \
        if (e_ != ncclSuccess)                                                                     \
            return fail(DSI_ERR_COMM, "%s failed: %s (%s:%d)", #expr, (R)->GetErrorString(e_), __FILE__, \
                        __LINE__);                                                                 \
    } while (0)

int rccl_ready(Rccl** out)
{
    Rccl* r = load_rccl();
    if (!r->error.empty()) return fail(DSI_ERR_COMM, "%s", r->error.c_str());
    *out = r;
    return DSI_OK;
}

// One group of collectives, rank i's issued by per_rank(i) on the device of communicator cs[i] (which the caller has
// checked to be its objects' device): every rank is issued whatever another returned, the first error is the one reported.
template <typename F>
int rccl_grouped(Rccl* r, dsi_comm_t* const* cs, int n, const char* what, F per_rank)
{
    RCCL_TRY(r, r->GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (int i = 0; i < n; ++i) {
        (void)hipSetDevice(cs[i]->device);
        const ncclResult_t e = per_rank(i);
        if (e != ncclSuccess && bad == ncclSuccess) bad = e;
    }
    const ncclResult_t e2 = r->GroupEnd();
    if (bad != ncclSuccess) return fail(DSI_ERR_COMM, "%s failed: %s", what, r->GetErrorString(bad));
    if (e2 != ncclSuccess) return fail(DSI_ERR_COMM, "ncclGroupEnd failed: %s", r->GetErrorString(e2));
    return DSI_OK;
}

bool to_nccl_op(int op, ncclRedOp_t* out)
{
    switch (op) {
    case DSI_REDUCE_SUM: *out = ncclSum; return true;
    case DSI_REDUCE_MIN: *out = ncclMin; return true;
    case DSI_REDUCE_MAX: *out = ncclMax; return true;
    default: return false;
    }
}

}  // namespace

extern "C" {

int dsi_comm_unique_id(uint8_t id[DSI_COMM_ID_BYTES])
{
    REQUIRE(id, DSI_ERR_INVALID, "id is null");
    static_assert(sizeof(ncclUniqueId) == DSI_COMM_ID_BYTES, "RCCL unique id size");
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    ncclUniqueId u;
    RCCL_TRY(r, r->GetUniqueId(&u));
    std::memcpy(id, &u, sizeof u);
    return DSI_OK;
}

int dsi_comm_create_rank(dsi_context_t* ctx, const uint8_t id[DSI_COMM_ID_BYTES], int nranks, int rank,
                         dsi_comm_t** out)
{
    REQUIRE(ctx && id && out, DSI_ERR_INVALID, "null argument");
    *out = nullptr;
    REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, DSI_ERR_INVALID, "rank %d of %d", rank, nranks);
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    if (int rc = set_device(ctx)) return rc;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    dsi_comm* c = new (std::nothrow) dsi_comm();
    REQUIRE(c, DSI_ERR_INVALID, "out of host memory");
    c->device = ctx->device;
    c->rank = rank;
    c->size = nranks;
    const ncclResult_t e = r->CommInitRank(&c->comm, nranks, u, rank);
    if (e != ncclSuccess) {
        delete c;
        return fail(DSI_ERR_COMM, "ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, r->GetErrorString(e));
    }
    *out = c;
    return DSI_OK;
}

int dsi_comm_create_all(dsi_context_t* const* contexts, int n, dsi_comm_t** out)
{
    REQUIRE(contexts && out && n >= 1, DSI_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) out[i] = nullptr;
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        REQUIRE(contexts[i], DSI_ERR_INVALID, "context %d is null", i);
        devs[i] = contexts[i]->device;
        for (int j = 0; j < i; ++j)
            REQUIRE(devs[j] != devs[i], DSI_ERR_CONTEXT, "contexts %d and %d share device %d (RCCL: one rank per GPU)",
                    j, i, devs[i]);
    }
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    std::vector<ncclComm_t> comms(n, nullptr);
    RCCL_TRY(r, r->CommInitAll(comms.data(), n, devs.data()));
    for (int i = 0; i < n; ++i) {
        dsi_comm* c = new (std::nothrow) dsi_comm();
        if (!c) {
            for (int j = 0; j < n; ++j) {
                if (comms[j]) (void)r->CommDestroy(comms[j]);
                delete out[j];
                out[j] = nullptr;
            }
            return fail(DSI_ERR_INVALID, "out of host memory");
        }
        c->comm = comms[i];
        c->device = devs[i];
        c->rank = i;
        c->size = n;
        out[i] = c;
    }
    return DSI_OK;
}

int dsi_comm_destroy(dsi_comm_t* c)
{
    if (!c) return DSI_OK;
    Rccl* r = load_rccl();
    if (c->comm && r->CommDestroy) {
        (void)hipSetDevice(c->device);
        (void)r->CommDestroy(c->comm);
    }
    delete c;
    return DSI_OK;
}

int dsi_comm_rank(const dsi_comm_t* c) { return c ? c->rank : -1; }
int dsi_comm_size(const dsi_comm_t* c) { return c ? c->size : 0; }

static int allreduce_check(const dsi_comm_t* c, const dsi_grid_t* g)
{
    REQUIRE(c && g, DSI_ERR_INVALID, "null argument");
    REQUIRE(c->device == g->ctx->device, DSI_ERR_CONTEXT, "grid on device %d, communicator rank on device %d",
            g->ctx->device, c->device);
    return DSI_OK;
}

int dsi_grid_allreduce(dsi_comm_t* c, dsi_grid_t* g, int op)
{
    if (int rc = allreduce_check(c, g)) return rc;
    ncclRedOp_t nop;
    REQUIRE(to_nccl_op(op, &nop), DSI_ERR_BAD_OP, "bad reduce op %d", op);
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    if (int rc = set_device(g->ctx)) return rc;
    RCCL_TRY(r, r->AllReduce(g->data, g->data, g->n, ncclFloat32, nop, c->comm, g->ctx->stream));
    return DSI_OK;
}

int dsi_grid_allreduce_all(dsi_comm_t* const* comms, dsi_grid_t* const* grids, int n, int op)
{
    REQUIRE(comms && grids && n >= 1, DSI_ERR_INVALID, "bad argument");
    ncclRedOp_t nop;
    REQUIRE(to_nccl_op(op, &nop), DSI_ERR_BAD_OP, "bad reduce op %d", op);
    for (int i = 0; i < n; ++i) {
        if (int rc = allreduce_check(comms[i], grids[i])) return rc;
        REQUIRE(same_shape(grids[0], grids[i]), DSI_ERR_SHAPE, "grid %d has another shape", i);
    }
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    return rccl_grouped(r, comms, n, "ncclAllReduce", [&](int i) {
        return r->AllReduce(grids[i]->data, grids[i]->data, grids[i]->n, ncclFloat32, nop, comms[i]->comm, grids[i]->ctx->stream);
    });
}

static int ensure_planes_full_dev(dsi_mapper_t* m)
{
    if (m->planes_full_dev.p) return DSI_OK;
    HIP_TRY(m->planes_full_dev.reserve(m->planes_full.size()));
    HIP_TRY(hipMemcpyAsync(m->planes_full_dev.p, m->planes_full.data(), m->planes_full.size() * sizeof(float),
                           hipMemcpyHostToDevice, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));  // the source is host memory of this object: simplest
    return DSI_OK;
}

// local collapse + key packing of one shard (everything on the mapper's stream)
static int sharded_prepare(dsi_mapper_t* m, dsi_grid_t* g)
{
    REQUIRE(m && g, DSI_ERR_INVALID, "null argument");
    REQUIRE(m->ctx->device == g->ctx->device, DSI_ERR_CONTEXT, "mapper and grid live on different devices");
    REQUIRE(same_shape(m->grid, g), DSI_ERR_SHAPE, "grid shape differs from the mapper's DSI");
    REQUIRE(m->planes_full.size() <= 256, DSI_ERR_INVALID, "arg-max indices are u8");
    if (int rc = set_device(m->ctx)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    HIP_TRY(m->conf.reserve(npix));
    HIP_TRY(m->depth.reserve(npix));
    HIP_TRY(m->idx.reserve(npix));
    HIP_TRY(m->argmax_keys.reserve(npix));
    if (int rc = ensure_planes_full_dev(m)) return rc;
    if (int rc = dsi_context_wait_for(m->ctx, g->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    HIP_TRY(dsi::launch_collapse_max_z(m->ctx->stream, g->data, g->nx, g->ny, g->nz, m->conf.p, m->idx.p, nullptr,
                                       nullptr));
    HIP_TRY(dsi::launch_pack_argmax(m->ctx->stream, m->conf.p, m->idx.p, (int)npix, m->plane_begin,
                                    m->argmax_keys.p, 0));
    return release_to(g->ctx, m->ctx);  // the collapse READ g on the mapper's stream
}

static int sharded_finish(dsi_mapper_t* m)
{
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    HIP_TRY(hipSetDevice(m->ctx->device));
    HIP_TRY(dsi::launch_unpack_argmax(m->ctx->stream, m->argmax_keys.p, (int)npix, m->planes_full_dev.p, m->conf.p,
                                      m->idx.p, m->depth.p));
    return depth_buffers_ready(m);
}

int dsi_mapper_depth_map_sharded(dsi_mapper_t* m, dsi_grid_t* g, dsi_comm_t* c)
{
    REQUIRE(c, DSI_ERR_INVALID, "communicator is null");
    if (int rc = sharded_prepare(m, g)) return rc;
    REQUIRE(c->device == m->ctx->device, DSI_ERR_CONTEXT, "communicator rank on another device");
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    const size_t npix = (size_t)g->nx * g->ny;
    RCCL_TRY(r, r->AllReduce(m->argmax_keys.p, m->argmax_keys.p, npix, ncclUint64, ncclMax, c->comm,
                             m->ctx->stream));
    return sharded_finish(m);
}

// the all-reduce(MAX) of every rank's packed arg-max keys, as one group
static int keys_allreduce_grouped(Rccl* r, dsi_mapper_t* const* ms, dsi_comm_t* const* cs, int n, size_t npix)
{
    return rccl_grouped(r, cs, n, "ncclAllReduce", [&](int i) {
        return r->AllReduce(ms[i]->argmax_keys.p, ms[i]->argmax_keys.p, npix, ncclUint64, ncclMax, cs[i]->comm, ms[i]->ctx->stream);
    });
}

int dsi_mapper_depth_map_sharded_all(dsi_mapper_t* const* ms, dsi_grid_t* const* gs, dsi_comm_t* const* cs, int n)
{
    REQUIRE(ms && gs && cs && n >= 1, DSI_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) {
        REQUIRE(cs[i], DSI_ERR_INVALID, "communicator %d is null", i);
        if (int rc = sharded_prepare(ms[i], gs[i])) return rc;
        REQUIRE(cs[i]->device == ms[i]->ctx->device, DSI_ERR_CONTEXT, "communicator %d on another device", i);
        REQUIRE(ms[i]->geom.nx == ms[0]->geom.nx && ms[i]->geom.ny == ms[0]->geom.ny, DSI_ERR_SHAPE,
                "mapper %d has another image size", i);
    }
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    const size_t npix = (size_t)ms[0]->geom.nx * ms[0]->geom.ny;
    if (int rc = keys_allreduce_grouped(r, ms, cs, n, npix)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = sharded_finish(ms[i])) return rc;
    return DSI_OK;
}

// ---- temporal fusion's last step with a reduce-scatter: rank r of n reduces only planes
// [r q, (r+1) q), q = nz / n, of the accumulator (the nz mod n planes left over are all-reduced: every rank then
// has them), finalises and arg-maxes what it owns, and ONE all-reduce(MAX) of the packed keys gives every rank
// the depth map.  Per rank (n-1)/n x S bytes cross xGMI instead of the all-reduce's 2 (n-1)/n x S.
static int scattered_check(dsi_mapper_t* m, dsi_grid_t* acc, dsi_comm_t* c, int mode)
{
    REQUIRE(m && acc && c, DSI_ERR_INVALID, "null argument");
    REQUIRE(valid_acc_mode(mode), DSI_ERR_BAD_OP, "bad accumulate mode %d", mode);
    REQUIRE(m->ctx->device == acc->ctx->device && c->device == acc->ctx->device, DSI_ERR_CONTEXT,
            "mapper, accumulator and communicator rank must live on one device");
    REQUIRE(same_shape(m->grid, acc), DSI_ERR_SHAPE, "accumulator shape differs from the mapper's DSI");
    REQUIRE(m->plane_begin == 0 && (int)m->planes_full.size() == acc->nz, DSI_ERR_INVALID,
            "the mapper must own the whole depth vector (time slices shard by time, not by plane)");
    REQUIRE(acc->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", acc->nz);
    return DSI_OK;
}

// the two collectives on the accumulator (callers bracket several ranks with ncclGroupStart / End); which planes go
// where is dsi::host::scatter_plan's business (shared with the host-staged tests)
static ncclResult_t scattered_reduce(Rccl* r, dsi_grid_t* acc, dsi_comm_t* c, ncclRedOp_t nop)
{
    const size_t plane = (size_t)acc->nx * acc->ny;
    dsi::host::ScatterPlan sp;
    if (!dsi::host::scatter_plan(acc->nz, c->size, c->rank, &sp)) return ncclInvalidArgument;
    ncclResult_t e = ncclSuccess;
    if (sp.q > 0)  // in place: the receive buffer is this rank's stretch of the send buffer
        e = r->ReduceScatter(acc->data, acc->data + (size_t)sp.own_begin * plane, (size_t)sp.q * plane, ncclFloat32, nop, c->comm,
                             acc->ctx->stream);
    if (e == ncclSuccess && sp.tail_count > 0) {
        float* tail = acc->data + (size_t)sp.tail_begin * plane;
        e = r->AllReduce(tail, tail, (size_t)sp.tail_count * plane, ncclFloat32, nop, c->comm, acc->ctx->stream);
    }
    return e;
}

// finalize + arg-max of the planes rank `rank` of `nranks` owns -> packed keys (on the mapper's stream)
static int scattered_local(dsi_mapper_t* m, dsi_grid_t* acc, int nranks, int rank, int mode, int n_maps)
{
    if (int rc = set_device(m->ctx)) return rc;
    const size_t plane = (size_t)acc->nx * acc->ny;
    dsi::host::ScatterPlan sp;
    REQUIRE(dsi::host::scatter_plan(acc->nz, nranks, rank, &sp), DSI_ERR_INVALID, "rank %d of %d", rank, nranks);
    HIP_TRY(m->conf.reserve(plane));
    HIP_TRY(m->depth.reserve(plane));
    HIP_TRY(m->idx.reserve(plane));
    HIP_TRY(m->argmax_keys.reserve(plane));
    if (int rc = ensure_planes_full_dev(m)) return rc;
    if (int rc = dsi_context_wait_for(m->ctx, acc->ctx)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    hipStream_t st = m->ctx->stream;
    const int begin[2] = {sp.own_begin, sp.tail_begin}, count[2] = {sp.own_count, sp.tail_count};
    bool first = true;
    for (int k = 0; k < 2; ++k) {
        if (count[k] <= 0) continue;
        float* p = acc->data + (size_t)begin[k] * plane;
        HIP_TRY(dsi::launch_finalize(st, p, (size_t)count[k] * plane, mode, n_maps));
        HIP_TRY(dsi::launch_collapse_max_z(st, p, acc->nx, acc->ny, count[k], m->conf.p, m->idx.p, nullptr, nullptr));
        HIP_TRY(dsi::launch_pack_argmax(st, m->conf.p, m->idx.p, (int)plane, begin[k], m->argmax_keys.p, first ? 0 : 1));
        first = false;
    }
    if (first) HIP_TRY(hipMemsetAsync(m->argmax_keys.p, 0, plane * sizeof(unsigned long long), st));  // owns no plane
    // finalize WROTE the accumulator on the mapper's stream: whatever the accumulator's context queues next (the
    // next round's accumulateBegin) must come after it
    return release_to(acc->ctx, m->ctx);
}

int dsi_mapper_depth_map_reduce_scattered(dsi_mapper_t* m, dsi_grid_t* acc, dsi_comm_t* c, int mode, int n_maps)
{
    if (int rc = scattered_check(m, acc, c, mode)) return rc;
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    ncclRedOp_t nop;
    REQUIRE(to_nccl_op(dsi_acc_reduce_op(mode), &nop), DSI_ERR_BAD_OP, "mode %d has no reduce op", mode);
    if (int rc = set_device(acc->ctx)) return rc;
    if (int rc = rccl_grouped(r, &c, 1, "reduce-scatter", [&](int) { return scattered_reduce(r, acc, c, nop); })) return rc;
    if (int rc = scattered_local(m, acc, c->size, c->rank, mode, n_maps)) return rc;
    const size_t npix = (size_t)acc->nx * acc->ny;
    RCCL_TRY(r, r->AllReduce(m->argmax_keys.p, m->argmax_keys.p, npix, ncclUint64, ncclMax, c->comm, m->ctx->stream));
    return sharded_finish(m);
}

int dsi_mapper_depth_map_reduce_scattered_all(dsi_mapper_t* const* ms, dsi_grid_t* const* accs, dsi_comm_t* const* cs, int n,
                                              int mode, int n_maps)
{
    REQUIRE(ms && accs && cs && n >= 1, DSI_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) {
        if (int rc = scattered_check(ms[i], accs[i], cs[i], mode)) return rc;
        REQUIRE(same_shape(accs[0], accs[i]), DSI_ERR_SHAPE, "accumulator %d has another shape", i);
    }
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    ncclRedOp_t nop;
    REQUIRE(to_nccl_op(dsi_acc_reduce_op(mode), &nop), DSI_ERR_BAD_OP, "mode %d has no reduce op", mode);
    if (int rc = rccl_grouped(r, cs, n, "reduce-scatter", [&](int i) { return scattered_reduce(r, accs[i], cs[i], nop); }))
        return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = scattered_local(ms[i], accs[i], cs[i]->size, cs[i]->rank, mode, n_maps)) return rc;
    if (int rc = keys_allreduce_grouped(r, ms, cs, n, (size_t)accs[0]->nx * accs[0]->ny)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = sharded_finish(ms[i])) return rc;
    return DSI_OK;
}

/* ---- the same three steps with the transport left to the caller (host-staged tests, other transports) ---- */
int dsi_scatter_plan(int nz, int nranks, int rank, dsi_scatter_plan_t* out)
{
    REQUIRE(out, DSI_ERR_INVALID, "out is null");
    dsi::host::ScatterPlan sp;
    REQUIRE(dsi::host::scatter_plan(nz, nranks, rank, &sp), DSI_ERR_INVALID, "bad partition: %d planes, rank %d of %d", nz, rank,
            nranks);
    out->q = sp.q;
    out->own_begin = sp.own_begin;
    out->own_count = sp.own_count;
    out->tail_begin = sp.tail_begin;
    out->tail_count = sp.tail_count;
    return DSI_OK;
}

int dsi_plane_range(int nz, int nranks, int rank, int* begin, int* count)
{
    REQUIRE(begin && count, DSI_ERR_INVALID, "null argument");
    REQUIRE(dsi::host::plane_range(nz, nranks, rank, begin, count), DSI_ERR_INVALID, "bad partition: %d planes, rank %d of %d",
            nz, rank, nranks);
    return DSI_OK;
}

int dsi_argmax_keys_pack(const float* conf, const uint8_t* idx_local, size_t n, int plane_begin, uint64_t* keys)
{
    REQUIRE(n == 0 || (conf && idx_local && keys), DSI_ERR_INVALID, "null argument");
    REQUIRE(plane_begin >= 0 && plane_begin <= 255, DSI_ERR_INVALID, "plane_begin %d outside 0..255", plane_begin);
    for (size_t i = 0; i < n; ++i) {
        const int gp = (int)idx_local[i] + plane_begin;
        REQUIRE(gp <= 255, DSI_ERR_INVALID, "global plane index %d does not fit the key's 8 bits", gp);
        keys[i] = dsi::host::argmax_key(conf[i], gp);
    }
    return DSI_OK;
}

int dsi_argmax_keys_unpack(const uint64_t* keys, size_t n, float* conf, uint8_t* idx)
{
    REQUIRE(n == 0 || (keys && conf && idx), DSI_ERR_INVALID, "null argument");
    for (size_t i = 0; i < n; ++i) {
        int gp = 0;
        dsi::host::argmax_unkey(keys[i], &conf[i], &gp);
        idx[i] = (uint8_t)gp;
    }
    return DSI_OK;
}

int dsi_mapper_depth_map_scattered_local(dsi_mapper_t* m, dsi_grid_t* acc, int nranks, int rank, int mode, int n_maps)
{
    REQUIRE(m && acc, DSI_ERR_INVALID, "null argument");
    REQUIRE(valid_acc_mode(mode), DSI_ERR_BAD_OP, "bad accumulate mode %d", mode);
    REQUIRE(m->ctx->device == acc->ctx->device, DSI_ERR_CONTEXT, "mapper and accumulator must live on one device");
    REQUIRE(same_shape(m->grid, acc), DSI_ERR_SHAPE, "accumulator shape differs from the mapper's DSI");
    REQUIRE(m->plane_begin == 0 && (int)m->planes_full.size() == acc->nz, DSI_ERR_INVALID,
            "the mapper must own the whole depth vector (time slices shard by time, not by plane)");
    REQUIRE(acc->nz <= 256, DSI_ERR_INVALID, "arg-max indices are u8: dimZ must be <= 256 (got %d)", acc->nz);
    REQUIRE(n_maps >= 1, DSI_ERR_INVALID, "number of maps must be >= 1 (got %d)", n_maps);
    return scattered_local(m, acc, nranks, rank, mode, n_maps);
}

int dsi_mapper_argmax_keys_download(dsi_mapper_t* m, uint64_t* host)
{
    REQUIRE(m && host, DSI_ERR_INVALID, "null argument");
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    REQUIRE(m->argmax_keys.cap >= npix, DSI_ERR_INVALID, "this mapper holds no arg-max keys");
    if (int rc = set_device(m->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(host, m->argmax_keys.p, npix * sizeof(uint64_t), hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    return DSI_OK;
}

int dsi_mapper_argmax_keys_upload(dsi_mapper_t* m, const uint64_t* host)
{
    REQUIRE(m && host, DSI_ERR_INVALID, "null argument");
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    if (int rc = set_device(m->ctx)) return rc;
    HIP_TRY(m->argmax_keys.reserve(npix));
    HIP_TRY(hipMemcpyAsync(m->argmax_keys.p, host, npix * sizeof(uint64_t), hipMemcpyHostToDevice, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));  // the source is pageable host memory
    return DSI_OK;
}

int dsi_mapper_depth_map_from_keys(dsi_mapper_t* m)
{
    REQUIRE(m, DSI_ERR_INVALID, "mapper is null");
    const size_t npix = (size_t)m->geom.nx * m->geom.ny;
    REQUIRE(m->argmax_keys.cap >= npix, DSI_ERR_INVALID, "this mapper holds no arg-max keys");
    if (int rc = set_device(m->ctx)) return rc;
    HIP_TRY(m->conf.reserve(npix));
    HIP_TRY(m->depth.reserve(npix));
    HIP_TRY(m->idx.reserve(npix));
    if (int rc = ensure_planes_full_dev(m)) return rc;
    if (int rc = depth_buffers_acquire(m)) return rc;
    return sharded_finish(m);
}

int dsi_comm_query(const dsi_comm_t* c, int* nranks, int* rank, int* device)
{
    REQUIRE(c && c->comm, DSI_ERR_INVALID, "communicator is null");
    Rccl* r = nullptr;
    if (int rc = rccl_ready(&r)) return rc;
    REQUIRE(r->CommCount && r->CommUserRank && r->CommCuDevice, DSI_ERR_COMM, "librccl lacks the communicator queries");
    int v = 0;
    if (nranks) {
        RCCL_TRY(r, r->CommCount(c->comm, &v));
        *nranks = v;
    }
    if (rank) {
        RCCL_TRY(r, r->CommUserRank(c->comm, &v));
        *rank = v;
    }
    if (device) {
        RCCL_TRY(r, r->CommCuDevice(c->comm, &v));
        *device = v;
    }
    return DSI_OK;
}

}  // extern "C"
