// dsi_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the DSI engine.
//
// Replaces, on the GPU, the reference CPU code
//   MapperEMVS::evaluateDSI stage A   mapper_emvs_stereo.cpp:101-142
//   MapperEMVS::fillVoxelGrid         mapper_emvs_stereo.cpp:151-205
//   Grid3D::accumulateGridValueAt     cartesian3dgrid.h:253-273
//   Grid3D fusion ops                 cartesian3dgrid.h:64-192
//   Grid3D::collapseMaxZSlice         cartesian3dgrid.cpp:115-137
//   Grid3D::computeMeanSquare         cartesian3dgrid.cpp:164-174
//
// Numerics: the reference is an SSE2 build without FMA.  Every coordinate is
// computed with the same operations in the same order (separate multiply, add,
// IEEE divide); only the order in which votes are summed into a voxel differs.
// This file must be compiled with -ffp-contract=off (the pragma below restates
// it); explicit fmaf() calls are the only fused operations.
#include "dsi_kernels.h"
#include "dsi_vote_asm.h"
#define DSI_PCA_FN __host__ __device__ inline  // (the solve of dsi_pca_host.hpp runs in k_map_pca too)
#include "dsi_pca_host.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <mutex>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace dsi {

namespace {

constexpr int kWave = 64;

__device__ __forceinline__ bool finitef(float v) { return __builtin_isfinite(v); }

// Eigen 3.3 fixed-size length-3 dot: x0 + (x1 + x2) (redux_novec_unroller).
__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2)
{
    const float x0 = a0 * b0, x1 = a1 * b1, x2 = a2 * b2;
    return x0 + (x1 + x2);
}

__device__ __forceinline__ float cof3(const float* m, int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
}

// Eigen compute_inverse<Matrix3f> (cofactors; first column drives the determinant).
__device__ void inverse3x3(const float* m, float* out)
{
    const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
    const float det = dot3(c0, m[0], c1, m[3], c2, m[6]);
    const float invdet = 1.f / det;
    out[0] = c0 * invdet;
    out[1] = c1 * invdet;
    out[2] = c2 * invdet;
    out[3] = cof3(m, 0, 1) * invdet;
    out[4] = cof3(m, 1, 1) * invdet;
    out[5] = cof3(m, 2, 1) * invdet;
    out[6] = cof3(m, 0, 2) * invdet;
    out[7] = cof3(m, 1, 2) * invdet;
    out[8] = cof3(m, 2, 2) * invdet;
}

__device__ void mul3x3(const float* a, const float* b, float* c)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            c[3 * i + j] = dot3(a[3 * i], b[j], a[3 * i + 1], b[3 + j], a[3 * i + 2], b[6 + j]);
}

// n / d, correctly rounded, given r = RN(1/d): two residual corrections, the same
// recurrence the gfx950 IEEE-divide expansion runs after v_rcp_f32, without its
// v_div_scale / v_div_fixup range handling (callers guarantee 2^-40 <= |d| <= 2^40;
// a non-finite or overflowing n gives NaN/inf, which the vote rejects either way).
__device__ __forceinline__ float div_rc(float n, float d, float r)
{
    float q = n * r;
    float e = __builtin_fmaf(-d, q, n);
    q = __builtin_fmaf(e, r, q);
    e = __builtin_fmaf(-d, q, n);
    return __builtin_fmaf(e, r, q);
}

// mapper_emvs_stereo.cpp:177-182
__device__ __forceinline__ void plane_coefficients(float cx_, float cy_, float cz_, float zi,
                                                   const Geom& g, float& a, float& bx, float& by,
                                                   float& d)
{
    a = g.z0 * (zi - cz_);
    bx = (g.z0 - zi) * (cx_ * g.vfx + cz_ * g.vcx);
    by = (g.z0 - zi) * (cy_ * g.vfy + cz_ * g.vcy);
    d = zi * (g.z0 - cz_);
}

// ---------------------------------------------------------------- stage A --
// mapper_emvs_stereo.cpp:101-126: one thread per packet.
// camera centre (3 floats) and H_z0 (9 floats, row-major) of one packet from its pose Rt (12 floats)
__device__ __forceinline__ void packet_geometry_of(const float* __restrict__ Rtk, const Geom& g,
                                                   float* __restrict__ center, float* __restrict__ Hout)
{
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rtk[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = Rtk[9 + i];

    // :108  C = -R^T t
#pragma unroll
    for (int i = 0; i < 3; ++i)
        center[i] = dot3(-R[i], t[0], -R[3 + i], t[1], -R[6 + i], t[2]);

    // :114-116
    float Hinv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hinv[i] = R[i] * g.z0;
    Hinv[2] += t[0];
    Hinv[5] += t[1];
    Hinv[8] += t[2];

    const float Km[9] = {g.kfx, 0.f, g.kcx, 0.f, g.kfy, g.kcy, 0.f, 0.f, 1.f};
    const float Kvm[9] = {g.vfx, 0.f, g.vcx, 0.f, g.vfy, g.vcy, 0.f, 0.f, 1.f};
    float Kvinv[9], M1[9], M[9], Hk[9];
    inverse3x3(Kvm, Kvinv);  // geometry_utils.hpp:47
    mul3x3(Km, Hinv, M1);    // :119, left to right
    mul3x3(M1, Kvinv, M);
    inverse3x3(M, Hk);       // :120
#pragma unroll
    for (int i = 0; i < 9; ++i) Hout[i] = Hk[i];
}

__global__ void k_packet_geometry(const float* __restrict__ Rt, int np, Geom g,
                                  float* __restrict__ centers, float* __restrict__ H)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= np) return;
    packet_geometry_of(Rt + 12 * (size_t)k, g, centers + 3 * (size_t)k, H + 9 * (size_t)k);
}

// mapper_emvs_stereo.cpp:129-142 for one event: LUT, 4x4 packet product ((c0*u + c1*v) + c2*1) + c3*0,
// p /= p[2]
// the two halves of it, for callers that keep several events in flight: the rectified pixel (:134; NaN for a pixel
// outside the sensor, which has no LUT entry -- the reference would read past its matrix --: the event then gets a
// non-finite location, which no plane accepts) ...
__device__ __forceinline__ float2 rectified_pixel(unsigned x, unsigned y, const float2* __restrict__ lut, int sensor_w,
                                                  int sensor_h)
{
    if (!lut) return make_float2((float)x, (float)y);
    // (branch-free, so that a thread's look-ups are issued back to back: entry 0 is read in place of a missing one)
    const bool inside = x < (unsigned)sensor_w && y < (unsigned)sensor_h;
    const float2 p = lut[inside ? (size_t)y * sensor_w + x : (size_t)0];
    const float nan = __builtin_nanf("");
    return make_float2(inside ? p.x : nan, inside ? p.y : nan);
}

// ... and the packet's homography applied to it (:135-142)
__device__ __forceinline__ float2 warp_pixel_z0(float2 uv, const float* __restrict__ h)
{
    const float u = uv.x, v = uv.y;
    const float px = ((h[0] * u + h[1] * v) + h[2] * 1.f) + 0.f;
    const float py = ((h[3] * u + h[4] * v) + h[5] * 1.f) + 0.f;
    const float pz = ((h[6] * u + h[7] * v) + h[8] * 1.f) + 0.f;
    return make_float2(px / pz, py / pz);
}

__device__ __forceinline__ float2 warp_event_z0(unsigned x, unsigned y, const float* __restrict__ h,
                                                const float2* __restrict__ lut, int sensor_w, int sensor_h)
{
    if (lut && (x >= (unsigned)sensor_w || y >= (unsigned)sensor_h)) return make_float2(__builtin_nanf(""), __builtin_nanf(""));
    return warp_pixel_z0(rectified_pixel(x, y, lut, sensor_w, sensor_h), h);
}

// mapper_emvs_stereo.cpp:129-142: one thread per event slot of a packet.
__global__ void k_warp_z0(const uint16_t* __restrict__ ex, const uint16_t* __restrict__ ey,
                          const uint32_t* __restrict__ packet_first, int np,
                          const float* __restrict__ H, const float2* __restrict__ lut,
                          int sensor_w, int sensor_h, float2* __restrict__ xy)
{
    const int k = blockIdx.x;  // packet
    const size_t first = packet_first ? (size_t)packet_first[k] : (size_t)k * kPacket;
    const float* h = H + 9 * (size_t)k;
    const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6],
                h7 = h[7], h8 = h[8];
    const float hh[9] = {h0, h1, h2, h3, h4, h5, h6, h7, h8};
    for (int j = threadIdx.x; j < kPacket; j += blockDim.x)
        xy[(size_t)k * kPacket + j] = warp_event_z0(ex[first + j], ey[first + j], hh, lut, sensor_w, sensor_h);
}

// ------------------------------------------------- stage B: global atomics --
// cartesian3dgrid.h:253-273 with the int-conversion guard expressed in float
// (x+1 < Nx  <=>  x_f < Nx-1 for x_f >= 0), so that inf/huge/NaN are rejected
// exactly like the x86 build rejects them.
__device__ __forceinline__ void vote_global(float X, float Y, float* __restrict__ plane, int nx,
                                            float xmax, float ymax)
{
    if (X >= 0.f && Y >= 0.f && X < xmax && Y < ymax) {
        const int xi = (int)X, yi = (int)Y;
        const float fx = X - (float)xi, fy = Y - (float)yi, fx1 = 1.f - fx, fy1 = 1.f - fy;
        float* gptr = plane + (size_t)yi * nx + xi;
        unsafeAtomicAdd(gptr, fx1 * fy1);
        unsafeAtomicAdd(gptr + 1, fx * fy1);
        unsafeAtomicAdd(gptr + nx, fx1 * fy);
        unsafeAtomicAdd(gptr + nx + 1, fx * fy);
    }
}

constexpr int kVgPlanes = 8;  // planes per block of the global-atomic kernel

// block = (packet, group of planes); thread t owns events t, t+256, ... of the packet
__global__ __launch_bounds__(256) void k_vote_global(const float2* __restrict__ xy,
                                                     const float* __restrict__ centers,
                                                     const float* __restrict__ planes, Geom g,
                                                     float* __restrict__ dsi)
{
    const int k = blockIdx.x;
    const int zbeg = blockIdx.y * kVgPlanes;
    const int zend = min(g.nz, zbeg + kVgPlanes);
    const float cx_ = centers[3 * k], cy_ = centers[3 * k + 1], cz_ = centers[3 * k + 2];
    float2 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = xy[(size_t)k * kPacket + threadIdx.x + 256 * i];
    const float xmax = (float)(g.nx - 1), ymax = (float)(g.ny - 1);
    const size_t plane_sz = (size_t)g.nx * g.ny;
    for (int z = zbeg; z < zend; ++z) {
        float a, bx, by, d;
        plane_coefficients(cx_, cy_, cz_, planes[z], g, a, bx, by, d);
        float* plane = dsi + (size_t)z * plane_sz;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float X = (e[i].x * a + bx) / d;  // :194
            const float Y = (e[i].y * a + by) / d;  // :195
            vote_global(X, Y, plane, g.nx, xmax, ymax);
        }
    }
}

// ------------------------------------------------ stage B: LDS row bands ---
// (1) per packet: drop events that no plane can accept (non-finite z0 location) and group
//     the rest by the row floor(y0) they fall in at z0 (counting sort in LDS; the order inside
//     a row does not matter).  For one (packet, plane) the map y0 -> Y is monotone (each of
//     *a, +by, /d rounds monotonically), so the events landing in a band of output rows come
//     from a contiguous range of z0 rows = one contiguous run of the grouped packet.
//     Rows are binned over [-pad, ny+pad) (events warped to z0 spill well outside the grid
//     when the camera is far from the reference view, and other planes pull them back in);
//     bin 0 holds everything below, the last bin everything above:
//     bin(y0) = clamp(floor(y0), -pad-1, ny+pad) + pad + 1, nb = ny + 2*pad + 2 bins,
//     rowstart[p][b] = number of kept events in bins < b, b = 0..nb.
__device__ __forceinline__ int row_bin(float y0, int ny, int pad)
{
    const float f = fminf(fmaxf(__builtin_floorf(y0), (float)(-pad - 1)), (float)(ny + pad));
    return (int)f + pad + 1;  // finite y0 only
}

// Events of one packet with bit-identical z0 locations (same raw pixel fired again within the
// packet) are merged into one record with a multiplicity: an open-addressing hash set in LDS
// keyed by the 64 bits of (x0, y0); the first event to arrive in a slot represents the rest.
constexpr int kHashSlots = 2048;  // >= 2 * kPacket
constexpr unsigned long long kHashEmpty = ~0ull;  // a NaN pair: never a finite location

// Stage A of a packet, fused in when the events come raw (xy == nullptr): the block computes its
// packet's camera centre and H_z0 (one thread; written to `centers` for k_plane_coef) and warps its
// 1024 events to z0 in registers -- the z0 locations never go through HBM (saves 8 B written +
// 8 B read per event and two launches per evaluateDSI).
struct RawEvents {
    const float* Rt;             // [np][12]
    const uint16_t *ex, *ey;
    const uint32_t* packet_first;  // or nullptr: packet k starts at k * 1024
    const float2* lut;             // or nullptr: identity
    int sensor_w, sensor_h;
    Geom g;
    float* centers;              // out [np][3]
    int unit_multiplicity;       // test hook: every record gets multiplicity 1 (the DSI then counts accepted RECORDS)
};

// one camera's share of a multi-camera preparation launch (k_sort_packets_multi, k_plane_coef_multi)
struct PrepCamera {
    RawEvents raw;
    int np;
    EvRec* sxy;
    uint32_t* nvalid;
    uint16_t* rowstart;
    const float* planes;
    PlaneCoef* coef;
    uint32_t* cuts;
    uint32_t* pair_work;  // [bands][nz]: records the voting kernel will look at per (band, plane), or nullptr
};
struct PrepCameras {
    PrepCamera cam[kFusedMaxCameras];
    int n;
};

// RAW (the events come as sensor pixels, stage A fused in): two events of a packet have the same z0
// location iff they have the same pixel, so the hash set is keyed by the 32-bit pixel and one 64-bit
// word per slot holds key and count -- 16 KB instead of 24 KB of LDS, which is what decides how many
// packets a CU sorts at once (time at 10 M events: 35 us + 260 us / blocks per CU, measured by
// padding the LDS: 5 blocks 86 us, 4: 99, 3: 122, 2: 172; now 8).
template <bool RAW>
__device__ __forceinline__ void sort_packets_body(const int k, const float2* __restrict__ xy, const RawEvents& raw,
                                                  int np, int ny,
                                                  int nz, int pad, EvRec* __restrict__ sxy,
                                                  uint32_t* __restrict__ nvalid,
                                                  uint16_t* __restrict__ rowstart, uint32_t* __restrict__ pair_work,
                                                  int n_pairs)
{
    extern __shared__ uint32_t hist[];  // nb + 1 counters, then scanned in place
    __shared__ float s_H[9];
    __shared__ __attribute__((aligned(16))) unsigned long long hkey[kHashSlots];  // RAW: pixel | count << 32
    __shared__ uint32_t hcnt[RAW ? 1 : kHashSlots];
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t big;  // some |x0| or |y0| above 2^40 (never a real pixel)
    const int nb = ny + 2 * pad + 2;
    // nvalid[np + z]: "plane z has a coefficient set that needs the IEEE divide", set by
    // k_plane_coef (next kernel on the stream), read by the packed voting kernel
    if (k == 0) {
        // (+ 8 work counters of the persistent voting kernel behind the per-plane flags, + lane mapping 8's overflow word)
        for (int i = threadIdx.x; i < nz + 9; i += 256) nvalid[np + i] = 0;
        // (+ the records per (band, plane) pair that k_plane_coef counts for the fused kernel's partition)
        if (pair_work)
            for (int i = threadIdx.x; i < n_pairs; i += 256) pair_work[i] = 0;
        if (threadIdx.x == 0) {  // the multiplicity-0 record behind the last packet
            const EvRec none = {0.f, 0.f, 0u};
            sxy[(size_t)np * kPacket] = none;
        }
    }
    if (threadIdx.x == 0) big = 0;
    for (int i = threadIdx.x; i <= nb; i += 256) hist[i] = 0;
    for (int i = threadIdx.x; i < kHashSlots; i += 256) {
        hkey[i] = kHashEmpty;
        if (!RAW) hcnt[i] = 0;
    }
    if (RAW && threadIdx.x == 0) {
        float c3[3], h9[9];
        packet_geometry_of(raw.Rt + 12 * (size_t)k, raw.g, c3, h9);
#pragma unroll
        for (int i = 0; i < 3; ++i) raw.centers[3 * (size_t)k + i] = c3[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) s_H[i] = h9[i];
    }
    // the four events of a thread travel TOGETHER: all coordinate loads, then all look-ups of the rectification table,
    // before the first hash insert (one after the other -- load, look-up, insert, next load -- a block spent four
    // round trips to HBM and four to L2 in a row: 63 us per 10 M events; the loads are issued before the barrier)
    float2 ev[4];
    uint32_t pixel4[4] = {0u, 0u, 0u, 0u};
    if (RAW) {
        const size_t first_ev = raw.packet_first ? (size_t)raw.packet_first[k] : (size_t)k * kPacket;
        unsigned px[4], py[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const size_t e = first_ev + threadIdx.x + 256 * h;
            px[h] = raw.ex[e];
            py[h] = raw.ey[e];
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) pixel4[h] = px[h] | (py[h] << 16);
        if (raw.lut) {  // rectified_pixel() x 4 with the four look-ups issued back to back
            bool inside[4];
            float2 p[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                inside[h] = px[h] < (unsigned)raw.sensor_w && py[h] < (unsigned)raw.sensor_h;
                p[h] = raw.lut[inside[h] ? (size_t)py[h] * raw.sensor_w + px[h] : (size_t)0];
            }
            const float nan = __builtin_nanf("");
#pragma unroll
            for (int h = 0; h < 4; ++h) ev[h] = make_float2(inside[h] ? p[h].x : nan, inside[h] ? p[h].y : nan);
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) ev[h] = make_float2((float)px[h], (float)py[h]);
        }
    } else {
#pragma unroll
        for (int h = 0; h < 4; ++h) ev[h] = xy[(size_t)k * kPacket + threadIdx.x + 256 * h];
    }
    __syncthreads();
    if (RAW) {
#pragma unroll
        for (int h = 0; h < 4; ++h) ev[h] = warp_pixel_z0(ev[h], s_H);  // (NaN in, NaN out)
    }
    int bin[4], slot[4];
    uint32_t rank[4], mult[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const uint32_t pixel = pixel4[h];
        bin[h] = -1;
        slot[h] = 0;
        rank[h] = 0;
        mult[h] = 0;
        if (finitef(ev[h].x) && finitef(ev[h].y)) {
            bool first;
            if (RAW) {
                // (a claimed word has a count < 2^11 in its high half, the empty word all ones: no pixel
                //  value can be mistaken for an empty slot)
                uint32_t hs = (pixel * 0x9E3779B1u) >> 21;  // 11 bits
                for (;;) {
                    const unsigned long long old = atomicCAS(&hkey[hs], kHashEmpty, (unsigned long long)pixel);
                    if (old == kHashEmpty || (uint32_t)old == pixel) break;
                    hs = (hs + 1) & (kHashSlots - 1);
                }
                slot[h] = (int)hs;
                first = (atomicAdd(&hkey[hs], 1ull << 32) >> 32) == 0ull;
            } else {
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint(ev[h].y) << 32) | __float_as_uint(ev[h].x);
                uint32_t hs = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 53);  // 11 bits
                for (;;) {
                    const unsigned long long old = atomicCAS(&hkey[hs], kHashEmpty, key);
                    if (old == kHashEmpty || old == key) break;
                    hs = (hs + 1) & (kHashSlots - 1);
                }
                slot[h] = (int)hs;
                first = atomicAdd(&hcnt[hs], 1u) == 0u;
            }
            if (first) bin[h] = row_bin(ev[h].y, ny, pad);  // representative
            if (!(fabsf(ev[h].x) <= 0x1p40f && fabsf(ev[h].y) <= 0x1p40f)) big = 1u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 4; ++h)
        if (bin[h] >= 0) {
            rank[h] = atomicAdd(&hist[bin[h]], 1u);
            mult[h] = RAW ? (uint32_t)(hkey[slot[h]] >> 32) : hcnt[slot[h]];  // (the records are staged over hkey later)
            if (RAW && raw.unit_multiplicity) mult[h] = 1u;
        }
    __syncthreads();
    // exclusive scan of hist[0..nb): each thread owns a contiguous slice
    const int per = (nb + 255) / 256;
    const int b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    uint32_t local = 0;
    for (int i = b0; i < b1; ++i) local += hist[i];
    uint32_t incl = local;
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - local;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) base += wave_tot[w];
    const uint32_t total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
    for (int i = b0; i < b1; ++i) {
        const uint32_t c = hist[i];
        hist[i] = base;
        base += c;
    }
    if (threadIdx.x == 0) hist[nb] = total;
    __syncthreads();
    uint16_t* rs = rowstart + (size_t)k * (nb + 1);
    for (int i = threadIdx.x; i <= nb; i += 256) rs[i] = (uint16_t)hist[i];
    // the grouped records go through LDS (the hash keys are dead by now: 16 KB >= 1024 x 12 B) and
    // leave as one linear 16-byte-per-lane copy; scattered 12-byte stores cost the kernel ~15 %
    static_assert(sizeof(unsigned long long) * kHashSlots >= sizeof(EvRec) * kPacket, "staging area");
    EvRec* stage = reinterpret_cast<EvRec*>(hkey);
#pragma unroll
    for (int h = 0; h < 4; ++h)
        if (bin[h] >= 0) {
            EvRec r;
            r.x = ev[h].x;
            r.y = ev[h].y;
            r.m = mult[h];
            stage[hist[bin[h]] + rank[h]] = r;
        }
    __syncthreads();
    {
        const int n16 = (int)((total * (uint32_t)sizeof(EvRec) + 15u) / 16u);  // <= 768
        const uint4* src = reinterpret_cast<const uint4*>(stage);
        uint4* dst = reinterpret_cast<uint4*>(sxy + (size_t)k * kPacket);  // k * 12 KB: 16-byte aligned
        for (int i = threadIdx.x; i < n16; i += 256) dst[i] = src[i];
    }
    if (threadIdx.x == 0) nvalid[k] = total | (big << 31);  // total <= 1024
}

template <bool RAW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_sort_packets(const float2* __restrict__ xy, RawEvents raw,
                                                      int np, int ny,
                                                      int nz, int pad, EvRec* __restrict__ sxy,
                                                      uint32_t* __restrict__ nvalid,
                                                      uint16_t* __restrict__ rowstart)
{
    sort_packets_body<RAW>((int)blockIdx.x, xy, raw, np, ny, nz, pad, sxy, nvalid, rowstart, nullptr, 0);
}

// the packets of up to two cameras in ONE launch (the fused kernel's preparation: a 50 ms window has ~490
// packets per camera, and two launches of ~490 blocks each cost two launch latencies for nothing)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_sort_packets_multi(PrepCameras cams, int ny, int nz, int pad,
                                                                                                       int n_pairs)
{
    int k = (int)blockIdx.x, c = 0;
    while (c + 1 < cams.n && k >= cams.cam[c].np) k -= cams.cam[c++].np;
    const PrepCamera& pc = cams.cam[c];
    sort_packets_body<true>(k, nullptr, pc.raw, pc.np, ny, nz, pad, pc.sxy, pc.nvalid, pc.rowstart, pc.pair_work, n_pairs);
}

// lane mappings 2 and 4 sort groups of packets together (k_sort_groups)
__device__ __host__ __forceinline__ bool grouped(int packed) { return packed == 2 || packed == 4; }

// (2) per (packet, plane): coefficients + for every band the run [lo,hi) of the grouped
//     packet whose Y can fall into the band.  The band's Y interval is mapped back to z0 rows
//     (in double, widened by one row on each side), and the run is read off the packet's
//     rowstart table.  The run is a superset; the voting kernel re-tests every event exactly.
//     A block covers 16 packets x (blockDim / 16) planes and, when they fit (STAGED), first copies
//     the 16 packets' rowstart tables into LDS with coalesced loads: every thread looks up two
//     entries per band at data-dependent positions, and out of global memory those look-ups, not
//     the table writes, bounded the kernel (1024 x 1024 x 256, 10 M events: 440 us, 16 x 16 tiles
//     best; wider tiles for longer write segments were slower).
constexpr int kCoefTilePackets = 16;

// The z0 row bins a band's rows come from: band rows [r0 - halo, min(r1, ny - 1)] -> y0 = Y * d_a - by_a (fp32; its rounding,
// <= 4e-7 of |y0| + |by/a|, disappears in the widening) -> entries of the packet's row table: the run is
// [rs[*bin_lo], rs[*bin_hi]).  false: a NaN bound -- the run is the whole packet.  ONE function for k_plane_coef's cut
// table and for the vector fill's inline cuts (BandPlan::cuts_inline), so that both take the same runs.
__device__ __forceinline__ bool band_row_bins(float d_a, float by_a, float L, float U, int ny, int pad, int* bin_lo, int* bin_hi)
{
    const float ya = L * d_a - by_a, yb = U * d_a - by_a;
    float ymin = fminf(ya, yb), ymax = fmaxf(ya, yb);
    if (!(ya == ya && yb == yb)) return false;
    // the fp32 forward map (mul, add, divide) is within a few ulps of the real
    // one: in y0 units that is ~2^-22 * (|y0| + |by/a|); widen by 80x that
    const float m = 2e-5f * (fmaxf(fabsf(ymin), fabsf(ymax)) + fabsf(by_a));
    ymin -= m;
    ymax += m;
    const float fa = fminf(fmaxf(__builtin_floorf(ymin), (float)(-pad - 1)), (float)(ny + pad));
    const float fb = fminf(fmaxf(__builtin_floorf(ymax), (float)(-pad - 1)), (float)(ny + pad));
    *bin_lo = (int)fa + pad + 1;  // events in bins below bin(fa)
    *bin_hi = (int)fb + pad + 2;  // events in bins up to and including bin(fb)
    return true;
}
// (the band's accepted Y interval: accepted iff 0 <= Y < ny-1; the band needs floor(Y) in [r0, r1-1]; bp.halo: the fused
//  kernel's bands also take the events of the row above their first)
__device__ __forceinline__ void band_y_interval(int j, const Geom& g, const BandPlan& bp, float* L, float* U)
{
    const int r0 = j * bp.band_rows;
    const int r1 = min(g.ny, r0 + bp.band_rows);
    *L = (float)(r0 - bp.halo) - 0.01f;
    *U = (float)min(r1, g.ny - 1) + 0.01f;
}

template <bool STAGED>
__device__ __forceinline__ void plane_coef_body(const unsigned bid, const float* __restrict__ centers,
                                                const float* __restrict__ planes,
                                                const uint16_t* __restrict__ rowstart,
                                                uint32_t* __restrict__ nvalid, int np,
                                                const Geom& g, const BandPlan& bp,
                                                PlaneCoef* __restrict__ coef,
                                                uint32_t* __restrict__ cuts, uint32_t* __restrict__ pair_work)
{
    // 16 consecutive packets per plane make the plane-major tables (coef[z][p], cuts[band][z][p])
    // 64-byte coalesced writes
    extern __shared__ uint16_t s_rowstart[];  // STAGED: [16][nb + 1]
    // Block b runs on XCD b % 8 (the dispatch rule the voting kernel relies on too).  Eight tiles that
    // are neighbours along the packet axis -- the eight 64-byte pieces of a 512-byte stretch of every
    // table row -- go to eight consecutive blocks of ONE XCD, so that they meet in that XCD's L2 and
    // leave it as whole lines (dealt round-robin over the XCDs, every line was written in pieces:
    // 1024 x 1024 x 256, 10 M events: 422 us; groups of four 365 us; groups of eight 337 us).
    const int tiles_p = (np + kCoefTilePackets - 1) / kCoefTilePackets;
    const unsigned tile = (bid >> 6) * 64u + (bid & 7u) * 8u + ((bid >> 3) & 7u);
    const int planes_per_block = (int)(blockDim.x >> 4);
    if (tile >= (unsigned)tiles_p * (unsigned)((g.nz + planes_per_block - 1) / planes_per_block)) return;
    const int k0 = (int)(tile % (unsigned)tiles_p) * kCoefTilePackets;
    const int k = k0 + (int)(threadIdx.x & 15);
    const int z = (int)(tile / (unsigned)tiles_p) * planes_per_block + (int)(threadIdx.x >> 4);
    const int pad = bp.row_pad;
    const int nb = g.ny + 2 * pad + 2;
    if (STAGED && !(bp.cuts_inline && !pair_work)) {
        // the tile's tables are one contiguous piece of rowstart, 4-byte aligned (k0 is even); the
        // last 32-bit word may reach one element past the piece (the buffer has that slack)
        const int count = min(kCoefTilePackets, np - k0) * (nb + 1);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(rowstart + (size_t)k0 * (nb + 1));
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_rowstart);
        for (int i = threadIdx.x; i < (count + 1) / 2; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    // (with pair_work the threads beyond the tables stay: the row reductions below need whole rows of lanes;
    //  they act as dead packets and store nothing)
    const bool valid = k < np && z < g.nz;
    if (!valid && !pair_work) return;
    const int kq = valid ? k : 0, zq = valid ? z : 0;
    const size_t tid = (size_t)zq * np + kq;
    PlaneCoef c;
    plane_coefficients(centers[3 * kq], centers[3 * kq + 1], centers[3 * kq + 2], planes[zq], g, c.a,
                       c.bx, c.by, c.d);
    c.r = 1.f / c.d;
    const uint32_t nvraw = !valid ? 0u : (grouped(bp.packed) ? 1u : nvalid[kq]);
    const int nv = (int)(nvraw & 0x7fffffffu);
    const bool big_events = (nvraw >> 31) != 0;
    // Which (packet, plane) pairs can vote at all?  NaN anywhere, d == 0, or an
    // infinite a / bx / by make X or Y non-finite for every event.
    const bool dead = !(c.a == c.a) || !(c.bx == c.bx) || !(c.by == c.by) || !(c.d == c.d) ||
                      c.d == 0.f || !finitef(c.a) || !finitef(c.bx) || !finitef(c.by) || nv == 0;
    const float ad = fabsf(c.d);
    // "slow": the residual-corrected division is only proven for 2^-40 <= |d| <= 2^40; with
    // |x0|, |y0|, |a|, |bx|, |by| <= 2^40 as well, no intermediate of the fast path can overflow,
    // so X and Y are finite there and the voting kernel needs no NaN / overflow guards
    const bool slow = !dead && (!(ad >= 0x1p-40f && ad <= 0x1p40f) /* incl. d = +-inf */ ||
                                big_events || fabsf(c.a) > 0x1p40f || fabsf(c.bx) > 0x1p40f ||
                                fabsf(c.by) > 0x1p40f);
    // y0 = (Y*d - by)/a inverts the transfer; unusable when the map is (nearly) constant or
    // the inversion is ill-conditioned -- then the whole packet is the (superset) run
    const double a = (double)c.a, d = (double)c.d, by = (double)c.by;
    const bool invertible = !dead && !slow && fabs(a) > 1e-3 * fabs(d);
    const double inv_a = 1.0 / a;
    // y0 = Y * d_a - by_a, per band in fp32: its rounding (<= 4e-7 of |y0| + |by/a|) disappears in the
    // widening below, and 2 x bands x planes x packets double-precision chains were what the kernel
    // spent its time on
    const float by_a = (float)(by * inv_a), d_a = (float)(d * inv_a);
    // The inline cuts (BandPlan::cuts_inline) widen every band's interval by ONE bound per (packet, plane), M >= the
    // 2e-5 * (|y0| + |by/a|) of band_row_bins for every band (|y0| <= (ny + 1) |d/a| + |by/a|), in 1/256 rows in the high half of
    // flags; they only trust d_a / by_a where every band's y0 stays far inside the int32 range of v_cvt_flr_i32_f32.
    const float margin = 2e-5f * ((float)(g.ny + 1) * fabsf(d_a) + 2.f * fabsf(by_a));
    const bool inline_ok = invertible && fabsf(d_a) <= 1e4f && fabsf(by_a) <= 1e8f && margin <= 200.f;
    const uint32_t margin_q = inline_ok ? (uint32_t)__builtin_ceilf(margin * 256.f) + 1u : 0u;
    c.flags = (dead ? kCoefSkip : (slow ? kCoefSlow : 0u)) | (inline_ok ? kCoefInvertible : 0u) | (margin_q << 16);
    c.d_a = d_a;
    c.by_a = by_a;
    if (valid) coef[tid] = c;
    if (slow) atomicOr(&nvalid[np + zq], 1u);  // (slow implies valid: nv > 0)
    // no cut table: the voting kernel's passes derive their runs themselves (BandPlan::cuts_inline)
    if (bp.cuts_inline && !pair_work) return;

    const uint16_t* rs = STAGED ? s_rowstart + (size_t)(threadIdx.x & 15) * (nb + 1)
                                : rowstart + (grouped(bp.packed) ? 0 : (size_t)kq * (nb + 1));
    for (int j = 0; j < bp.bands; ++j) {
        uint32_t lo = 0, hi = 0;
        if (!dead) {
            hi = (uint32_t)nv;
            if (invertible) {
                float L, U;
                band_y_interval(j, g, bp, &L, &U);
                int bin_lo, bin_hi;
                if (band_row_bins(d_a, by_a, L, U, g.ny, pad, &bin_lo, &bin_hi)) {  // not NaN
                    if (grouped(bp.packed)) {  // grouped mapping: row bins, resolved per group later
                        lo = (uint32_t)bin_lo;
                        hi = (uint32_t)bin_hi;
                    } else {
                        lo = rs[bin_lo];
                        hi = rs[bin_hi];
                    }
                } else if (grouped(bp.packed)) {
                    lo = 0;
                    hi = (uint32_t)nb;
                }
            } else if (grouped(bp.packed)) {
                lo = 0;
                hi = (uint32_t)nb;  // whole packet = all row bins
            }
            if (hi < lo) hi = lo;
        } else if (grouped(bp.packed)) {
            lo = 0xffffu;  // dead packet: contributes no rows
            hi = 0;
        }
        if (valid && !bp.cuts_inline) cuts[((size_t)j * g.nz + zq) * np + kq] = lo | (hi << 16);  // 16 bits each
        if (pair_work) {
            // records of this (band, plane) over the 16 packets of the tile (lanes 16 i .. 16 i + 15 of a wave
            // share the plane): a row reduction, then one atomic per (band, plane, tile)
            int len = (int)hi - (int)lo;
            len += __builtin_amdgcn_update_dpp(0, len, 0x111, 0xf, 0xf, true);  // row_shr:1
            len += __builtin_amdgcn_update_dpp(0, len, 0x112, 0xf, 0xf, true);  // row_shr:2
            len += __builtin_amdgcn_update_dpp(0, len, 0x114, 0xf, 0xf, true);  // row_shr:4
            len += __builtin_amdgcn_update_dpp(0, len, 0x118, 0xf, 0xf, true);  // row_shr:8
            if ((threadIdx.x & 15) == 15 && len > 0 && z < g.nz) atomicAdd(&pair_work[j * g.nz + z], (uint32_t)len);
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(1024) void k_plane_coef(const float* __restrict__ centers,
                                                    const float* __restrict__ planes,
                                                    const uint16_t* __restrict__ rowstart,
                                                    uint32_t* __restrict__ nvalid, int np,
                                                    Geom g, BandPlan bp,
                                                    PlaneCoef* __restrict__ coef,
                                                    uint32_t* __restrict__ cuts)
{
    plane_coef_body<STAGED>(blockIdx.x, centers, planes, rowstart, nvalid, np, g, bp, coef, cuts, nullptr);
}

// the coefficient / cut tables of up to four cameras in one launch; camera c's blocks follow camera c - 1's
struct PrepBlocks {
    unsigned n[kFusedMaxCameras];  // blocks of camera c
};

template <bool STAGED>
__global__ __launch_bounds__(1024) void k_plane_coef_multi(PrepCameras cams, BandPlan bp, PrepBlocks blocks)
{
    unsigned bid = blockIdx.x;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kFusedMaxCameras - 1; ++k)
        if (c == k && cams.n > k + 1 && bid >= blocks.n[k]) {
            bid -= blocks.n[k];
            c = k + 1;
        }
    const PrepCamera& pc = cams.cam[c];
    plane_coef_body<STAGED>(bid, pc.raw.centers, pc.planes, pc.rowstart, pc.nvalid, pc.np, pc.raw.g, bp, pc.coef, pc.cuts, pc.pair_work);
}

// (2b) BandPlan::cuts_inline: the packets' row tables TRANSPOSED -- rsT[bin][packet], rows of `stride` packets -- so
//      that a pass of the vector fill (lane = packet, 64 consecutive packets whose poses are microseconds apart: their
//      bins for one band and plane differ by a row or two) reads its two entries per packet from one or two 128-byte
//      pieces.  64 packets x 64 bins per block through LDS.
__global__ __launch_bounds__(256) void k_transpose_rowstart(const uint16_t* __restrict__ rs, int np, int nb1, int stride,
                                                            uint16_t* __restrict__ rsT)
{
    __shared__ uint16_t tile[64][66];
    const int p0 = (int)blockIdx.x * 64, b0 = (int)blockIdx.y * 64;
    {
        const int bin = b0 + (int)(threadIdx.x & 63);
        for (int i = (int)(threadIdx.x >> 6); i < 64; i += 4) {
            const int p = p0 + i;
            tile[i][threadIdx.x & 63] = (p < np && bin < nb1) ? rs[(size_t)p * nb1 + bin] : (uint16_t)0;
        }
    }
    __syncthreads();
    const int p = p0 + (int)(threadIdx.x & 63);
    if (p >= stride) return;
    for (int i = (int)(threadIdx.x >> 6); i < 64; i += 4) {
        const int bin = b0 + i;
        if (bin < nb1) rsT[(size_t)bin * stride + p] = tile[threadIdx.x & 63][i];
    }
}

// (3) the voting kernel.  Work item = (packet chunk c, band j, plane z): the band's
//     rows [r0-1, r1] of plane z live in LDS (two halo rows, so a bilinear vote never
//     needs a row test), every wave walks packets of the chunk with the packet's
//     coefficients in SGPRs, and the owned rows [r0, r1) are written back with plain
//     coalesced stores -- no global atomics, no memset.
//
//     Block b runs on XCD b % 8 (observed dispatch rule): the blocks of one XCD walk
//     the planes of ONE (chunk, band) pair at a time, so its events stream through
//     that XCD's L2 once instead of once per plane.
// LDS accumulators are 64-bit fixed point (Q33.31), voted with ds_add_u64 (no return).
// Measured on gfx950 (tools/lds_atomic_bench2.hip, cycles per wave instruction, random band
// addresses): ds_add_f32 ~185 (lanes serialised), ds_add_u64 ~11, ds_add_u32 ~6.5.  A 32-bit
// Q8.24 word + carry counter was tried (needs the returning form to detect wraps): the wait
// for the returned value cost more than the cheaper atomic saved (3.5 vs 4.3 Gev/s).
// A weight w = fl(fx*fy) in [0,1] is added as trunc(w * 2^31): exact for w >= 2^-8, off by
// < 2^-31 below, so a voxel holds the EXACT sum of its fp32 weights (to 5e-10 per vote),
// independent of vote order, and is rounded to fp32 once at write-back.  (The CPU reference
// rounds after every += instead.)
using acc_t = unsigned long long;
// k_vote_fuse_argmax keeps two fp32 values and a plane index per band cell in registers: 1024-cell stretches per
// thread.  20 cover the whole LDS (160 KB of 8-byte cells); the vector-fill mappings leave fewer registers: 16.
constexpr int kFusedTracePhases = 64;
__host__ __device__ constexpr int fused_cells_per_thread(int mapping) { return (mapping == 5 || mapping == 6) ? 16 : 20; }
constexpr int kFusedCellsFourCameras = 16;  // four cameras keep TWO fp32 arrays per thread beside the running maxima
constexpr int kFusedCellsTwoPerCu = 10;  // k_vote_fuse_argmax_2cu: half the LDS per workgroup = 10 x 1024 cells
constexpr float kFixScale = 2147483648.f;      // 2^31
constexpr double kFixInv = 1.0 / 2147483648.0;  // 2^-31

// Q33.31 sum -> fp32, ONE rounding (to nearest, ties to even) for EVERY v < 2^64: the contract of DESIGN.md
// ("GPU vs oracle"), asserted bit for bit by tests/test_gpu_exact_voxels.py (sums of 2^52 and more:
// test_large_sums_are_rounded_once) against oracle.q31_to_float.
//
// Any v: below 2^53 the double of v is exact, and the conversion to fp32 rounds once.  From 2^53 up
// (double)v would round first, and rounding that double to fp32 again can go wrong (2^53 + 2^30 + 2^29 - 1
// -> 4194305.0 instead of 4194304.5).  There the low 11 bits are folded into bit 11 as one sticky bit
// (round to odd): they lie below fp32's rounding bit (bit 29 at the least), so the folded value rounds to
// fp32 exactly as v does, and with no set bit below bit 11 it is exact in a double.  (32-bit operations on
// the low word only: the fused kernel's read-back converts a wave of these next to its register-resident
// state.)
__device__ __forceinline__ float fix_to_float_any(acc_t v)
{
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t folded = (lo & ~0x7ffu) | (((lo & 0x7ffu) + 0x7ffu) & 0x800u);
    const acc_t w = ((acc_t)hi << 32) | (hi >= (1u << 21) ? folded : lo);
    return (float)((double)w * kFixInv);
}

// For v < 2^52 the double whose bits are (1044 << 52) | v is exactly 2^21 + v * 2^-31; subtracting 2^21 is
// exact, so two double-rate instructions replace the 64-bit integer -> double conversion (two conversions, a
// scale and an add).
__device__ __forceinline__ float fix_to_float_narrow(acc_t v)
{
    return (float)(__longlong_as_double((long long)(v | 0x4140000000000000ull)) - 2097152.0);
}

__device__ __forceinline__ float fix_to_float(acc_t v)
{
    if (__builtin_expect((v >> 52) == 0ull, 1)) return fix_to_float_narrow(v);
    return fix_to_float_any(v);  // sums of 2^52 and more (> 2 M votes in one voxel)
}

// the four bilinear votes of m identical events (cartesian3dgrid.h:261-270) into the band
__device__ __forceinline__ void vote4(acc_t* __restrict__ band, int idx, int nx, float fx, float fy,
                                      uint32_t m)
{
    const float fx1 = 1.f - fx, fy1 = 1.f - fy;
    // scaling one factor by 2^31 scales the rounded product exactly; w * 2^31 <= 2^31 fits u32;
    // m votes of trunc(w * 2^31) are one vote of m * trunc(w * 2^31) (v_mad_u64_u32), exactly
    const float fxs = fx * kFixScale, fx1s = fx1 * kFixScale;
    acc_t* cell = band + idx;
    __hip_atomic_fetch_add(cell, (acc_t)(unsigned int)(fx1s * fy1) * m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(cell + 1, (acc_t)(unsigned int)(fxs * fy1) * m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(cell + nx, (acc_t)(unsigned int)(fx1s * fy) * m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(cell + nx + 1, (acc_t)(unsigned int)(fxs * fy) * m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- lane mapping 8: PAIRED 32-bit cells (dsi_vote_asm.h, DSI_ASM_VOTE_PAIRED19) ----
constexpr int kPairedFracBits = 19;                       // Q.19 weights, rounded
constexpr uint32_t kPairedGuard = 0x80000000u;            // a sub-cell at or above this is reported (4,096 full votes)
__host__ __device__ inline int paired_row_words(int nx) { return 2 * ((nx >> 1) + 1); }  // 8-byte words per band row

__device__ __forceinline__ uint32_t cvt_rpi(float x)  // floor(x + 0.5), the instruction the hand-scheduled vote uses
{
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return (uint32_t)r;
}

// the compiled twin of DSI_ASM_VOTE_PAIRED19's tail (the IEEE-divide planes of mapping 8 use it): same operations, same bits
__device__ __forceinline__ void vote_paired(char* __restrict__ band_bytes, int xi, int yi, int row_bytes, int cbase, float fx,
                                            float fy, uint32_t m)
{
    const float fy1 = 1.f - fy;
    const float S = 524288.f * (float)m;  // m * 2^19, exact (m <= 1024)
    const float fxs = S * fx, fx1s = S - fxs;
    const uint32_t w00 = cvt_rpi(fx1s * fy1), w10 = cvt_rpi(fxs * fy1);
    const uint32_t w01 = cvt_rpi(fx1s * fy), w11 = cvt_rpi(fxs * fy);
    acc_t* word = reinterpret_cast<acc_t*>(band_bytes + (__mul24(yi, row_bytes) + (((xi >> 1) << 3) + cbase) + (xi & 1) * (row_bytes >> 1)));
    __hip_atomic_fetch_add(word, (acc_t)w00 | ((acc_t)w10 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    acc_t* below = reinterpret_cast<acc_t*>(reinterpret_cast<char*>(word) + row_bytes);
    __hip_atomic_fetch_add(below, (acc_t)w01 | ((acc_t)w11 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the raw sum of cell x of a paired row, as the Q33.31 value the exact mappings hold (so that seam rows, partial volumes
// and the one rounding to fp32 are theirs); *guard |= a sub-cell reached kPairedGuard
__device__ __forceinline__ acc_t paired_cell(const uint2* __restrict__ row, int rw, int x, uint32_t* guard)
{
    const int k = x >> 1;
    uint32_t a, b;
    if (x & 1) {
        a = row[k].y;        // votes at xi = x - 1 (even): W_k's upper cell
        b = row[rw + k].x;   // votes at xi = x (odd):      V_k's lower cell
    } else {
        a = row[k].x;                            // votes at xi = x (even): W_k's lower cell
        b = k > 0 ? row[rw + k - 1].y : 0u;      // votes at xi = x - 1 (odd): V_(k-1)'s upper cell
    }
    *guard |= (a | b) & kPairedGuard;
    return ((acc_t)a + (acc_t)b) << (31 - kPairedFracBits);
}

// owned rows of the band -> fp32 volume (a linear, coalesced copy).  A vote of an event in the band's
// last owned row also lands in the row below, which is the next band's first row: that "carry" row,
// and the next band's own sums for its first row (its "head"), leave the CU as the raw 64-bit
// fixed-point sums -- seam[c][z][j][0][x] = head of band j (j >= 1), seam[c][z][j][1][x] = carry of
// band j (j < bands - 1) -- and k_seam_rows writes fl((head + carry) * 2^-31) into the volume: ONE
// rounding of the exact sum, like every other voxel.  The DSI therefore does not depend on the band
// decomposition (round 2 added fl(carry) to fl(head) in fp32: two roundings on seam rows).  A band
// processes exactly the events with floor(Y) in its OWNED rows: no event is processed by two bands.
__device__ __forceinline__ acc_t* seam_rows(acc_t* seam, int c, int z, int j, const Geom& g, const BandPlan& bp)
{
    return seam + ((((size_t)c * g.nz + z) * bp.bands + j) * 2) * g.nx;
}

// `out` + `off`: the band's first owned voxel in the chunk's volume -- fp32 (the DSI itself: one chunk, no
// accumulation) or, raw != 0, the chunk's PARTIAL volume of raw 64-bit sums, which k_reduce_partials adds up
// exactly over the chunks before the one rounding to fp32: the DSI is fl(exact sum of all votes) for any
// number of chunks as well.
// Work item b -> (pair q = (chunk, band), plane z); false: the block has nothing to do.
// Block b runs on XCD b % 8 (observed dispatch rule).  Groups of 8 pairs: XCD x walks the planes of pair 8k + x, so
// that pair's events stream through that XCD's L2 once instead of once per plane.  The pairs % 8 pairs left over:
// 1, 2 or 4 of them share the XCDs evenly (8, 4 or 2 XCDs each, the planes dealt among those: their events
// stream through 8 / L L2s); any other count is dealt plane by plane over all XCDs (round 2's rule for all).
__device__ __forceinline__ bool item_of(int b, int pairs, int nz, int& q, int& z, bool spread_all = false)
{
    const int full_pairs = (pairs / 8) * 8, full = full_pairs * nz;
    if (b < full) {
        const int xcd = b & 7, s = b >> 3;
        q = (s / nz) * 8 + xcd;
        z = s % nz;
        return true;
    }
    const int r = b - full, L = pairs - full_pairs;
    if ((L == 1 || L == 2 || L == 4) && !spread_all) {  // (spread_all: round 2's rule, experiments builds only)
        const int per = 8 / L, xcd = r & 7, s = r >> 3;  // (full is a multiple of 8: r & 7 == b & 7)
        q = full_pairs + xcd / per;
        z = s * per + xcd % per;
        return z < nz;
    }
    q = full_pairs + r / nz;
    z = r % nz;
    return q < pairs;
}

__host__ __device__ inline int item_count(int pairs, int nz, bool spread_all = false)
{
    const int full_pairs = (pairs / 8) * 8, L = pairs - full_pairs;
    if ((L == 1 || L == 2 || L == 4) && !spread_all) return full_pairs * nz + 8 * ((nz + 8 / L - 1) / (8 / L));
    return pairs * nz;
}

template <int BLOCK, bool CLEAR>
__device__ __forceinline__ void flush_band_t(acc_t* __restrict__ band, int nx, int n_out, void* __restrict__ out, size_t off,
                                             int raw, acc_t* __restrict__ seam_j, int j, int bands)
{
    const int head = j >= 1 ? nx : 0;  // cells that go to the seam buffer instead of the volume
    float* __restrict__ dstf = reinterpret_cast<float*>(out) + off;
    acc_t* __restrict__ dstr = reinterpret_cast<acc_t*>(out) + off;
    for (int i = threadIdx.x; i < n_out; i += BLOCK) {
        const acc_t v = band[i];
        if (i < head)
            seam_j[i] = v;
        else if (raw)
            dstr[i] = v;
        else
            dstf[i] = fix_to_float(v);  // exact in f64, one rounding to f32
        if (CLEAR) band[i] = 0;
    }
    acc_t* src = band + n_out;
    for (int i = threadIdx.x; i < nx; i += BLOCK) {
        if (j < bands - 1) seam_j[nx + i] = src[i];
        if (CLEAR) src[i] = 0;
    }
}

template <int BLOCK>
__device__ __forceinline__ void flush_band(acc_t* __restrict__ band, int nx, int n_out, void* __restrict__ out, size_t off,
                                           int raw, acc_t* __restrict__ seam_j, int j, int bands)
{
    flush_band_t<BLOCK, false>(band, nx, n_out, out, off, raw, seam_j, j, bands);
}

// the same, leaving the band zeroed for the workgroup's next work item (persistent kernel)
template <int BLOCK>
__device__ __forceinline__ void flush_band_and_clear(acc_t* __restrict__ band, int nx, int n_out, void* __restrict__ out,
                                                     size_t off, int raw, acc_t* __restrict__ seam_j, int j, int bands)
{
    flush_band_t<BLOCK, true>(band, nx, n_out, out, off, raw, seam_j, j, bands);
}

// flush_band_t for a band of PAIRED cells (lane mapping 8): a cell's two parts are added, scaled to Q33.31 and leave the CU the
// way the exact sums do.  n_rows owned rows + the carry row; the band is always cleared (persistent or not, it is cheap).
// overflow: one word, set when a sub-cell reached the guard (2^31: half its capacity) -- the caller re-runs in an exact mode.
template <int BLOCK>
__device__ __forceinline__ void flush_band_paired(acc_t* __restrict__ band, int nx, int n_rows, void* __restrict__ out, size_t off,
                                                  int raw, acc_t* __restrict__ seam_j, int j, int bands,
                                                  uint32_t* __restrict__ overflow)
{
    const int rw = (nx >> 1) + 1;
    const uint2* __restrict__ words = reinterpret_cast<const uint2*>(band);
    float* __restrict__ dstf = reinterpret_cast<float*>(out) + off;
    acc_t* __restrict__ dstr = reinterpret_cast<acc_t*>(out) + off;
    const int head = j >= 1 ? nx : 0;  // cells that go to the seam buffer instead of the volume
    const int n_out = n_rows * nx;
    uint32_t guard = 0u;
    for (int i = threadIdx.x; i < n_out + nx; i += BLOCK) {  // (the last nx: the carry row)
        const int r = i / nx, x = i - r * nx;
        const acc_t v = paired_cell(words + (size_t)r * 2 * rw, rw, x, &guard);
        if (i >= n_out) {
            if (j < bands - 1) seam_j[nx + (i - n_out)] = v;
        } else if (i < head)
            seam_j[i] = v;
        else if (raw)
            dstr[i] = v;
        else
            dstf[i] = fix_to_float(v);
    }
    if (__builtin_amdgcn_ballot_w64(guard != 0u) != 0ull && (threadIdx.x & 63) == 0) atomicOr(overflow, 1u);
    __syncthreads();  // every cell has been read
    const int all_words = (n_rows + 1) * 2 * rw;
    for (int i = threadIdx.x; i < all_words; i += BLOCK) band[i] = 0;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_vote_bands(const EvRec* __restrict__ sxy,
                                                      const PlaneCoef* __restrict__ coef,
                                                      const uint32_t* __restrict__ cuts, int np,
                                                      Geom g, BandPlan bp,
                                                      void* __restrict__ out,
                                                      acc_t* __restrict__ seam)
{
    extern __shared__ acc_t band[];
    // block -> (pair q = (chunk, band), plane z).  Groups of 8 pairs: XCD x (= block % 8) walks
    // the planes of pair 8k + x.  The last (pairs % 8) pairs are dealt plane by plane over all
    // XCDs so that no XCD idles (their events then stream through every L2).
    const int b = blockIdx.x;
    const int pairs = bp.chunks * bp.bands;
    int q, z;
    if (!item_of(b, pairs, g.nz, q, z, bp.experiment == 200)) return;
    const int c = q / bp.bands, j = q % bp.bands;
    const int r0 = j * bp.band_rows;
    const int r1 = min(g.ny, r0 + bp.band_rows);
    const int nx = g.nx;
    const int cells = (r1 - r0 + 1) * nx;  // owned rows + the carry row
    for (int i = threadIdx.x; i < cells; i += BLOCK) band[i] = 0;
    __syncthreads();

    const int p_begin = (int)(((long long)np * c) / bp.chunks);
    const int p_end = (int)(((long long)np * (c + 1)) / bp.chunks);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int lane = threadIdx.x & (kWave - 1);
    const float L = (float)r0, U = (float)min(r1, g.ny - 1);
    const float xmax = (float)(nx - 1);
    const int row_base = r0;

    // Per-packet metadata (coefficients + this band's run) is fetched with VECTOR loads whose
    // address is the same in every lane, one packet ahead of its use: scalar loads would
    // share lgkmcnt with the LDS atomics and serialise flags -> cuts -> coefficients.
    constexpr int kStride = BLOCK / kWave;
    const uint4* __restrict__ coef4 = reinterpret_cast<const uint4*>(coef);
    const size_t coef_base = (size_t)z * np;                 // coef[z][p]
    const size_t cuts_base = ((size_t)j * g.nz + z) * np;    // cuts[band][z][p]
    auto fetch_meta = [&](int p, uint4& m0, uint2& m1, uint32_t& cu) {
        size_t pz = coef_base + p;
        asm volatile("" : "+v"(pz));  // keep the address in VGPRs => global_load, counted by vmcnt
        m0 = coef4[2 * pz];
        m1 = *reinterpret_cast<const uint2*>(coef4 + 2 * pz + 1);
        cu = cuts[cuts_base + (pz - coef_base)];
    };
    int p = p_begin + wave;
    uint4 m0 = make_uint4(0, 0, 0, 0), n0 = m0;
    uint2 m1 = make_uint2(0, kCoefSkip), n1 = m1;
    uint32_t mcu = 0, ncu = 0;
    if (p < p_end) fetch_meta(p, m0, m1, mcu);
    for (; p < p_end; p += kStride) {
        // unpack the current packet first (this is where its loads are waited for), THEN put
        // the next packet's metadata in flight so that it overlaps this packet's votes
        const float ka = __uint_as_float(__builtin_amdgcn_readfirstlane(m0.x));
        const float kbx = __uint_as_float(__builtin_amdgcn_readfirstlane(m0.y));
        const float kby = __uint_as_float(__builtin_amdgcn_readfirstlane(m0.z));
        const float kd = __uint_as_float(__builtin_amdgcn_readfirstlane(m0.w));
        const float kr = __uint_as_float(__builtin_amdgcn_readfirstlane(m1.x));
        const uint32_t flags = __builtin_amdgcn_readfirstlane(m1.y);
        const uint32_t cu = __builtin_amdgcn_readfirstlane(mcu);
        const int lo = (int)(cu & 0xffffu), hi = (int)(cu >> 16);
        const int pn = p + kStride;
        n1 = make_uint2(0, kCoefSkip);
        if (pn < p_end) fetch_meta(pn, n0, n1, ncu);
        if (!(flags & kCoefSkip) && lo < hi) {
            const EvRec* __restrict__ ev = sxy + (size_t)p * kPacket;
            const bool slow = (flags & kCoefSlow) != 0;
            int i = lo + lane;
            EvRec e = {0.f, 0.f, 0u};
            if (i < hi) e = ev[i];
            for (int base = lo; base < hi; base += kWave) {
                // prefetch the next 64 events of the run while this batch is voted
                const int inext = i + kWave;
                EvRec en = e;
                if (inext < hi) en = ev[inext];
                if (i < hi) {
                    const float nxv = e.x * ka + kbx;  // mapper_emvs_stereo.cpp:194-195
                    const float nyv = e.y * ka + kby;
                    float X, Y;
                    if (slow) {
                        X = nxv / kd;
                        Y = nyv / kd;
                    } else {
                        X = div_rc(nxv, kd, kr);
                        Y = div_rc(nyv, kd, kr);
                    }
                    // cartesian3dgrid.h:255-259 restricted to this band's rows.  (Voting rejected
                    // events into a spare cell instead of branching was tried: 12 % slower.)
                    if (X >= 0.f && X < xmax && Y >= L && Y < U) {
                        const float xf = __builtin_floorf(X), yf = __builtin_floorf(Y);
                        const int idx = __mul24((int)yf - row_base, nx) + (int)xf;
                        vote4(band, idx, nx, X - xf, Y - yf, e.m);  // cartesian3dgrid.h:261-270
                    }
                }
                e = en;
                i = inext;
            }
        }
        m0 = n0;
        m1 = n1;
        mcu = ncu;
    }
    __syncthreads();

    // owned rows are contiguous in the [z][y][x] volume: a linear coalesced copy
    const size_t vol = partial_stride((size_t)g.nx * g.ny * g.nz);
    const size_t off = (size_t)c * vol + ((size_t)z * g.ny + r0) * nx;
    flush_band<BLOCK>(band, nx, (r1 - r0) * nx, out, off, bp.raw_out, seam_rows(seam, c, z, j, g, bp), j, bp.bands);
}

// (3b) the same work item decomposition for SHORT runs (tall or wide grids: a band of a
//     1024-wide plane sees ~20 events of a packet).  A wave takes 64 packets at a time,
//     appends their runs back to back into its 64 lanes and votes whenever the lanes are
//     full, so lane utilisation no longer depends on the run length.  Coefficients are then
//     per lane (gathered from the plane-major table), not per wave.
// floor(X) as an integer in one instruction (saturating, NaN -> 0), instead of floor + convert
__device__ __forceinline__ int floor_to_int(float x)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// The stream of one wave.  SLOW = the plane has coefficient sets outside the range where the
// residual-corrected division is proven (or events / coefficients above 2^40): every lane then
// takes the IEEE divide and the accept test also guards against inf / inf.
//
// Issue rates measured on gfx950 (tools/valu_rate_bench.hip, wave-instructions / clk / CU):
// fp32 add/mul/fma and plain integer add/sub/logic/shift ~1.6-2, everything else (conversions,
// floor/fract, three-operand integer ops, compares, v_cndmask, 24-bit and 64-bit multiplies)
// ~0.95, and v_pk_*_f32 0.95 (no gain over two scalar ops).  The loop below is bound by VALU
// issue, so it is written to need few instructions of the second kind.
template <bool SLOW, bool PAIRED = false>
__device__ __forceinline__ void packed_stream(const EvRec* __restrict__ sxy,
                                              const uint4* __restrict__ coef4,
                                              const uint32_t* __restrict__ cutz,
                                              char* __restrict__ band_bytes, int p_first,
                                              int p_end, int lg_group, int stride, int lane,
                                              int nx, int Li, int Ui, int row_base,
                                              uint32_t dummy_eo, int row_bytes = 0)
{
    // ---- the run stream (all wave-uniform).  The wave owns packets i = 0 .. n_my-1:
    //      packet i is p_first + (i >> lg_group) * stride + (i & (group-1)); it contributes the
    //      records [off, hi) of its grouped storage.
    const int group = 1 << lg_group;
    int n_my = 0;
    if (p_first < p_end) {
        const int passes = (p_end - p_first + stride - 1) / stride;         // >= 1
        const int last = p_first + (passes - 1) * stride;
        n_my = (passes - 1) * group + min(group, p_end - last);
    }
    n_my = __builtin_amdgcn_readfirstlane(n_my);  // (the division runs on the vector unit)
    int i = -1;
    int cur = 0, end = 0;  // absolute record indices (packet * 1024 + slot) of the current run
    int pbase = 0;         // current packet * 1024
    uint32_t mycu = 0;     // lane l: cut word of packet l of the current pass
    uint32_t eo = 0;       // per lane: the record the lane takes next
    const int gmask = __builtin_amdgcn_readfirstlane(group - 1);

    // Append runs to the lanes until 64 are taken or the stream ends; returns the lanes taken.
    // The bookkeeping is scalar work, and the CU issues ONE scalar instruction per clock (for
    // all its waves): compiled from C++ this loop cost ~60 scalar instructions per batch and
    // bounded the kernel (PMC: SQ_INSTS_SALU ~ SQ_INSTS_VALU).  Hand-scheduled: 11 per run
    // piece + 13 per packet, and the lane update is one VALU add under a shifted exec mask
    // (lanes [fill, 64) take consecutive records; those beyond the run are overwritten by the
    // next piece, or retired to the multiplicity-0 record when the stream ends).
    auto fill_batch = [&]() -> int {
        int fill = 0;
        for (;;) {
            int status, t0, t1;
            // (all wave-uniform already; the readfirstlanes only pin them to scalar registers)
            cur = __builtin_amdgcn_readfirstlane(cur);
            end = __builtin_amdgcn_readfirstlane(end);
            i = __builtin_amdgcn_readfirstlane(i);
            pbase = __builtin_amdgcn_readfirstlane(pbase);
            fill = __builtin_amdgcn_readfirstlane(fill);
            asm volatile(
                "Ltop%=:\n\t"
                "s_cmp_ge_i32 %0, %1\n\t"
                "s_cbranch_scc1 Lnext%=\n\t"
                "s_sub_i32 %7, 64, %4\n\t"        // room in the batch
                "s_sub_i32 %8, %1, %0\n\t"        // records left in the run
                "s_min_i32 %7, %7, %8\n\t"        // take
                "s_sub_i32 %8, %0, %4\n\t"        // record of lane 0 if the run started there
                "s_lshl_b64 exec, -1, %4\n\t"     // lanes >= fill
                "v_add_u32 %5, %8, %11\n\t"
                "s_mov_b64 exec, -1\n\t"
                "s_add_i32 %4, %4, %7\n\t"
                "s_add_i32 %0, %0, %7\n\t"
                "s_cmp_lt_u32 %4, 64\n\t"
                "s_cbranch_scc0 Lfull%=\n"        // not full => the run is exhausted
                "Lnext%=:\n\t"
                "s_add_i32 %2, %2, 1\n\t"
                "s_cmp_ge_i32 %2, %9\n\t"
                "s_cbranch_scc1 Leos%=\n\t"
                "s_and_b32 %7, %2, %10\n\t"       // packet within the pass
                "s_cmp_eq_u32 %7, 0\n\t"
                "s_cbranch_scc1 Lreload%=\n\t"
                "v_readlane_b32 %8, %12, %7\n\t"  // its cut word
                "s_addk_i32 %3, 0x400\n\t"
                "s_and_b32 %7, %8, 0xffff\n\t"
                "s_lshr_b32 %8, %8, 16\n\t"
                "s_add_i32 %0, %3, %7\n\t"
                "s_add_i32 %1, %3, %8\n\t"
                "s_branch Ltop%=\n"
                "Lfull%=:\n\t"
                "s_mov_b32 %6, 0\n\t"
                "s_branch Ldone%=\n"
                "Lreload%=:\n\t"
                "s_mov_b32 %6, 1\n\t"
                "s_branch Ldone%=\n"
                "Leos%=:\n\t"
                "s_mov_b32 %6, 2\n"
                "Ldone%=:"
                : "+s"(cur), "+s"(end), "+s"(i), "+s"(pbase), "+s"(fill), "+v"(eo), "=&s"(status),
                  "=&s"(t0), "=&s"(t1)
                : "s"(n_my), "s"(gmask), "v"(lane), "v"(mycu)
                : "scc");
            if (status == 0) break;  // 64 lanes taken
            if (status == 2) {       // end of the stream
                if (fill > 0) eo = lane >= fill ? dummy_eo : eo;
                break;
            }
            // first packet of a pass: one coalesced load of the pass's cut words, waited for
            // HERE (a compiler-visible load still pending later would make its next wait a wait
            // for everything in flight)
            const int pp = __builtin_amdgcn_readfirstlane(p_first + (i >> lg_group) * stride);
            mycu = cutz[min(pp + lane, p_end - 1)];
            const uint32_t cu = __builtin_amdgcn_readfirstlane(mycu);
            pbase = pp << 10;
            cur = pbase + (int)(cu & 0xffffu);
            end = pbase + (int)(cu >> 16);
        }
        return fill;
    };
    // Issue the gathers of the filled batch: plain loads the compiler counts.  (Its waitcnt pass
    // then waits for ALL outstanding loads inside fill_batch -- the register allocator reuses
    // destination registers of the set in flight as temporaries there -- so the prefetch is
    // only partly effective.  Hiding the loads from the compiler in inline assembly fixes that
    // but leaves the in-flight registers unprotected against compiler copies; the hand-scheduled
    // stream below owns its registers instead.)
    typedef float v3f __attribute__((ext_vector_type(3)));
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    auto gather = [&](v3f& ev, v4u& va, uint32_t& vr) {
        const EvRec r = sxy[eo];
        ev.x = r.x;
        ev.y = r.y;
        ev.z = __uint_as_float(r.m);
        const uint32_t co = (eo >> 9) & ~1u;  // 2 * packet
        const uint4 c4 = coef4[co];
        va.x = c4.x;
        va.y = c4.y;
        va.z = c4.z;
        va.w = c4.w;
        vr = *reinterpret_cast<const uint32_t*>(coef4 + co + 1u);
    };
    auto arrived = [&](v3f&, v4u&, uint32_t&) {};
    const int nx8 = nx * 8;
    const int cbase = -row_base * nx8;
    auto vote = [&](const v3f& ev, const v4u& va, uint32_t vr) {
        const float ka = __uint_as_float(va.x), kbx = __uint_as_float(va.y);
        const float kby = __uint_as_float(va.z), kd = __uint_as_float(va.w);
        const float nxv = ev.x * ka + kbx;  // mapper_emvs_stereo.cpp:194-195
        const float nyv = ev.y * ka + kby;
        float X, Y;
        if (SLOW) {
            X = nxv / kd;
            Y = nyv / kd;
        } else {
            const float kr = __uint_as_float(vr);
            X = div_rc(nxv, kd, kr);
            Y = div_rc(nyv, kd, kr);
        }
        // cartesian3dgrid.h:255-259 restricted to this band's rows, as ONE integer test:
        // with xi = floor(X), yi = floor(Y) (the conversion saturates, NaN -> 0)
        //   0 <= X < nx-1  <=>  xi >= 0 and nx-2-xi >= 0        (X = -0.0 -> 0, accepted like >= 0.f)
        //   L <= Y < U     <=>  yi-Li >= 0 and Ui-1-yi >= 0     (L, U are integers)
        // all four hold iff the OR of the four values has a clear sign bit.  On the fast path X
        // and Y are finite by construction (k_plane_coef); on the slow path the only NaN source
        // is inf / inf, excluded by asking for finite numerators.
        const int xi = floor_to_int(X), yi = floor_to_int(Y);
        int sgn = xi | (nx - 2 - xi) | (yi - Li) | (Ui - 1 - yi);
        if (SLOW)
            sgn |= (fabsf(nxv) < __builtin_inff() && fabsf(nyv) < __builtin_inff()) ? 0 : -1;
        if (sgn >= 0) {
            // accepted => X, Y >= 0, where v_fract is exactly X - floor(X)
            const float fx = __builtin_amdgcn_fractf(X), fy = __builtin_amdgcn_fractf(Y);
            if (PAIRED) {  // lane mapping 8: two atomics on paired 32-bit cells
                vote_paired(band_bytes, xi, yi, row_bytes, -row_base * row_bytes, fx, fy, __float_as_uint(ev.z));
            } else {
                acc_t* cell = reinterpret_cast<acc_t*>(band_bytes + (__mul24(yi, nx8) + ((xi << 3) + cbase)));
                vote4(cell, 0, nx, fx, fy, __float_as_uint(ev.z));  // cartesian3dgrid.h:261-270
            }
        }
    };

    // two register sets: while the votes of one batch run, the gathers of the next are in flight
    // (the gathers are issued unconditionally -- an empty batch re-reads valid stale records --
    //  so that exactly three loads are newer than the ones a vote waits for)
    v3f eA, eB;
    v4u caA, caB;
    uint32_t crA, crB;
    int nA = fill_batch();
    gather(eA, caA, crA);
    while (nA > 0) {
        const int nB = fill_batch();
        gather(eB, caB, crB);
        arrived(eA, caA, crA);
        vote(eA, caA, crA);
        if (nB == 0) break;
        nA = fill_batch();
        gather(eA, caA, crA);
        arrived(eB, caB, crB);
        vote(eB, caB, crB);
    }
}

// ---- lane mapping 5: VECTOR fill.  The packed streams above append runs to the lanes with
// scalar bookkeeping (11 scalar instructions per run piece + 13 per packet, ~3 taken branches
// each); with short runs -- wide grids: ~19 records per (packet, band) at 1024 x 1024, 4.4 run
// pieces per batch -- a wave then spends ~80 dependent scalar instructions per batch and, with
// only 16 waves per CU (the band fills the LDS), nothing hides that latency (PMC at
// 1024x1024x256: scalar unit 67 % busy, LDS 37 %, 123 CU-clocks per batch).  Here the slot ->
// record mapping of a whole pass of up to 64 packets is computed with vector operations:
//   lane l = packet l of the pass: run length len_l, inclusive prefix incl_l (wave scan);
//   the non-empty packets are compacted (ballot + mbcnt + ds_permute) into tables
//   D_c = first record - first slot, P_c = packet index;
//   the LAST slot of every run sets one bit in a per-wave LDS bit array (ds_or_b64), read back
//   as one 64-bit word per batch (lane j = word j);
//   for batch b, slot lane i belongs to compacted packet  c = #tail bits before slot i
//   = (tails before the batch, a scalar) + v_mbcnt(word_b), and its record is D_c + slot.
// Per batch: 3 v_readlane, 2 v_mbcnt, 2 ds_bpermute, a few adds -- no loop over packets.
// The arithmetic of a vote is the function the other compiled streams use, so all mappings give
// the same bits.
template <bool SLOW>
__device__ __forceinline__ void vote_record(char* __restrict__ band_bytes, float ex, float ey,
                                            uint32_t em, uint4 va, uint32_t vr, int nx, int nx8,
                                            int cbase, int Li, int Ui)
{
    const float ka = __uint_as_float(va.x), kbx = __uint_as_float(va.y);
    const float kby = __uint_as_float(va.z), kd = __uint_as_float(va.w);
    const float nxv = ex * ka + kbx;  // mapper_emvs_stereo.cpp:194-195
    const float nyv = ey * ka + kby;
    float X, Y;
    if (SLOW) {
        X = nxv / kd;
        Y = nyv / kd;
    } else {
        const float kr = __uint_as_float(vr);
        X = div_rc(nxv, kd, kr);
        Y = div_rc(nyv, kd, kr);
    }
    // cartesian3dgrid.h:255-259 restricted to the band's rows, as one integer sign test (see
    // packed_stream)
    const int xi = floor_to_int(X), yi = floor_to_int(Y);
    int sgn = xi | (nx - 2 - xi) | (yi - Li) | (Ui - 1 - yi);
    if (SLOW)
        sgn |= (fabsf(nxv) < __builtin_inff() && fabsf(nyv) < __builtin_inff()) ? 0 : -1;
    if (sgn >= 0) {
        const float fx = __builtin_amdgcn_fractf(X), fy = __builtin_amdgcn_fractf(Y);
        acc_t* cell = reinterpret_cast<acc_t*>(band_bytes + (__mul24(yi, nx8) + ((xi << 3) + cbase)));
        vote4(cell, 0, nx, fx, fy, em);  // cartesian3dgrid.h:261-270
    }
}

// inclusive prefix sum over the 64 lanes with DPP moves only (no LDS round trips: the per-pass set-up
// of the vector fill sits on a wave's critical path while the LDS queue is full of votes)
__device__ __forceinline__ int wave_incl_scan(int v, int /*lane*/)
{
    // row_shr:n = 0x110 + n, row_bcast:15 = 0x142, row_bcast:31 = 0x143; lanes a mask disables
    // (and reads beyond a row) contribute `old` = 0
    int s = v;
    s += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, v, 0x113, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x114, 0xf, 0xe, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x118, 0xf, 0xc, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x142, 0xa, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x143, 0xc, 0xf, true);
    return s;
}

// BandPlan::cuts_inline: what a pass of the vector fill needs to find its packets' runs without a cut table.  Per item
// (band, plane): the band's Y interval; per packet two steps -- (1) the second half of its PlaneCoef {r, flags, d_a, by_a},
// (2) two entries of the transposed row table.  The streams issue (1) two stretches and (2) one stretch ahead of the votes.
struct InlineCuts {
    const uint16_t* rsT;  // nullptr: cut table
    uint32_t stride2;     // BYTES per row of rsT (the whole table is < 4 GB: vote_device)
    int nb;               // last entry of a packet's table: all its records
    int pad;
    float L, U;
};

__device__ __forceinline__ InlineCuts inline_cuts_of(const uint32_t* cuts, const Geom& g, const BandPlan& bp, int j)
{
    InlineCuts ic{};
    if (!bp.cuts_inline) return ic;
    ic.rsT = reinterpret_cast<const uint16_t*>(cuts);
    ic.stride2 = 2u * (uint32_t)bp.rs_stride;
    ic.pad = bp.row_pad;
    ic.nb = g.ny + 2 * bp.row_pad + 2;
    band_y_interval(j, g, bp, &ic.L, &ic.U);
    return ic;
}

// step 2 for the packet at byte column p2 (= 2 * packet; a valid packet of the plane): the byte offsets of its two table
// entries.  c1 = {r, flags | margin << 16, d_a, by_a}.  A vector instruction here is paid 1,500 times per wave and work
// item at configs[4]'s size, beside ~50 per batch of votes: the bins are band_row_bins' with the widening taken from the
// packet's own bound (PlaneCoef::flags >> 16, 1/256 rows: >= every band's), fused multiply-adds, one v_cvt_flr each and
// the clamps on integers -- a superset of that superset; the vote re-tests every event exactly.
__device__ __forceinline__ void inline_cut_entries(const InlineCuts& ic, uint4 c1, uint32_t p2, uint32_t* at_lo, uint32_t* at_hi)
{
    const float d_a = __uint_as_float(c1.z), by_a = __uint_as_float(c1.w);
    const float M = (float)(c1.y >> 16) * (1.f / 256.f);
    const float ya = __builtin_fmaf(ic.L, d_a, -by_a), yb = __builtin_fmaf(ic.U, d_a, -by_a);  // (finite: kCoefInvertible's range)
    const int lo = floor_to_int(fminf(ya, yb) - M) + (ic.pad + 1);  // events in bins below bin(floor(ymin))
    const int hi = floor_to_int(fmaxf(ya, yb) + M) + (ic.pad + 2);  // events in bins up to and including bin(floor(ymax))
    int bin_lo = min(max(lo, 0), ic.nb - 1), bin_hi = min(max(hi, 1), ic.nb);
    if (!(c1.y & kCoefInvertible)) {  // entry 0 is 0, entry nb the packet's records: the whole packet
        bin_lo = 0;
        bin_hi = ic.nb;
    }
    *at_lo = (uint32_t)bin_lo * ic.stride2 + p2;
    *at_hi = (uint32_t)bin_hi * ic.stride2 + p2;
}

__device__ __forceinline__ uint32_t inline_cut_load(const InlineCuts& ic, uint32_t byte_offset)
{
    return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(ic.rsT) + byte_offset);
}

// the cut word lo | hi << 16 of what the two loads returned (k_plane_coef's rules: a dead pair has no run, hi >= lo)
__device__ __forceinline__ uint32_t inline_cut_word(uint32_t flags, uint32_t lo, uint32_t hi)
{
    if (flags & kCoefSkip) return 0u;
    return lo | (max(hi, lo) << 16);
}

template <bool SLOW>
__device__ __forceinline__ void vfill_stream(const EvRec* __restrict__ sxy,
                                             const uint4* __restrict__ coef4,
                                             const uint32_t* __restrict__ cutz,
                                             char* __restrict__ band_bytes,
                                             unsigned long long* __restrict__ scratch /* 64 words of this wave */,
                                             int p_first, int p_end, int lg_pass, int stride,
                                             int lane, int nx, int Li, int Ui, int row_base,
                                             uint32_t dummy_eo, const InlineCuts& ic)
{
    if (Ui - 1 < Li) return;  // the band accepts no row
    const int pass = 1 << lg_pass;
    const int nx8 = nx * 8;
    const int cbase = -row_base * nx8;
    // ---- state of the batch generator (wave-uniform unless noted)
    int pass_base = p_first - stride;  // advanced before use
    int T = 0;                          // records of the current pass
    int rbase = 0;                      // first slot of the current range of 4096 slots
    int b = 0, nb = 0;                  // batch within the range, batches of the range
    int Cbase = 0;                      // compacted packets that end before the range
    int Dc = 0, Pc = 0;                 // per lane c: tables of the c-th non-empty packet
    int incl = 0, len = 0;              // per lane l: packet l of the pass
    unsigned long long w = 0;           // per lane j: tail bits of batch j of the range
    int cbefore = 0;                    // per lane j: tails of the range before batch j

    int rtot = 0;                       // tails of the current range
    auto build_range = [&]() {
        scratch[lane] = 0ull;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int ts = incl - 1 - rbase;  // tail slot of packet `lane`, relative to the range
        if (len > 0 && ts >= 0 && ts < 4096)
            atomicOr(&scratch[ts >> 6], 1ull << (ts & 63));
        // (same wave: its LDS operations complete in order; the fences only pin the compiler)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        w = scratch[lane];
        const int pc = __builtin_popcountll(w);
        const int inc = wave_incl_scan(pc, lane);
        cbefore = inc - pc;
        rtot = __builtin_amdgcn_readlane(inc, 63);
        nb = min(64, (T - rbase + 63) >> 6);
        b = 0;
    };
    // advance to the next batch; false at the end of the stream.  rec: record index per lane,
    // pk: packet whose coefficients the lane needs
    auto next_batch = [&](uint32_t& rec, int& pk) -> bool {
        while (b >= nb) {
            if (T > 0 && rbase + 4096 < T) {
                Cbase += rtot;
                rbase += 4096;
                build_range();
                continue;
            }
            pass_base += stride;
            if (pass_base >= p_end) return false;
            const int p = pass_base + lane;
            uint32_t cu = 0;
            if (lane < pass && p < p_end) {
                if (ic.rsT) {  // (this compiled stream is the A/B twin and the IEEE-divide planes' path: no prefetch)
                    const uint4 c1 = coef4[2 * (size_t)p + 1];
                    uint32_t at_lo, at_hi;
                    inline_cut_entries(ic, c1, 2u * (uint32_t)p, &at_lo, &at_hi);
                    cu = inline_cut_word(c1.y, inline_cut_load(ic, at_lo), inline_cut_load(ic, at_hi));
                } else {
                    cu = cutz[p];
                }
            }
            const int lo = (int)(cu & 0xffffu), hi = (int)(cu >> 16);
            len = max(hi - lo, 0);
            incl = wave_incl_scan(len, lane);
            T = __builtin_amdgcn_readlane(incl, 63);
            rbase = 0;
            Cbase = 0;
            b = nb = 0;
            if (T == 0) continue;
            const int D = (p << 10) + lo - (incl - len);
            const unsigned long long ne = __builtin_amdgcn_ballot_w64(len > 0);
            const int c = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ne >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)ne, 0u));
            // push (D, p) of the non-empty packets to lanes 0, 1, 2, ...; empty ones to an unused lane
            const int dst = len > 0 ? c : 63 - (lane - c);
            Dc = __builtin_amdgcn_ds_permute(dst << 2, D);
            Pc = __builtin_amdgcn_ds_permute(dst << 2, p);
            build_range();
        }
        const uint32_t wlo = (uint32_t)__builtin_amdgcn_readlane((int)w, b);
        const uint32_t whi = (uint32_t)__builtin_amdgcn_readlane((int)(w >> 32), b);
        const int cb = __builtin_amdgcn_readlane(cbefore, b) + Cbase;
        const int c = cb + (int)__builtin_amdgcn_mbcnt_hi(whi, __builtin_amdgcn_mbcnt_lo(wlo, 0u));
        const int slot = rbase + (b << 6) + lane;
        const int Dl = __builtin_amdgcn_ds_bpermute(c << 2, Dc);
        const int Pl = __builtin_amdgcn_ds_bpermute(c << 2, Pc);
        const bool live = slot < T;
        rec = live ? (uint32_t)(Dl + slot) : dummy_eo;
        pk = live ? Pl : p_first;
        ++b;
        return true;
    };
    struct Loaded {
        EvRec e;
        uint4 va;
        uint32_t vr;
    };
    auto gather = [&](uint32_t rec, int pk, Loaded& L) {
        L.e = sxy[rec];
        L.va = coef4[2 * (size_t)pk];
        L.vr = *reinterpret_cast<const uint32_t*>(coef4 + 2 * (size_t)pk + 1);
    };
    auto vote = [&](const Loaded& L) {
        vote_record<SLOW>(band_bytes, L.e.x, L.e.y, L.e.m, L.va, L.vr, nx, nx8, cbase, Li, Ui);
    };
    uint32_t rec;
    int pk;
    Loaded A, B;
    if (!next_batch(rec, pk)) return;
    gather(rec, pk, A);
    for (;;) {
        const bool haveB = next_batch(rec, pk);
        if (haveB) gather(rec, pk, B);
        vote(A);
        if (!haveB) break;
        const bool haveA = next_batch(rec, pk);
        if (haveA) gather(rec, pk, A);
        vote(B);
        if (!haveA) break;
    }
}

// The same stream, fast path only (no IEEE-divide planes), written in gfx950 assembly.
//
// Why: PMC counters of the compiled stream (10 M events x 100 planes) show ~61 scalar and ~63
// vector instructions per 64-lane batch at ~78 CU-clocks per batch: the scalar unit (one
// instruction per clock per CU, shared by all its waves) is ~80 % busy, mostly with compiler
// glue around the run bookkeeping, and the prefetch registers get shuffled.  Written by hand
// the batch costs ~34 scalar + ~46 vector instructions + 4 ds_add_u64, which leaves the LDS
// atomic unit (~11 clocks per ds_add_u64 wave instruction) as the next bound.
//
// Register map (all listed as clobbers; the operands are read-only):
//   s40 cur  s41 end  s42 packet counter i  s43 packet*1024  s44 fill  s45,s46 temporaries
//   s47 lanes of the batch in set A, s48 of set B
//   v40 record index per lane (eo)   v41 cut words of the pass
//   set A: v[42:44] record (x0,y0,m)  v45 r  v[46:49] a,bx,by,d      set B: v[50:52] v53 v[54:57]
//   (register tuples must be even-aligned on gfx950)
//   v36-v39, v58-v63 temporaries
// The arithmetic of VOTE is instruction for instruction what packed_stream<false> compiles to
// (mapper_emvs_stereo.cpp:194-195, div_rc, cartesian3dgrid.h:255-270), so both give the same bits.
#define DSI_ASM_FILL(NOUT, L)                                                                      \
    "s_mov_b32 s44, 0\n"                                                                            \
    "Ltop" L "%=:\n\t"                                                                              \
    "s_cmp_ge_i32 s40, s41\n\t"                                                                     \
    "s_cbranch_scc1 Lnext" L "%=\n\t"                                                               \
    "s_sub_i32 s45, 64, s44\n\t"          /* room in the batch */                                   \
    "s_sub_i32 s46, s41, s40\n\t"         /* records left in the run */                             \
    "s_min_i32 s45, s45, s46\n\t"         /* take */                                                \
    "s_sub_i32 s46, s40, s44\n\t"         /* record of lane 0 if the run started there */           \
    "s_lshl_b64 exec, -1, s44\n\t"        /* lanes >= fill */                                       \
    "v_add_u32 v40, s46, %15\n\t"                                                                   \
    "s_mov_b64 exec, -1\n\t"                                                                        \
    "s_add_i32 s44, s44, s45\n\t"                                                                   \
    "s_add_i32 s40, s40, s45\n\t"                                                                   \
    "s_cmp_lt_u32 s44, 64\n\t"                                                                      \
    "s_cbranch_scc0 Ldone" L "%=\n"       /* not full => the run is exhausted */                    \
    "Lnext" L "%=:\n\t"                                                                             \
    "s_add_i32 s42, s42, 1\n\t"                                                                     \
    "s_cmp_ge_i32 s42, %3\n\t"                                                                      \
    "s_cbranch_scc1 Leos" L "%=\n\t"                                                                \
    "s_and_b32 s45, s42, %4\n\t"          /* packet within the pass */                              \
    "s_cmp_eq_u32 s45, 0\n\t"                                                                       \
    "s_cbranch_scc1 Lreload" L "%=\n\t"                                                             \
    "v_readlane_b32 s46, v41, s45\n\t"    /* its cut word */                                        \
    "s_addk_i32 s43, 0x400\n"                                                                       \
    "Lhave" L "%=:\n\t"                                                                             \
    "s_and_b32 s45, s46, 0xffff\n\t"                                                                \
    "s_lshr_b32 s46, s46, 16\n\t"                                                                   \
    "s_add_i32 s40, s43, s45\n\t"                                                                   \
    "s_add_i32 s41, s43, s46\n\t"                                                                   \
    "s_branch Ltop" L "%=\n"                                                                        \
    "Lreload" L "%=:\n\t"                 /* first packet of a pass: its cut words were prefetched */ \
    "s_lshr_b32 s45, s42, %7\n\t"         /* into v35 one pass ago (loads return in order: once a    */ \
    "s_mul_i32 s45, s45, %6\n\t"          /* GATHER has been issued since, all but the 3 newest      */ \
    "s_add_i32 s45, s45, %5\n\t"          /* loads include them; first packet of the pass:)          */ \
    "s_lshl_b32 s43, s45, 10\n\t"                                                                   \
    "s_cmp_eq_u32 s50, 0\n\t"                                                                       \
    "s_cbranch_scc1 Lwall" L "%=\n\t"                                                               \
    "s_waitcnt vmcnt(3)\n\t"                                                                        \
    "s_branch Lgot" L "%=\n"                                                                        \
    "Lwall" L "%=:\n\t"                                                                             \
    "s_waitcnt vmcnt(0)\n"                                                                          \
    "Lgot" L "%=:\n\t"                                                                              \
    "v_mov_b32 v41, v35\n\t"                                                                        \
    "s_add_i32 s45, s45, %6\n\t"          /* the next pass's cut words travel during this pass */   \
    "v_add_u32 v58, s45, %15\n\t"                                                                   \
    "v_min_i32 v58, %8, v58\n\t"                                                                    \
    "v_lshlrev_b32 v58, 2, v58\n\t"                                                                 \
    "global_load_dword v35, v58, %2\n\t"                                                            \
    "s_mov_b32 s50, 0\n\t"                                                                          \
    "v_readfirstlane_b32 s46, v41\n\t"                                                              \
    "s_branch Lhave" L "%=\n"                                                                       \
    "Leos" L "%=:\n\t"                    /* stream over: unreached lanes -> multiplicity-0 record */ \
    "s_cmp_eq_u32 s44, 0\n\t"                                                                       \
    "s_cbranch_scc1 Ldone" L "%=\n\t"                                                               \
    "s_lshl_b64 exec, -1, s44\n\t"                                                                  \
    "v_mov_b32 v40, %14\n\t"                                                                        \
    "s_mov_b64 exec, -1\n"                                                                          \
    "Ldone" L "%=:\n\t"                                                                             \
    "s_mov_b32 " NOUT ", s44\n\t"

// DSI_ASM_GATHER, DSI_ASM_VOTE: dsi_vote_asm.h

__device__ __forceinline__ void packed_stream_asm(const EvRec* sxy, const uint4* coef4,
                                                  const uint32_t* cutz, char* band_bytes,
                                                  int p_first, int p_end, int lg_group, int stride,
                                                  int lane, int nx, int Li, int Ui, int row_base,
                                                  uint32_t dummy_eo)
{
    const int group = 1 << lg_group;
    int n_my = 0;
    if (p_first < p_end) {
        const int passes = (p_end - p_first + stride - 1) / stride;
        const int last = p_first + (passes - 1) * stride;
        n_my = (passes - 1) * group + min(group, p_end - last);
    }
    if (Ui - 1 < Li) n_my = 0;  // no acceptable row (the unsigned range test needs Ui-1-Li >= 0)
    // every operand is wave-uniform; the readfirstlanes pin them to scalar registers
    const int s_n_my = __builtin_amdgcn_readfirstlane(n_my);
    const int s_gmask = __builtin_amdgcn_readfirstlane(group - 1);
    const int s_p_first = __builtin_amdgcn_readfirstlane(p_first);
    const int s_stride = __builtin_amdgcn_readfirstlane(stride);
    const int s_lg = __builtin_amdgcn_readfirstlane(lg_group);
    const int s_p_last = __builtin_amdgcn_readfirstlane(p_end - 1);
    const int s_nx8 = __builtin_amdgcn_readfirstlane(nx * 8);
    const int lds_base = (int)(uintptr_t)band_bytes;  // LDS byte offset of the band
    const int s_cbase = __builtin_amdgcn_readfirstlane(lds_base - row_base * nx * 8);
    const int s_nxm2 = __builtin_amdgcn_readfirstlane(nx - 2);
    const int s_Li = __builtin_amdgcn_readfirstlane(Li);
    // rows the band accepts: 0 <= yi - Li <= Ui - 1 - Li  (a band with no acceptable row gets no stream)
    const int s_Uim1 = __builtin_amdgcn_readfirstlane(Ui - 1 - Li);
    const uint32_t s_dummy = __builtin_amdgcn_readfirstlane(dummy_eo);
    asm volatile(
        "s_mov_b32 s42, -1\n\t"
        "s_mov_b32 s40, 0\n\t"
        "s_mov_b32 s41, 0\n\t"
        "s_mov_b32 s43, 0\n\t"
        "v_mov_b32 v40, 0\n\t"
        "v_mov_b32 v41, 0\n\t"
        "s_mov_b32 s50, 0\n\t"
        "v_add_u32 v58, %5, %15\n\t"        // the first pass's cut words
        "v_min_i32 v58, %8, v58\n\t"
        "v_max_i32 v58, 0, v58\n\t"          // (a chunk without packets has p_end - 1 = -1)
        "v_lshlrev_b32 v58, 2, v58\n\t"
        "global_load_dword v35, v58, %2\n\t"
        DSI_ASM_FILL("s47", "a")
        DSI_ASM_GATHER("v[42:44]", "v[46:49]", "v45")
        "s_cmp_eq_u32 s47, 0\n\t"
        "s_cbranch_scc1 Lend%=\n"
        "Lloop%=:\n\t"
        DSI_ASM_FILL("s48", "b")
        DSI_ASM_GATHER("v[50:52]", "v[54:57]", "v53")
        "s_waitcnt vmcnt(3)\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "s_cmp_eq_u32 s48, 0\n\t"
        "s_cbranch_scc1 Lend%=\n\t"
        DSI_ASM_FILL("s47", "c")
        DSI_ASM_GATHER("v[42:44]", "v[46:49]", "v45")
        "s_waitcnt vmcnt(3)\n\t"
        DSI_ASM_VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")
        "s_cmp_lg_u32 s47, 0\n\t"
        "s_cbranch_scc1 Lloop%=\n"
        "Lend%=:\n\t"
        "s_waitcnt vmcnt(0) lgkmcnt(0)"
        :
        : "s"(sxy), "s"(coef4), "s"(cutz), "s"(s_n_my), "s"(s_gmask), "s"(s_p_first), "s"(s_stride),
          "s"(s_lg), "s"(s_p_last), "s"(s_nx8), "s"(s_cbase), "s"(s_nxm2), "s"(s_Li), "s"(s_Uim1),
          "s"(s_dummy), "v"(lane)
        : "memory", "scc", "vcc", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s50",
          "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48",
          "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61",
          "v62", "v63");
}

// ---- the packed stream with DEALT passes (the fused kernel: one workgroup per CU, nothing else hides a
// workgroup's tail).  With fixed assignments (wave w takes passes w, w + 16, ...) the waves of a workgroup
// finish a work item at very different times -- 512 x 512 x 200, 489 packets in passes of 8: 61 passes over
// 16 waves is 3 or 4 each, and waves with EQUAL work still spread by 20 % (time stamps of
// tools/fused_trace.py: first wave done after 11.3 us, median 13.7, last 16.8) -- and everybody waits at the
// item's barrier.  Here wave w starts with passes w and w + 16 and draws every further pass from a counter in
// LDS (set to 32 by the item's set-up): ds_add_rtn_u32 by one lane, two passes ahead, so that neither the
// atomic's round trip through the vote-filled LDS queue nor the next pass's cut words are ever waited for:
//   at the start of pass k:  its cut words (requested at pass k-1) arrive; the index of pass k+1 (drawn at
//   pass k-1) is read; pass k+1's cut words are requested; pass k+2 is drawn.
// The sums are integer, so which wave votes a pass changes no bit.
//   s53 current pass, s55 next pass, s54 packets of the current pass, s42 packet within the pass,
//   v34 the drawn pass index (lane 0); everything else as in packed_stream_asm.
#define DSI_ASM_FILL_DEAL(NOUT, L)                                                                 \
    "s_mov_b32 s44, 0\n"                                                                            \
    "Ltop" L "%=:\n\t"                                                                              \
    "s_cmp_ge_i32 s40, s41\n\t"                                                                     \
    "s_cbranch_scc1 Lnext" L "%=\n\t"                                                               \
    "s_sub_i32 s45, 64, s44\n\t"          /* room in the batch */                                   \
    "s_sub_i32 s46, s41, s40\n\t"         /* records left in the run */                             \
    "s_min_i32 s45, s45, s46\n\t"         /* take */                                                \
    "s_sub_i32 s46, s40, s44\n\t"         /* record of lane 0 if the run started there */           \
    "s_lshl_b64 exec, -1, s44\n\t"        /* lanes >= fill */                                       \
    "v_add_u32 v40, s46, %15\n\t"                                                                   \
    "s_mov_b64 exec, -1\n\t"                                                                        \
    "s_add_i32 s44, s44, s45\n\t"                                                                   \
    "s_add_i32 s40, s40, s45\n\t"                                                                   \
    "s_cmp_lt_u32 s44, 64\n\t"                                                                      \
    "s_cbranch_scc0 Ldone" L "%=\n"       /* not full => the run is exhausted */                    \
    "Lnext" L "%=:\n\t"                                                                             \
    "s_add_i32 s42, s42, 1\n\t"                                                                     \
    "s_cmp_ge_i32 s42, s54\n\t"                                                                     \
    "s_cbranch_scc1 Lreload" L "%=\n\t"   /* the pass is exhausted */                               \
    "v_readlane_b32 s46, v41, s42\n\t"    /* the packet's cut word */                               \
    "s_addk_i32 s43, 0x400\n"                                                                       \
    "Lhave" L "%=:\n\t"                                                                             \
    "s_and_b32 s45, s46, 0xffff\n\t"                                                                \
    "s_lshr_b32 s46, s46, 16\n\t"                                                                   \
    "s_add_i32 s40, s43, s45\n\t"                                                                   \
    "s_add_i32 s41, s43, s46\n\t"                                                                   \
    "s_branch Ltop" L "%=\n"                                                                        \
    "Lreload" L "%=:\n\t"                                                                           \
    "s_mov_b32 s53, s55\n\t"              /* the pass whose cut words are in flight */              \
    "s_cmp_ge_i32 s53, %3\n\t"                                                                      \
    "s_cbranch_scc1 Leos" L "%=\n\t"                                                                \
    "s_lshl_b32 s45, s53, %7\n\t"                                                                   \
    "s_add_i32 s45, s45, %5\n\t"          /* its first packet */                                    \
    "s_sub_i32 s54, %6, s45\n\t"                                                                    \
    "s_min_i32 s54, s54, %4\n\t"          /* its packets (the last pass may be short) */            \
    "s_lshl_b32 s43, s45, 10\n\t"                                                                   \
    "s_cmp_eq_u32 s50, 0\n\t"                                                                       \
    "s_cbranch_scc1 Lwall" L "%=\n\t"                                                               \
    "s_waitcnt vmcnt(3)\n\t"              /* (a GATHER has been issued since: all but the 3 newest) */ \
    "s_branch Lgot" L "%=\n"                                                                        \
    "Lwall" L "%=:\n\t"                                                                             \
    "s_waitcnt vmcnt(0)\n"                                                                          \
    "Lgot" L "%=:\n\t"                                                                              \
    "v_mov_b32 v41, v35\n\t"                                                                        \
    "s_waitcnt lgkmcnt(0)\n\t"            /* the draw of one pass ago */                            \
    "v_readfirstlane_b32 s55, v34\n\t"                                                              \
    "s_lshl_b32 s45, s55, %7\n\t"                                                                   \
    "s_add_i32 s45, s45, %5\n\t"                                                                    \
    "v_add_u32 v58, s45, %15\n\t"         /* the next pass's cut words travel during this pass */   \
    "v_min_i32 v58, %8, v58\n\t"                                                                    \
    "v_lshlrev_b32 v58, 2, v58\n\t"                                                                 \
    "global_load_dword v35, v58, %2\n\t"                                                            \
    "s_mov_b32 s50, 0\n\t"                                                                          \
    "s_mov_b64 exec, 1\n\t"                                                                         \
    "ds_add_rtn_u32 v34, %16, %17\n\t"    /* draw the pass after the next */                        \
    "s_mov_b64 exec, -1\n\t"                                                                        \
    "s_mov_b32 s42, 0\n\t"                                                                          \
    "v_readfirstlane_b32 s46, v41\n\t"                                                              \
    "s_branch Lhave" L "%=\n"                                                                       \
    "Leos" L "%=:\n\t"                    /* stream over: unreached lanes -> multiplicity-0 record */ \
    "s_mov_b32 s40, 0\n\t"                                                                          \
    "s_mov_b32 s41, 0\n\t"                                                                          \
    "s_mov_b32 s42, 0\n\t"                                                                          \
    "s_mov_b32 s54, 0\n\t"                /* (a later fill comes straight back here) */             \
    "s_cmp_eq_u32 s44, 0\n\t"                                                                       \
    "s_cbranch_scc1 Ldone" L "%=\n\t"                                                               \
    "s_lshl_b64 exec, -1, s44\n\t"                                                                  \
    "v_mov_b32 v40, %14\n\t"                                                                        \
    "s_mov_b64 exec, -1\n"                                                                          \
    "Ldone" L "%=:\n\t"                                                                             \
    "s_mov_b32 " NOUT ", s44\n\t"

// passes of `1 << lg_group` packets of [p_begin, p_end); wave `wave` of `n_waves`; pass_counter: LDS word set
// to 2 * n_waves before the workgroup's waves enter
// (the whole stream as one asm statement; VOTE = DSI_ASM_VOTE or, lane mapping 8, DSI_ASM_VOTE_PAIRED19)
#define DSI_DEALT_STREAM_ASM(VOTE)                                                                                      \
    asm volatile(                                                                                                       \
        "s_mov_b32 s42, 0\n\t"                                                                                          \
        "s_mov_b32 s54, 0\n\t"                                                                                          \
        "s_mov_b32 s40, 0\n\t"                                                                                          \
        "s_mov_b32 s41, 0\n\t"                                                                                          \
        "s_mov_b32 s43, 0\n\t"                                                                                          \
        "s_mov_b32 s55, %18\n\t"             /* the first pass: the wave's index ... */                                 \
        "v_mov_b32 v34, %19\n\t"             /* ... the second: n_waves further */                                      \
        "v_mov_b32 v40, 0\n\t"                                                                                          \
        "v_mov_b32 v41, 0\n\t"                                                                                          \
        "s_mov_b32 s50, 0\n\t"                                                                                          \
        "v_mov_b32 v35, %20\n\t"             /* the first pass's cut words (already here) */                            \
        DSI_ASM_FILL_DEAL("s47", "a")                                                                                   \
        DSI_ASM_GATHER("v[42:44]", "v[46:49]", "v45")                                                                   \
        "s_cmp_eq_u32 s47, 0\n\t"                                                                                       \
        "s_cbranch_scc1 Lend%=\n"                                                                                       \
        "Lloop%=:\n\t"                                                                                                  \
        DSI_ASM_FILL_DEAL("s48", "b")                                                                                   \
        DSI_ASM_GATHER("v[50:52]", "v[54:57]", "v53")                                                                   \
        "s_waitcnt vmcnt(3)\n\t"                                                                                        \
        VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")                                                    \
        "s_cmp_eq_u32 s48, 0\n\t"                                                                                       \
        "s_cbranch_scc1 Lend%=\n\t"                                                                                     \
        DSI_ASM_FILL_DEAL("s47", "c")                                                                                   \
        DSI_ASM_GATHER("v[42:44]", "v[46:49]", "v45")                                                                   \
        "s_waitcnt vmcnt(3)\n\t"                                                                                        \
        VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")                                                    \
        "s_cmp_lg_u32 s47, 0\n\t"                                                                                       \
        "s_cbranch_scc1 Lloop%=\n"                                                                                      \
        "Lend%=:\n\t"                                                                                                   \
        "s_waitcnt vmcnt(0) lgkmcnt(0)"                                                                                 \
        :                                                                                                               \
        : "s"(sxy), "s"(coef4), "s"(cutz), "s"(s_npass), "s"(s_group), "s"(s_p_begin), "s"(s_p_end),                    \
          "s"(s_lg), "s"(s_p_last), "s"(s_nx8), "s"(s_cbase), "s"(s_nxm2), "s"(s_Li), "s"(s_Uim1),                      \
          "s"(s_dummy), "v"(lane), "v"(ctr_addr), "v"(1), "s"(s_first), "v"(wave + n_waves), "v"(first_cuts), "s"(s_halfb) \
        : "memory", "scc", "vcc", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s50", "s53", "s54", "s55", \
          "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48",     \
          "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61",                   \
          "v62", "v63")

// PAIRED (lane mapping 8): the band's rows are rows of paired 32-bit cells (dsi_vote_asm.h), row_bytes = 16 * rw apart
template <bool PAIRED = false>
__device__ __forceinline__ void packed_stream_asm_dealt(const EvRec* sxy, const uint4* coef4,
                                                        const uint32_t* cutz, char* band_bytes,
                                                        int p_begin, int p_end, int lg_group, int wave, int n_waves,
                                                        int lane, int nx, int Li, int Ui, int row_base,
                                                        uint32_t dummy_eo, int* pass_counter, uint32_t first_cuts,
                                                        int row_bytes = 0)
{
    // first_cuts: the cut words of the wave's first pass, lane l = packet p_begin + wave * group + l (clamped to
    // p_end - 1), loaded by the caller -- in the fused kernel BEFORE the previous phase's barrier and read-back,
    // which hide the round trip that would otherwise open every phase
    const int group = 1 << lg_group;
    int npass = (p_end - p_begin + group - 1) >> lg_group;
    if (Ui - 1 < Li) npass = 0;  // no acceptable row (the unsigned range test needs Ui-1-Li >= 0)
    if (!PAIRED) row_bytes = nx * 8;
    const int s_npass = __builtin_amdgcn_readfirstlane(npass);
    const int s_group = __builtin_amdgcn_readfirstlane(group);
    const int s_p_begin = __builtin_amdgcn_readfirstlane(p_begin);
    const int s_p_end = __builtin_amdgcn_readfirstlane(p_end);
    const int s_lg = __builtin_amdgcn_readfirstlane(lg_group);
    const int s_p_last = __builtin_amdgcn_readfirstlane(p_end - 1);
    const int s_nx8 = __builtin_amdgcn_readfirstlane(row_bytes);
    const int lds_base = (int)(uintptr_t)band_bytes;  // LDS byte offset of the band
    const int s_cbase = __builtin_amdgcn_readfirstlane(lds_base - row_base * row_bytes);
    const int s_nxm2 = __builtin_amdgcn_readfirstlane(nx - 2);
    const int s_Li = __builtin_amdgcn_readfirstlane(Li);
    const int s_Uim1 = __builtin_amdgcn_readfirstlane(Ui - 1 - Li);
    const uint32_t s_dummy = __builtin_amdgcn_readfirstlane(dummy_eo);
    const int ctr_addr = (int)(uintptr_t)pass_counter;
    const int s_first = __builtin_amdgcn_readfirstlane(wave);
    const int s_halfb = __builtin_amdgcn_readfirstlane(row_bytes >> 1);  // (PAIRED: byte offset of a row's V words)
    if constexpr (PAIRED)
        DSI_DEALT_STREAM_ASM(DSI_ASM_VOTE_PAIRED19);
    else
        DSI_DEALT_STREAM_ASM(DSI_ASM_VOTE);
}

// ---- lane mapping 5, hand-scheduled: the batches of one range (<= 64 batches = 4096 slots) of a
// vector-fill pass (see vfill_stream for the slot -> record mapping; the per-pass tables are built
// by compiled code and handed over through the wave's LDS scratch).  Per batch: 3 v_readlane +
// 2 v_mbcnt + 1 ds_read_b64 of the run table find every lane's record and packet (two ds_bpermute of
// register tables at first: one LDS instruction fewer per batch was worth 7 % at 1024 x 1024 x 256,
// 4.96 -> 4.60 ms), then the same GATHER / VOTE as the packed
// stream.  Two batches of gathers are in flight while one is voted: the table look-up of batch k+2
// is issued BEFORE the votes of batch k (its latency hides behind ~45 vector instructions),
// waited for with lgkmcnt(4) (the four ds_add_u64 of batch k are younger), and the gathers of
// batch k+2 go into the register set batch k has just released.
//   s42 batch counter k   s45 k+2   s46,s49,s50 tail-bit words / tails before the batch   s51 first slot of batch k+2
//   v32 slot per lane   v34 12 * (record - slot)   v35 table address, then the coefficient byte offset
//   sets A / B and the temporaries as in packed_stream_asm
#define DSI_ASM_VPREP1                                                                             \
    "v_readlane_b32 s46, %5, s45\n\t"     /* tail bits of the batch, low / high half */             \
    "v_readlane_b32 s49, %6, s45\n\t"                                                               \
    "v_readlane_b32 s50, %7, s45\n\t"     /* runs that end before the batch */                      \
    "v_mbcnt_lo_u32_b32 v35, s46, 0\n\t"                                                            \
    "v_mbcnt_hi_u32_b32 v35, s49, v35\n\t" /* + runs that end before this lane's slot */            \
    "v_add_u32 v35, v35, s50\n\t"                                                                   \
    "v_lshl_add_u32 v35, v35, 3, %8\n\t"                                                            \
    "ds_read_b64 v[34:35], v35\n\t"       /* the run's {D, coefficient byte offset} */              \
    "s_lshl_b32 s51, s45, 6\n\t"                                                                    \
    "s_add_i32 s51, s51, %3\n\t"          /* first slot of the batch */

#define DSI_ASM_VPREP2(EV, CA, CR)                                                                 \
    "v_add_u32 v32, s51, %15\n\t"         /* slot */                                                \
    "s_mul_i32 s46, s51, 12\n\t"                                                                    \
    "v_cmp_gt_i32 vcc, %4, v32\n\t"       /* slot < T */                                            \
    "v_add3_u32 v58, v34, s46, %17\n\t"   /* byte offset of the record: 12 * (D + slot) */          \
    "v_cndmask_b32 v58, %14, v58, vcc\n\t" /* beyond the pass: the multiplicity-0 record */         \
    "global_load_dwordx3 " EV ", v58, %0\n\t"                                                       \
    "global_load_dwordx4 " CA ", v35, %1\n\t"                                                       \
    "global_load_dword " CR ", v35, %1 offset:16\n\t"

__device__ __forceinline__ void vfill_range_asm(const EvRec* sxy, const uint4* coef4, int nb, int slot0,
                                                int T, uint32_t wlo, uint32_t whi, int cb, const void* tab,
                                                char* band_bytes, int lane, int nx, int Li,
                                                int Ui, int row_base, uint32_t dummy_eo)
{
    const int s_tab = __builtin_amdgcn_readfirstlane((int)(uintptr_t)tab);  // LDS address of the run table
    const int s_nb = __builtin_amdgcn_readfirstlane(nb);
    const int s_slot0 = __builtin_amdgcn_readfirstlane(slot0);
    const int s_T = __builtin_amdgcn_readfirstlane(T);
    const int s_nx8 = __builtin_amdgcn_readfirstlane(nx * 8);
    const int lds_base = (int)(uintptr_t)band_bytes;
    const int s_cbase = __builtin_amdgcn_readfirstlane(lds_base - row_base * nx * 8);
    const int s_nxm2 = __builtin_amdgcn_readfirstlane(nx - 2);
    const int s_Li = __builtin_amdgcn_readfirstlane(Li);
    const int s_Uim1 = __builtin_amdgcn_readfirstlane(Ui - 1 - Li);
    asm volatile(
        // prologue: batches 0 and 1 (batch 1 may lie beyond the range: all its lanes then take the
        // multiplicity-0 record only if it is also beyond the pass; it is never voted)
        "s_mov_b32 s42, 0\n\t"
        "s_mov_b32 s45, 0\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt lgkmcnt(0)\n\t"
        DSI_ASM_VPREP2("v[42:44]", "v[46:49]", "v45")
        "s_cmp_lt_i32 1, %2\n\t"
        "s_cbranch_scc0 Llast1%=\n\t"        // nb == 1
        "s_mov_b32 s45, 1\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt lgkmcnt(0)\n\t"
        DSI_ASM_VPREP2("v[50:52]", "v[54:57]", "v53")
        "Lloop%=:\n\t"
        // ---- batch k in set A
        "s_add_i32 s45, s42, 2\n\t"
        "s_cmp_lt_i32 s45, %2\n\t"
        "s_cbranch_scc0 LtailA%=\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt vmcnt(3)\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "s_waitcnt lgkmcnt(4)\n\t"
        DSI_ASM_VPREP2("v[42:44]", "v[46:49]", "v45")
        "s_add_i32 s42, s42, 1\n\t"
        // ---- batch k+1 in set B
        "s_add_i32 s45, s42, 2\n\t"
        "s_cmp_lt_i32 s45, %2\n\t"
        "s_cbranch_scc0 LtailB%=\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt vmcnt(3)\n\t"
        DSI_ASM_VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")
        "s_waitcnt lgkmcnt(4)\n\t"
        DSI_ASM_VPREP2("v[50:52]", "v[54:57]", "v53")
        "s_add_i32 s42, s42, 1\n\t"
        "s_branch Lloop%=\n"
        "LtailA%=:\n\t"                      // batches k (A) and k+1 (B) remain, both in flight
        "s_waitcnt vmcnt(3)\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "s_waitcnt vmcnt(0)\n\t"
        DSI_ASM_VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")
        "s_branch Lend%=\n"
        "LtailB%=:\n\t"                      // batches k (B) and k+1 (A) remain
        "s_waitcnt vmcnt(3)\n\t"
        DSI_ASM_VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")
        "s_waitcnt vmcnt(0)\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "s_branch Lend%=\n"
        "Llast1%=:\n\t"                      // a single batch
        "s_waitcnt vmcnt(0)\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "Lend%=:\n\t"
        "s_waitcnt vmcnt(0) lgkmcnt(0)"
        :
        : "s"(sxy), "s"(coef4), "s"(s_nb), "s"(s_slot0), "s"(s_T), "v"(wlo), "v"(whi), "v"(cb), "s"(s_tab),
          "s"(s_nx8), "s"(s_cbase), "s"(s_nxm2), "s"(s_Li), "s"(s_Uim1), "v"(dummy_eo * 12u), "v"(lane),
          "v"(0), "v"(lane * 12)
        : "memory", "scc", "vcc", "s42", "s45", "s46", "s49", "s50", "s51", "v32", "v33", "v34", "v35",
          "v36", "v37", "v38", "v39", "v40", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50",
          "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63");
}

// The same range with THREE register sets (k_vote_bands_vfill: one workgroup per CU, 128 VGPRs): the
// gathers of batch k+3 are issued while batch k is voted, i.e. two whole iterations of other work
// cover a gather's round trip instead of one -- with 16 waves per CU a wave's iteration is ~1300
// clocks and the loaded L2 / fabric takes about that long.  Set C = v[24:26] record, v27 r,
// v[28:31] a,bx,by,d.  The closing votes wait for everything in flight at once (vmcnt(0)) and then
// run in any order, so one drain serves all three phases: s52 = bit mask of the sets still to vote.
__device__ __forceinline__ void vfill_range_asm3(const EvRec* sxy, const uint4* coef4, int nb, int slot0,
                                                 int T, uint32_t wlo, uint32_t whi, int cb, const void* tab,
                                                 char* band_bytes, int lane, int nx, int Li,
                                                 int Ui, int row_base, uint32_t dummy_eo)
{
    const int s_tab = __builtin_amdgcn_readfirstlane((int)(uintptr_t)tab);  // LDS address of the run table
    const int s_nb = __builtin_amdgcn_readfirstlane(nb);
    const int s_slot0 = __builtin_amdgcn_readfirstlane(slot0);
    const int s_T = __builtin_amdgcn_readfirstlane(T);
    const int s_nx8 = __builtin_amdgcn_readfirstlane(nx * 8);
    const int lds_base = (int)(uintptr_t)band_bytes;
    const int s_cbase = __builtin_amdgcn_readfirstlane(lds_base - row_base * nx * 8);
    const int s_nxm2 = __builtin_amdgcn_readfirstlane(nx - 2);
    const int s_Li = __builtin_amdgcn_readfirstlane(Li);
    const int s_Uim1 = __builtin_amdgcn_readfirstlane(Ui - 1 - Li);
    asm volatile(
        // prologue: up to three batches in flight
        "s_mov_b32 s42, 0\n\t"
        "s_mov_b32 s45, 0\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt lgkmcnt(0)\n\t"
        DSI_ASM_VPREP2("v[42:44]", "v[46:49]", "v45")
        "s_mov_b32 s52, 1\n\t"
        "s_cmp_lt_i32 1, %2\n\t"
        "s_cbranch_scc0 Ldrain%=\n\t"
        "s_mov_b32 s45, 1\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt lgkmcnt(0)\n\t"
        DSI_ASM_VPREP2("v[50:52]", "v[54:57]", "v53")
        "s_mov_b32 s52, 3\n\t"
        "s_cmp_lt_i32 2, %2\n\t"
        "s_cbranch_scc0 Ldrain%=\n\t"
        "s_mov_b32 s45, 2\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt lgkmcnt(0)\n\t"
        DSI_ASM_VPREP2("v[24:26]", "v[28:31]", "v27")
        "Lloop%=:\n\t"
        // ---- batch k in set A; B and C in flight behind it
        "s_add_i32 s45, s42, 3\n\t"
        "s_cmp_lt_i32 s45, %2\n\t"
        "s_mov_b32 s52, 7\n\t"
        "s_cbranch_scc0 Ldrain%=\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt vmcnt(6)\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "s_waitcnt lgkmcnt(4)\n\t"
        DSI_ASM_VPREP2("v[42:44]", "v[46:49]", "v45")
        "s_add_i32 s42, s42, 1\n\t"
        // ---- batch k in set B; C and A behind it
        "s_add_i32 s45, s42, 3\n\t"
        "s_cmp_lt_i32 s45, %2\n\t"
        "s_cbranch_scc0 Ldrain%=\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt vmcnt(6)\n\t"
        DSI_ASM_VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")
        "s_waitcnt lgkmcnt(4)\n\t"
        DSI_ASM_VPREP2("v[50:52]", "v[54:57]", "v53")
        "s_add_i32 s42, s42, 1\n\t"
        // ---- batch k in set C; A and B behind it
        "s_add_i32 s45, s42, 3\n\t"
        "s_cmp_lt_i32 s45, %2\n\t"
        "s_cbranch_scc0 Ldrain%=\n\t"
        DSI_ASM_VPREP1
        "s_waitcnt vmcnt(6)\n\t"
        DSI_ASM_VOTE("v24", "v25", "v26", "v28", "v29", "v30", "v31", "v27")
        "s_waitcnt lgkmcnt(4)\n\t"
        DSI_ASM_VPREP2("v[24:26]", "v[28:31]", "v27")
        "s_add_i32 s42, s42, 1\n\t"
        "s_branch Lloop%=\n"
        // ---- everything that is still in flight (1..3 batches: exactly nb - k of them, and when the
        //      loop has run all three sets hold one) is voted after one wait, in any order
        "Ldrain%=:\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_bitcmp1_b32 s52, 0\n\t"
        "s_cbranch_scc0 LnoA%=\n\t"
        DSI_ASM_VOTE("v42", "v43", "v44", "v46", "v47", "v48", "v49", "v45")
        "LnoA%=:\n\t"
        "s_bitcmp1_b32 s52, 1\n\t"
        "s_cbranch_scc0 LnoB%=\n\t"
        DSI_ASM_VOTE("v50", "v51", "v52", "v54", "v55", "v56", "v57", "v53")
        "LnoB%=:\n\t"
        "s_bitcmp1_b32 s52, 2\n\t"
        "s_cbranch_scc0 LnoC%=\n\t"
        DSI_ASM_VOTE("v24", "v25", "v26", "v28", "v29", "v30", "v31", "v27")
        "LnoC%=:\n\t"
        "s_waitcnt vmcnt(0) lgkmcnt(0)"
        :
        : "s"(sxy), "s"(coef4), "s"(s_nb), "s"(s_slot0), "s"(s_T), "v"(wlo), "v"(whi), "v"(cb), "s"(s_tab),
          "s"(s_nx8), "s"(s_cbase), "s"(s_nxm2), "s"(s_Li), "s"(s_Uim1), "v"(dummy_eo * 12u), "v"(lane),
          "v"(0), "v"(lane * 12)
        : "memory", "scc", "vcc", "s42", "s45", "s46", "s49", "s50", "s51", "s52", "v24", "v25", "v26", "v27",
          "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v42", "v43",
          "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58",
          "v59", "v60", "v61", "v62", "v63");
}

// the passes of a wave: per-pass tables by compiled code, the batches by vfill_range_asm
__device__ __forceinline__ void vfill_stream_asm(const EvRec* __restrict__ sxy,
                                                 const uint4* __restrict__ coef4,
                                                 const uint32_t* __restrict__ cutz,
                                                 char* __restrict__ band_bytes,
                                                 unsigned long long* __restrict__ scratch,
                                                 int p_first, int p_end, int lg_pass, int stride,
                                                 int lane, int nx, int Li, int Ui, int row_base,
                                                 uint32_t dummy_eo, int variant, int p_begin_of_wg,
                                                 int* __restrict__ pass_counter, const InlineCuts& ic)
{
    if (Ui - 1 < Li) return;  // the band accepts no row (the unsigned range test needs Ui-1-Li >= 0)
    const int pass = 1 << lg_pass;
    const int p_begin = p_begin_of_wg;
    (void)stride;
    // Passes are DEALT, not pre-assigned, in UNITS of half a pass: wave w starts with units 2w and 2w + 1 and
    // draws every further stretch from a counter in LDS (set to twice the number of waves by the item's set-up).
    // A pass holds 64 packets' records of this band and plane -- anything from a few hundred to a few thousand
    // slots -- and an item has only ~2-10 passes per wave, so with fixed assignments the workgroup waited for its
    // unluckiest wave.  A draw takes two units (a whole pass: the per-pass set-up is amortised over 64 packets)
    // until few are left, then one (guided: the waves finish within half a pass of each other).  (The sums are
    // integer: which wave votes a pass does not change a bit.)
    const int half = pass >> 1;
    const int n_units = (p_end - p_begin + half - 1) / half;
    // single units once fewer than kGuided per wave remain (variant 100, experiments builds only: never, i.e. whole
    // passes to the end as in round 2, for same-box A/B runs)
    const int kGuided = (variant >= 100 && variant <= 108) ? variant - 100 : 4;
    const int n_waves_wg = (int)(blockDim.x >> 6);
    auto draw = [&](int& take) {
        int v = 0, t = 2;
        if (lane == 0) {
            const int seen = __hip_atomic_load(pass_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = (kGuided == 0 || n_units - seen > kGuided * n_waves_wg) ? 2 : 1;
            v = atomicAdd(pass_counter, t);
        }
        take = __builtin_amdgcn_readfirstlane(t);
        return __builtin_amdgcn_readfirstlane(v);
    };
    // lane l = packet l of the stretch that starts at unit u.  (Tried: interleaved passes -- lane l = packet
    // p_begin + l * npass + j, so that the 3-4 packets a batch mixes are far apart in time and a scene point's
    // votes do not meet in one wave instruction: -1 % ... +3 %, not adopted.  Tried: the ds_bpermute look-ups
    // issued a further iteration ahead, waited for with lgkmcnt(6): no change, 5.01 vs 5.00 ms.)
    auto packet_of = [&](int u) { return p_begin + u * half + lane; };
    const int u0 = 2 * ((p_first - p_begin) / pass);  // this wave's first stretch: a whole pass
    uint32_t cu_next = 0;
    // BandPlan::cuts_inline (ic.rsT): no cut table.  The runs of a stretch come in two dependent steps -- the packets'
    // {flags, d_a, by_a}, then two entries of the transposed row table -- so stretches are drawn TWO ahead: while stretch
    // u is voted, step 2 of stretch u' (the next) and step 1 of stretch u'' (the one after) are in flight.
    const bool inl = ic.rsT != nullptr;
    uint4 c1_next = make_uint4(0u, 0u, 0u, 0u);   // step 1 of the stretch after this one
    uint32_t e_lo = 0, e_hi = 0, e_flags = kCoefSkip;  // step 2 of this stretch (arrives during the previous one)
    int u_after = n_units, t_after = 2;
    bool valid_next = false;
    auto lanes_of = [&](int u, int t) { return u < n_units && lane < t * half && packet_of(u) < p_end; };
    auto step2 = [&](uint4 c1, int p, bool valid) {
        e_flags = kCoefSkip;
        e_lo = e_hi = 0;
        if (valid) {
            uint32_t at_lo, at_hi;
            inline_cut_entries(ic, c1, 2u * (uint32_t)p, &at_lo, &at_hi);
            e_flags = c1.y;
            e_lo = inline_cut_load(ic, at_lo);
            e_hi = inline_cut_load(ic, at_hi);
        }
    };
    int take = 2, tn = 2;
    if (inl) {
        const bool v0 = lanes_of(u0, 2);
        uint4 c1 = make_uint4(0u, 0u, 0u, 0u);
        if (v0) c1 = coef4[2 * (size_t)packet_of(u0) + 1];
        u_after = draw(t_after);                     // the second stretch
        valid_next = lanes_of(u_after, t_after);
        if (valid_next) c1_next = coef4[2 * (size_t)packet_of(u_after) + 1];
        step2(c1, packet_of(u0), v0);                // (waits for the first stretch's step 1: once per item and wave)
    } else if (u0 < n_units && lane < pass && packet_of(u0) < p_end) {
        cu_next = cutz[packet_of(u0)];
    }
    for (int u = u0, un; u < n_units; u = un, take = tn) {
        const int p = packet_of(u);
        uint32_t cu;
        (void)take;  // (lanes beyond the stretch loaded no cut word: length 0)
        if (inl) {
            cu = inline_cut_word(e_flags, e_lo, e_hi);   // this stretch's entries (requested one stretch ago)
            un = u_after;
            tn = t_after;
            const uint4 c1 = c1_next;                    // the next stretch's step 1 (requested one stretch ago) ...
            const bool vn = valid_next;
            u_after = draw(t_after);                     // ... the stretch after it is drawn now, its step 1 requested ...
            valid_next = lanes_of(u_after, t_after);
            c1_next = make_uint4(0u, 0u, 0u, 0u);
            if (valid_next) c1_next = coef4[2 * (size_t)packet_of(u_after) + 1];
            step2(c1, packet_of(un), vn);                // ... and the next stretch's entries
        } else {
            cu = cu_next;
            // the next stretch is drawn now and its cut words travel while this one is voted
            un = draw(tn);
            cu_next = 0;
            if (un < n_units && lane < tn * half && packet_of(un) < p_end) cu_next = cutz[packet_of(un)];
        }
        const int lo = (int)(cu & 0xffffu), hi = (int)(cu >> 16);
        const int len = max(hi - lo, 0);
        const int incl = wave_incl_scan(len, lane);
        const int T = __builtin_amdgcn_readlane(incl, 63);
        if (T == 0) continue;
        const int D = (p << 10) + lo - (incl - len);
        const unsigned long long ne = __builtin_amdgcn_ballot_w64(len > 0);
        const int c = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ne >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)ne, 0u));
        const int dst = len > 0 ? c : 63 - (lane - c);  // non-empty runs to lanes 0, 1, ...; the rest behind
        // table entry of compacted run `dst`: {12 * D (byte offsets of 12-byte records, mod 2^32), byte
        // offset of the packet's coefficients}
        const unsigned long long entry =
            (unsigned long long)(uint32_t)(D * 12) | ((unsigned long long)(uint32_t)(min(p, p_end - 1) << 5) << 32);
        int Cbase = 0;
        for (int rbase = 0; rbase < T; rbase += 4096) {
            scratch[lane] = 0ull;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const int ts = incl - 1 - rbase;  // last slot of this lane's run, relative to the range
            if (len > 0 && ts >= 0 && ts < 4096) atomicOr(&scratch[ts >> 6], 1ull << (ts & 63));
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const unsigned long long w = scratch[lane];
            // the tail words now live in registers: the same words carry the run table
            // {D, coefficient byte offset} of the compacted runs, one ds_read_b64 per batch instead
            // of two ds_bpermute
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            scratch[dst] = entry;  // (a permutation of the lanes: every entry 0..63 is written)
            // slots beyond the pass count all R <= 64 runs as ended: entry 64 must hold a valid
            // coefficient offset too (their record is the multiplicity-0 dummy)
            if (lane == 0) scratch[64] = entry;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const int pc = __builtin_popcountll(w);
            const int inc = wave_incl_scan(pc, lane);
            const int nb = min(64, (T - rbase + 63) >> 6);
            if (variant == 3)
                vfill_range_asm(sxy, coef4, nb, rbase, T, (uint32_t)w, (uint32_t)(w >> 32), inc - pc + Cbase, scratch,
                                band_bytes, lane, nx, Li, Ui, row_base, dummy_eo);
            else
                vfill_range_asm3(sxy, coef4, nb, rbase, T, (uint32_t)w, (uint32_t)(w >> 32), inc - pc + Cbase, scratch,
                                 band_bytes, lane, nx, Li, Ui, row_base, dummy_eo);
            Cbase += __builtin_amdgcn_readlane(inc, 63);
        }
    }
}

// ---- the same hand-scheduled loop over GROUPS of S packets sorted together (lane mapping 4).
// A run is then S times longer (wide grids: ~19 records per packet and band at 1024 x 1024, which
// makes the per-packet stream scalar-bound at 4.4 run pieces per batch).  A record's coefficients
// now depend on the record (its packet index within the group sits in the high half of m), so
// the pipeline is three batches deep: records of batch i+2 and coefficients of batch i+1 are in
// flight while batch i is voted; three register slots, loop unrolled three times.
//   s47,s48,s49 lanes of the batches in slots 0,1,2      v52 record index per lane   v53 cut words
//   slot 0: v[20:22] record  v23 group's coefficient base  v[24:27] a,bx,by,d  v28 r
//   slot 1: v[30:32]         v33                           v[40:43]            v29
//   slot 2: v[44:46]         v47                           v[48:51]            v34
//   temporaries v36-v39, v56-v63 (v57 = multiplicity)
#define DSI_ASM_FILL_G(NOUT, L)                                                                    \
    "s_mov_b32 s44, 0\n"                                                                            \
    "Ltop" L "%=:\n\t"                                                                              \
    "s_cmp_ge_i32 s40, s41\n\t"                                                                     \
    "s_cbranch_scc1 Lnext" L "%=\n\t"                                                               \
    "s_sub_i32 s45, 64, s44\n\t"                                                                    \
    "s_sub_i32 s46, s41, s40\n\t"                                                                   \
    "s_min_i32 s45, s45, s46\n\t"                                                                   \
    "s_sub_i32 s46, s40, s44\n\t"                                                                   \
    "s_lshl_b64 exec, -1, s44\n\t"                                                                  \
    "v_add_u32 v52, s46, %15\n\t"                                                                   \
    "s_mov_b64 exec, -1\n\t"                                                                        \
    "s_add_i32 s44, s44, s45\n\t"                                                                   \
    "s_add_i32 s40, s40, s45\n\t"                                                                   \
    "s_cmp_lt_u32 s44, 64\n\t"                                                                      \
    "s_cbranch_scc0 Ldone" L "%=\n"                                                                 \
    "Lnext" L "%=:\n\t"                                                                             \
    "s_add_i32 s42, s42, 1\n\t"                                                                     \
    "s_cmp_ge_i32 s42, %3\n\t"                                                                      \
    "s_cbranch_scc1 Leos" L "%=\n\t"                                                                \
    "s_and_b32 s45, s42, %4\n\t"                                                                    \
    "s_cmp_eq_u32 s45, 0\n\t"                                                                       \
    "s_cbranch_scc1 Lreload" L "%=\n\t"                                                             \
    "v_readlane_b32 s46, v53, s45\n\t"                                                              \
    "s_add_i32 s43, s43, %16\n"           /* next group: S * 1024 records further */                \
    "Lhave" L "%=:\n\t"                                                                             \
    "s_and_b32 s45, s46, 0xffff\n\t"                                                                \
    "s_lshr_b32 s46, s46, 16\n\t"                                                                   \
    "s_add_i32 s40, s43, s45\n\t"                                                                   \
    "s_add_i32 s41, s43, s46\n\t"                                                                   \
    "s_branch Ltop" L "%=\n"                                                                        \
    "Lreload" L "%=:\n\t"                                                                           \
    "s_lshr_b32 s45, s42, %7\n\t"                                                                   \
    "s_mul_i32 s45, s45, %6\n\t"                                                                    \
    "s_add_i32 s45, s45, %5\n\t"          /* first group of the pass */                             \
    "s_mul_i32 s43, s45, %16\n\t"                                                                   \
    "v_add_u32 v58, s45, %15\n\t"                                                                   \
    "v_min_i32 v58, %8, v58\n\t"                                                                    \
    "v_lshlrev_b32 v58, 2, v58\n\t"                                                                 \
    "global_load_dword v53, v58, %2\n\t"                                                            \
    "s_waitcnt vmcnt(0)\n\t"                                                                        \
    "v_readfirstlane_b32 s46, v53\n\t"                                                              \
    "s_branch Lhave" L "%=\n"                                                                       \
    "Leos" L "%=:\n\t"                                                                              \
    "s_cmp_eq_u32 s44, 0\n\t"                                                                       \
    "s_cbranch_scc1 Ldone" L "%=\n\t"                                                               \
    "s_lshl_b64 exec, -1, s44\n\t"                                                                  \
    "v_mov_b32 v52, %14\n\t"                                                                        \
    "s_mov_b64 exec, -1\n"                                                                          \
    "Ldone" L "%=:\n\t"                                                                             \
    "s_mov_b32 " NOUT ", s44\n\t"

// request the records of the batch just filled; keep the byte offset of its group's coefficients
#define DSI_ASM_GREC(REC, GB)                                                                      \
    "v_mul_lo_u32 v56, v52, 12\n\t"                                                                 \
    "v_lshrrev_b32 " GB ", 10, v52\n\t"   /* packet of the record, if groups were single packets */ \
    "v_and_b32 " GB ", %17, " GB "\n\t"   /* first packet of the group */                           \
    "v_lshlrev_b32 " GB ", 5, " GB "\n\t" /* 32 bytes per coefficient set */                        \
    "global_load_dwordx3 " REC ", v56, %0\n\t"

// the records have arrived: request each lane's coefficients (packet index = high half of m)
#define DSI_ASM_GCOEF(M, GB, CA, CR)                                                               \
    "v_lshrrev_b32 v56, 16, " M "\n\t"                                                              \
    "v_lshl_add_u32 v56, v56, 5, " GB "\n\t"                                                        \
    "global_load_dwordx4 " CA ", v56, %1\n\t"                                                       \
    "global_load_dword " CR ", v56, %1 offset:16\n\t"

#define DSI_ASM_GITER(NJ, RECJ2, GBJ2, NJ2, MJ1, GBJ1, CAJ1, CRJ1, EX, EY, EM, KA, KBX, KBY, KD, KR, L) \
    DSI_ASM_FILL_G(NJ2, L)                                                                         \
    DSI_ASM_GREC(RECJ2, GBJ2)                                                                      \
    "s_waitcnt vmcnt(3)\n\t"              /* records of the next batch are here */                  \
    DSI_ASM_GCOEF(MJ1, GBJ1, CAJ1, CRJ1)                                                           \
    "s_waitcnt vmcnt(3)\n\t"              /* coefficients of this batch are here */                 \
    "s_cmp_eq_u32 " NJ ", 0\n\t"                                                                    \
    "s_cbranch_scc1 Lend%=\n\t"                                                                     \
    "v_and_b32 v57, 0xffff, " EM "\n\t"   /* multiplicity */                                        \
    DSI_ASM_VOTE(EX, EY, "v57", KA, KBX, KBY, KD, KR)

__device__ __forceinline__ void group_stream_asm(const EvRec* sxy, const uint4* coef4,
                                                 const uint32_t* cutz, char* band_bytes,
                                                 int g_first, int g_end, int lg_pass, int stride,
                                                 int lane, int nx, int Li, int Ui, int row_base,
                                                 uint32_t dummy_eo, int S)
{
    const int pass = 1 << lg_pass;
    int n_my = 0;
    if (g_first < g_end) {
        const int passes = (g_end - g_first + stride - 1) / stride;
        const int last = g_first + (passes - 1) * stride;
        n_my = (passes - 1) * pass + min(pass, g_end - last);
    }
    if (Ui - 1 < Li) n_my = 0;  // no acceptable row (the unsigned range test needs Ui-1-Li >= 0)
    const int s_n_my = __builtin_amdgcn_readfirstlane(n_my);
    const int s_gmask = __builtin_amdgcn_readfirstlane(pass - 1);
    const int s_g_first = __builtin_amdgcn_readfirstlane(g_first);
    const int s_stride = __builtin_amdgcn_readfirstlane(stride);
    const int s_lg = __builtin_amdgcn_readfirstlane(lg_pass);
    const int s_g_last = __builtin_amdgcn_readfirstlane(g_end - 1);
    const int s_nx8 = __builtin_amdgcn_readfirstlane(nx * 8);
    const int lds_base = (int)(uintptr_t)band_bytes;
    const int s_cbase = __builtin_amdgcn_readfirstlane(lds_base - row_base * nx * 8);
    const int s_nxm2 = __builtin_amdgcn_readfirstlane(nx - 2);
    const int s_Li = __builtin_amdgcn_readfirstlane(Li);
    // rows the band accepts: 0 <= yi - Li <= Ui - 1 - Li  (a band with no acceptable row gets no stream)
    const int s_Uim1 = __builtin_amdgcn_readfirstlane(Ui - 1 - Li);
    const uint32_t s_dummy = __builtin_amdgcn_readfirstlane(dummy_eo);
    const int s_gs = __builtin_amdgcn_readfirstlane(S * kPacket);
    const int s_pkmask = __builtin_amdgcn_readfirstlane(~(S - 1));
    asm volatile(
        "s_mov_b32 s42, -1\n\t"
        "s_mov_b32 s40, 0\n\t"
        "s_mov_b32 s41, 0\n\t"
        "s_mov_b32 s43, 0\n\t"
        "v_mov_b32 v52, 0\n\t"
        "v_mov_b32 v53, 0\n\t"
        DSI_ASM_FILL_G("s47", "p")
        DSI_ASM_GREC("v[20:22]", "v23")
        DSI_ASM_FILL_G("s48", "q")
        DSI_ASM_GREC("v[30:32]", "v33")
        "s_waitcnt vmcnt(1)\n\t"
        DSI_ASM_GCOEF("v22", "v23", "v[24:27]", "v28")
        "Lloop%=:\n\t"
        DSI_ASM_GITER("s47", "v[44:46]", "v47", "s49", "v32", "v33", "v[40:43]", "v29",
                      "v20", "v21", "v22", "v24", "v25", "v26", "v27", "v28", "a")
        DSI_ASM_GITER("s48", "v[20:22]", "v23", "s47", "v46", "v47", "v[48:51]", "v34",
                      "v30", "v31", "v32", "v40", "v41", "v42", "v43", "v29", "b")
        DSI_ASM_GITER("s49", "v[30:32]", "v33", "s48", "v22", "v23", "v[24:27]", "v28",
                      "v44", "v45", "v46", "v48", "v49", "v50", "v51", "v34", "c")
        "s_branch Lloop%=\n"
        "Lend%=:\n\t"
        "s_waitcnt vmcnt(0) lgkmcnt(0)"
        :
        : "s"(sxy), "s"(coef4), "s"(cutz), "s"(s_n_my), "s"(s_gmask), "s"(s_g_first), "s"(s_stride),
          "s"(s_lg), "s"(s_g_last), "s"(s_nx8), "s"(s_cbase), "s"(s_nxm2), "s"(s_Li), "s"(s_Uim1),
          "s"(s_dummy), "v"(lane), "s"(s_gs), "s"(s_pkmask)
        : "memory", "scc", "vcc", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49",
          "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32",
          "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45",
          "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58",
          "v59", "v60", "v61", "v62", "v63");
}

// The votes of ONE work item (band j, plane z, packets [p_begin, p_end) of one camera) into the band in
// LDS: every wave of the workgroup streams its share of the packets.  LDS row 0 of the band is grid
// row `row_base`; the item accepts events with floor(Y) in [Li, Ui - 1].
// MAPPING = the lane mapping (1 packed / hand-scheduled, 3 packed / compiled, 5 vector fill /
// hand-scheduled, 6 vector fill / compiled, 7 packed / hand-scheduled with dealt passes).  TWO_SETS: the vector fill keeps two instead of three batches of
// gathers in flight (32 instead of 40 named registers; the fused kernel needs the difference).  DEAL: the hand-scheduled
// packed stream draws its passes from *s_pass instead of taking every kWaves-th one.
template <int BLOCK, int MAPPING, bool TWO_SETS = false, bool DEAL = false>
__device__ __forceinline__ void stream_item(const EvRec* __restrict__ sxy, const PlaneCoef* __restrict__ coef,
                                            const uint32_t* __restrict__ cuts, const uint32_t* __restrict__ slow_any,
                                            int np, const Geom& g, const BandPlan& bp, int j, int z, int p_begin,
                                            int p_end, char* __restrict__ band_bytes, int Li, int Ui, int row_base,
                                            int* __restrict__ s_pass, uint32_t first_cuts = 0)
{
    const int nx = g.nx;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int lane = threadIdx.x & (kWave - 1);
    // packets a wave takes per pass:
    constexpr int kWaves = BLOCK / kWave;
    // as many as possible (fewer pass boundaries), but every wave should get >= 3 passes so that the
    // waves of the workgroup finish together (measured: 2 % at 346x260, 6 % at 512x512 against one
    // pass per wave; 512x512x200, 489 packets: passes of 16 / 8 / 4 / 2 packets 0.224 / 0.216 / 0.219 /
    // 0.232 ms)
    int lg_group = 6;
    while (lg_group > 2 && (p_end - p_begin) < ((kWaves * 3) << lg_group)) --lg_group;
    if (bp.pass_lg > 0) lg_group = bp.pass_lg;
    const int group = 1 << lg_group;
    const uint4* __restrict__ coef4 = reinterpret_cast<const uint4*>(coef) + 2 * (size_t)z * np;
    // (bp.cuts_inline: `cuts` is the transposed row table, there is no table row of this item)
    const uint32_t* __restrict__ cutz = bp.cuts_inline ? cuts : cuts + ((size_t)j * g.nz + z) * np;
    // record np * 1024 is a dummy with multiplicity 0 (k_sort_packets) for the lanes a short last
    // batch does not reach; "its" coefficients are whatever follows the plane's table
    const uint32_t dummy_eo = (uint32_t)np * (uint32_t)kPacket;
    if constexpr (MAPPING == 5 || MAPPING == 6) {
        // vector fill (wide grids): passes of up to 64 packets, smaller when the chunk has few
        // packets so that every wave gets >= 2 passes; 64 words of LDS per wave behind the band.
        // 5 = hand-scheduled batches, 6 = all compiled (A/B tests; also the IEEE-divide planes of 5)
        // (the per-pass set-up costs a few LDS round trips: as few, as large passes as keep every
        //  wave busy)
        int lg_pass = 6;
        while (lg_pass > 3 && (p_end - p_begin) < (kWaves << lg_pass)) --lg_pass;
        if (bp.pass_lg > 0) lg_pass = bp.pass_lg;
        const int pass = 1 << lg_pass;
        unsigned long long* scratch =
            reinterpret_cast<unsigned long long*>(band_bytes + bp.scratch_offset) + wave * kVfillScratchWords;
        const InlineCuts ic = inline_cuts_of(cuts, g, bp, j);  // (ic.rsT != nullptr: `cuts` is the transposed row table)
        if (slow_any[z] != 0)
            vfill_stream<true>(sxy, coef4, cutz, band_bytes, scratch, p_begin + wave * pass, p_end, lg_pass,
                               kWaves * pass, lane, nx, Li, Ui, row_base, dummy_eo, ic);
        else if constexpr (MAPPING == 6)
            vfill_stream<false>(sxy, coef4, cutz, band_bytes, scratch, p_begin + wave * pass, p_end, lg_pass,
                                kWaves * pass, lane, nx, Li, Ui, row_base, dummy_eo, ic);
        else
            vfill_stream_asm(sxy, coef4, cutz, band_bytes, scratch, p_begin + wave * pass, p_end, lg_pass,
                             kWaves * pass, lane, nx, Li, Ui, row_base, dummy_eo, TWO_SETS ? 3 : bp.experiment, p_begin, s_pass, ic);
    } else {
        // MAPPING 3 is the compiled stream on the fast path too (A/B testing)
        if (slow_any[z] != 0)
            packed_stream<true, MAPPING == 8>(sxy, coef4, cutz, band_bytes, p_begin + wave * group, p_end, lg_group,
                                              kWaves * group, lane, nx, Li, Ui, row_base, dummy_eo, paired_row_words(nx) * 8);
        else if constexpr (MAPPING == 3)
            packed_stream<false>(sxy, coef4, cutz, band_bytes, p_begin + wave * group, p_end, lg_group,
                                 kWaves * group, lane, nx, Li, Ui, row_base, dummy_eo);
        else if constexpr (MAPPING == 8) {  // mapping 7's stream on paired 32-bit cells (opt-in, NOT the exact sums)
            int lg = (p_end - p_begin) >= kWaves * 16 ? 3 : 2;
            while (lg < 5 && (p_end - p_begin) >= ((kWaves * 16) << (lg + 1))) ++lg;
            if (bp.pass_lg > 0) lg = bp.pass_lg;
            first_cuts = p_end > p_begin ? cutz[min(p_begin + (wave << lg) + lane, p_end - 1)] : 0u;
            packed_stream_asm_dealt<true>(sxy, coef4, cutz, band_bytes, p_begin, p_end, lg, wave, kWaves, lane, nx, Li, Ui, row_base,
                                          dummy_eo, s_pass, first_cuts, paired_row_words(nx) * 8);
        }
        else if constexpr (DEAL || MAPPING == 7) {
            // (*s_pass = 2 * kWaves, set by the item's set-up.)  Packets per pass: enough passes per wave for the dealing
            // to balance the waves (>= ~16), few enough switches (each costs a wait for the wave's outstanding LDS
            // operations): 4 at a 50 ms window's 489 packets (measured 4 / 8 / 16: 446 / 455 / 471 us for the fused kernel),
            // 16 at 4,900 (346x260x100: 1.190 / 1.182 / 1.179 ms for 4 / 8 / 16), 16-32 at 9,800 (512x512x200, 10 M
            // events: 2.76 / 2.62 / 2.55 ms for 4 / 8 / 16)
            // Re-measured at the end of round 3 (passes of 4 / 8 / 16 packets, kernel time): 976 packets 346x260x100
            // 146.5 / 143.6 / 143.4 us; 3,906 packets 497 / 491 / 492 us, at 512x512x200 1.138 / 1.095 / 1.088 ms; a window's
            // 489 packets in the fused kernel 431.9 / 430.6 / 458.5 us (2 packets: 450.9) -- 8 is never worse than 4.
            int lg = (p_end - p_begin) >= kWaves * 16 ? 3 : 2;
            while (lg < 5 && (p_end - p_begin) >= ((kWaves * 16) << (lg + 1))) ++lg;
            if (bp.pass_lg > 0) lg = bp.pass_lg;
            if constexpr (!DEAL)  // nobody loaded the wave's first cut words ahead of time (the fused kernel does)
                first_cuts = p_end > p_begin ? cutz[min(p_begin + (wave << lg) + lane, p_end - 1)] : 0u;
            packed_stream_asm_dealt(sxy, coef4, cutz, band_bytes, p_begin, p_end, lg, wave, kWaves,
                                    lane, nx, Li, Ui, row_base, dummy_eo, s_pass, first_cuts);
        }
        else
            packed_stream_asm(sxy, coef4, cutz, band_bytes, p_begin + wave * group, p_end, lg_group,
                              kWaves * group, lane, nx, Li, Ui, row_base, dummy_eo);
    }
}

// One kernel per mapping, so that each carries only its own
// streams (all of them in one kernel needed 70 VGPRs -- 7 waves per SIMD, i.e. ONE 1024-thread
// workgroup per CU instead of two -- and spilled scalars).  8 waves per SIMD = at most 64 VGPRs.
template <int BLOCK, int MAPPING>
__device__ __forceinline__ void vote_bands_packed_body(const EvRec* __restrict__ sxy,
                                                       const PlaneCoef* __restrict__ coef,
                                                       const uint32_t* __restrict__ cuts,
                                                       const uint32_t* __restrict__ slow_any,
                                                       int np, const Geom& g, const BandPlan& bp,
                                                       void* __restrict__ out,
                                                       acc_t* __restrict__ seam,
                                                       uint32_t* __restrict__ work_counters)
{
    extern __shared__ acc_t band[];
    __shared__ int s_item;
    __shared__ int s_pass;  // mapping 5: the next pass of the item to hand out (vfill_stream_asm)
    const int pairs = bp.chunks * bp.bands;
    const int total = item_count(pairs, g.nz, bp.experiment == 200);
    const int nx = g.nx;
    // PERSISTENT workgroups (work_counters != nullptr): the grid is only as large as the chip holds
    // at once and every workgroup pulls work items until none is left -- a 1024-thread workgroup
    // with up to 160 KB of LDS costs ~5 us to launch and a CU cannot overlap that with the previous
    // workgroup (measured at 512x512x200: 7.7 us of fixed cost per work item, 38 % of a 500 k-event
    // launch).  Items are dealt per XCD class (block % 8, the dispatch rule the block -> (pair, plane)
    // mapping relies on): class x takes items x, x + 8, x + 16, ... in order, through one atomic
    // counter per class, so the load stays balanced like the hardware's own dispatch.
    const int cls = blockIdx.x & 7;
    __shared__ int s_next;  // persistent: the item AFTER the current one, drawn while the current one is voted
    constexpr bool kPaired = MAPPING == 8;
    const int row_words = kPaired ? paired_row_words(nx) : nx;  // 8-byte words per band row
    if (work_counters) {
        const int all_cells = (bp.band_rows + 1) * row_words;
        for (int i = threadIdx.x; i < all_cells; i += BLOCK) band[i] = 0;
        if (threadIdx.x == 0) {
            s_item = (int)atomicAdd(&work_counters[cls], 1u) * 8 + cls;
            s_pass = 2 * (BLOCK / kWave);  // (vector fill: units of half a pass, two pre-assigned per wave)
        }
        __syncthreads();
    }
    for (;;) {
    const int b = work_counters ? s_item : (int)blockIdx.x;
    if (b >= total) break;
    int q, z;
    if (!item_of(b, pairs, g.nz, q, z, bp.experiment == 200)) {  // (a leftover slot beyond the last plane)
        if (!work_counters) break;
        __syncthreads();  // every thread has read s_item before thread 0 draws again
        if (threadIdx.x == 0) s_item = (int)atomicAdd(&work_counters[cls], 1u) * 8 + cls;
        __syncthreads();
        continue;
    }
    // Round 4: the NEXT item is drawn now, at the start of this one.  Only thread 0's wave waits for the atomic's round
    // trip (~1 us); the other 15 waves are already voting, and because the waves of a workgroup draw their passes from a
    // counter, a wave that enters the stream late simply takes fewer passes.  Drawn after the flush (rounds 2-3), the
    // round trip stood between two items with all 16 waves idle: 61 items per CU at 1024x1024x256.
    if (work_counters && threadIdx.x == 0) s_next = (int)atomicAdd(&work_counters[cls], 1u) * 8 + cls;
    const int c = q / bp.bands, j = q % bp.bands;
    const int r0 = j * bp.band_rows;
    const int r1 = min(g.ny, r0 + bp.band_rows);
    const int cells = (r1 - r0 + 1) * row_words;  // owned rows + the carry row
    if (!work_counters) {
        for (int i = threadIdx.x; i < cells; i += BLOCK) band[i] = 0;
        if (threadIdx.x == 0) s_pass = 2 * (BLOCK / kWave);
        __syncthreads();
    }

    const int p_begin = (int)(((long long)np * c) / bp.chunks);
    const int p_end = (int)(((long long)np * (c + 1)) / bp.chunks);
    if (bp.experiment != 1)  // (1: timing experiment, the item's fixed cost only: zero, barriers, flush)
        stream_item<BLOCK, MAPPING>(sxy, coef, cuts, slow_any, np, g, bp, j, z, p_begin, p_end,
                                    reinterpret_cast<char*>(band), r0, min(r1, g.ny - 1), r0, &s_pass);
    __syncthreads();

    const size_t vol = partial_stride((size_t)g.nx * g.ny * g.nz);
    const size_t off = (size_t)c * vol + ((size_t)z * g.ny + r0) * nx;
    if constexpr (kPaired) {
        // (the overflow word sits behind the per-plane flags and the 8 work counters: zeroed by the sort kernel)
        flush_band_paired<BLOCK>(band, nx, r1 - r0, out, off, bp.raw_out, seam_rows(seam, c, z, j, g, bp), j, bp.bands,
                                 const_cast<uint32_t*>(slow_any) + g.nz + 8);
        if (!work_counters) break;
    } else {
    if (!work_counters) {
        flush_band<BLOCK>(band, nx, (r1 - r0) * nx, out, off, bp.raw_out, seam_rows(seam, c, z, j, g, bp), j, bp.bands);
        break;
    }
    if (bp.experiment != 2)  // (2: timing experiment without the flush)
        flush_band_and_clear<BLOCK>(band, nx, (r1 - r0) * nx, out, off, bp.raw_out, seam_rows(seam, c, z, j, g, bp), j, bp.bands);
    }
    if (threadIdx.x == 0) {  // (every thread read s_item before the stream's barrier; s_pass is idle between the barriers)
        s_item = s_next;
        s_pass = 2 * (BLOCK / kWave);
    }
    __syncthreads();  // the band is clear and the next item known before anybody goes on
    }
}

template <int BLOCK, int MAPPING>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_vote_bands_packed(
    const EvRec* __restrict__ sxy, const PlaneCoef* __restrict__ coef, const uint32_t* __restrict__ cuts,
    const uint32_t* __restrict__ slow_any, int np, Geom g, BandPlan bp, void* __restrict__ out,
    acc_t* __restrict__ seam, uint32_t* __restrict__ work_counters)
{
    vote_bands_packed_body<BLOCK, MAPPING>(sxy, coef, cuts, slow_any, np, g, bp, out, seam, work_counters);
}

// The vector-fill mappings run where ONE workgroup fills a CU (wide grids): 4 waves per SIMD may use up
// to 128 VGPRs, which pays for a third register set -- three batches of gathers in flight.  (Run with a
// band small enough for two workgroups per CU, this kernel still places only one.)
template <int BLOCK, int MAPPING>
__global__ __launch_bounds__(BLOCK) void k_vote_bands_vfill(
    const EvRec* __restrict__ sxy, const PlaneCoef* __restrict__ coef, const uint32_t* __restrict__ cuts,
    const uint32_t* __restrict__ slow_any, int np, Geom g, BandPlan bp, void* __restrict__ out,
    acc_t* __restrict__ seam, uint32_t* __restrict__ work_counters)
{
    vote_bands_packed_body<BLOCK, MAPPING>(sxy, coef, cuts, slow_any, np, g, bp, out, seam, work_counters);
}

// the 2-ary camera-fusion ops of Grid3D (cartesian3dgrid.h:111-192), used by the fused kernel below and by
// the Grid3D kernels further down
// Grid3D::harmonicMeanTwoGrids(grid2, n) (cartesian3dgrid.h:130-139); fn = n, fn1 = n - 1
__device__ __forceinline__ float harmonic_mean_n(float a, float g, float fn, float fn1)
{
    const float av = a / fn1;
    const float prod = av * g, sum = av + g;
    return fn * prod / (sum + 0.1f);
}

template <int OP>
__device__ __forceinline__ float fuse_op(float a, float g)
{
    if (OP == 1) return (g < a) ? g : a;  // std::min, cartesian3dgrid.h:115
    if (OP == 2) {                        // :119-127, eps = 1e-1f in the denominator
        const float prod = a * g, sum = a + g;
        return 2.f * prod / (sum + 0.1f);
    }
    if (OP == 3) return __builtin_sqrtf(a * g);  // :154
    if (OP == 4) return 0.5f * (a + g);  // :162, double 0.5 * float sum: exact halving
    if (OP == 5) {                       // :145-146, pow() and 0.5 in double
        const double ad = (double)a, gd = (double)g;
        const float ms = (float)(0.5 * (ad * ad + gd * gd));
        return __builtin_sqrtf(ms);  // == (float)sqrt((double)ms): 53 >= 2*24+2
    }
    return (a < g) ? g : a;  // std::max, :188
}

// (3d) FUSED: vote -> camera fusion -> arg-max over Z without the DSIs ever leaving the CU.
//
// What "evaluateDSI x n; fused = op(dsi_0, dsi_1); collapseMaxZSlice(fused)" (process1.cpp:76-166 + :222
// -> mapper_emvs_stereo.cpp:368) computes, for callers that keep only the depth map (the 50 ms window
// loop of main.cpp:177-302): at 512 x 512 x 200 a window writes 2 x 210 MB of camera DSIs only for the
// arg-max to read them straight back.  Here a persistent workgroup owns a contiguous range of
// (band, plane) pairs; for each pair it votes camera 0's events into the band in LDS, reads the
// owned rows back as fp32 into REGISTERS (one value per thread and 1024-voxel stretch; <= 20 of them),
// clears the band, votes camera 1, applies the 2-ary op per voxel (fuse_op, the function the value Fuse2
// hands to k_voxelwise and k_collapse_max_z: same bits) and keeps a running (maximum, first index) per pixel in
// registers.  When its range leaves a band (and at the end) the running maxima go to one 64-bit key
// per pixel -- confidence bits << 8 | 255 - plane, the key of the plane-sharded arg-max -- with a
// global atomic MAX, which is collapseMaxZSlice's first-maximum-wins over the plane ranges of all
// workgroups; k_unpack_argmax turns the keys into confidence / index / depth.
//
// A band cannot wait for the band above to hand over its carry row here, so the band keeps a HALO row
// on either side of its owned rows [r0, r1) (LDS row 0 = grid row r0 - 1) and processes the events
// with floor(Y) in [r0 - 1, r1 - 1]: the events of the two seam rows are voted by both neighbours
// (1 / band_rows more votes), the halo rows collect the halves that belong to the neighbours and are
// dropped.  The owned rows then hold the exact 64-bit sums, which is what k_seam_rows reconstructs
// for the unfused path: both paths round the same integers once, so their depth maps are bit-equal.
template <int CELLS>
struct FusedBest {
    float best[CELLS];
    uint32_t idx4[(CELLS + 3) / 4];  // plane indices, four per register
};

// Read the band's owned rows back (one value per thread and 1024-cell stretch), zero the band, and either keep
// the fp32 values (camera 0 of 2) or fuse them with camera 0's and update the running arg-max.  Written without
// control flow per cell -- out-of-range lanes read the last owned cell and "zero" a halo cell that is zeroed
// anyway -- so that the CELLS / 2 LDS reads of a half are in flight together: with a branch per cell every
// read was waited for on its own, and the read-back took 3 us per phase (tools/fused_trace.py).
// MODE: what a phase does with the band it has just voted
enum { FUSED_LAST4 = 6,  // camera 3 of 4: sqrt(sqrt(c0 c1) * sqrt(c2 c3)) -- the GM tree's root (cartesian3dgrid.h:150-156), arg-max
       FUSED_READ1 = 5,  // camera 1 of 2, round 6: read back, clear and convert only -- values kept in vb; the fusion op and the
                         // running arg-max (the VALU-bound two thirds of that read-back) are DEFERRED to fused_deferred_argmax,
                         // which every wave runs at the end of ITS OWN next voting stream, while the other waves still vote
       FUSED_KEEP = 0,   // camera 0 of several: keep the values
       FUSED_MID = 1,    // camera 1 of 3: the two-camera op, result kept (process1.cpp:126-158)
       FUSED_LAST2 = 2,  // camera 1 of 2: the two-camera op, then the running arg-max
       FUSED_LAST1 = 3,  // the only camera: arg-max of its own values
       FUSED_LAST3 = 4 };// camera 2 of 3: the third-camera op (process1.cpp:169-191: 1 min, 2 HM with n = 3, 6 max), arg-max
// the deferred half of camera 1's read-back (two cameras): process1.cpp:126-158 on the values of both cameras, then the
// running first maximum (cartesian3dgrid.cpp:132-134) -- registers only, no LDS, no barrier
template <int CELLS, int OP>
__device__ __forceinline__ void fused_deferred_argmax(const float* __restrict__ va, const float* __restrict__ vb,
                                                      FusedBest<CELLS>& fb, int z)
{
#pragma unroll
    for (int kk = 0; kk < CELLS; ++kk) {
        const float f = fuse_op<OP>(0.f + va[kk], vb[kk]);
        const bool better = fb.best[kk] < f;
        fb.best[kk] = better ? f : fb.best[kk];
        const int sh = (kk & 3) * 8;
        const uint32_t with_z = (fb.idx4[kk >> 2] & ~(0xffu << sh)) | ((uint32_t)z << sh);
        fb.idx4[kk >> 2] = better ? with_z : fb.idx4[kk >> 2];
    }
}

// The read-back itself, shared by every consumer of a voted band: the owned cells read in parts of HALF (the reads of a
// part in flight together), zeroed, converted (one rounding, the wide conversion decided per wave) and handed to
// cell(kk, v) in cell order; then the two halo rows are cleared.
template <int CELLS, int HALF, typename Cell>
__device__ __forceinline__ void fused_readback(acc_t* __restrict__ band, int nx, int n_own, int rows_lds, Cell&& cell)
{
    acc_t* own = band + nx;
    // (the thread index is re-read behind an opaque barrier so that the compiler recomputes the 20 cell
    //  addresses per call instead of keeping them -- 60 registers of loop invariants -- alive across
    //  the voting loops, which name 40 physical registers themselves)
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    static_assert(CELLS % 2 == 0 && CELLS % HALF == 0, "whole parts");
#pragma unroll
    for (int h = 0; h < CELLS; h += HALF) {
        acc_t raw[HALF];
#pragma unroll
        for (int k = 0; k < HALF; ++k) raw[k] = own[min(t + (h + k) * 1024, n_own - 1)];
        uint32_t hi_or = 0;
#pragma unroll
        for (int k = 0; k < HALF; ++k) hi_or |= (uint32_t)(raw[k] >> 32);
#pragma unroll
        for (int k = 0; k < HALF; ++k) {
            const int i = t + (h + k) * 1024;
            acc_t* c = i < n_own ? own + i : band;  // band[0]: first halo row, cleared below
            *c = 0;
        }
        // sums of 2^52 and more (2 M votes in one voxel) take the wide conversion: decided per wave, then per lane
        const bool big = __builtin_amdgcn_ballot_w64((hi_or >> 20) != 0u) != 0ull;
#pragma unroll
        for (int k = 0; k < HALF; ++k) cell(h + k, big ? fix_to_float_any(raw[k]) : fix_to_float_narrow(raw[k]));
    }
    acc_t* last = band + (size_t)(rows_lds - 1) * nx;
    for (int i = threadIdx.x; i < nx; i += 1024) {
        band[i] = 0;
        last[i] = 0;
    }
}

template <int CELLS, int OP, int MODE>
__device__ __forceinline__ void fused_consume(acc_t* __restrict__ band, int nx, int n_own, int rows_lds,
                                              float* __restrict__ va, FusedBest<CELLS>& fb, int z,
                                              const float* __restrict__ vpair = nullptr /* FUSED_LAST4: cameras 2's values */)
{
    // cells read back together.  With camera 1's values parked in a second register array (DEFER) the kernel has ~20
    // registers fewer for the reads in flight: quarters instead of halves there
    constexpr int HALF = (MODE == FUSED_READ1 || (MODE == FUSED_KEEP && CELLS % 4 == 0 && CELLS == 20)) ? CELLS / 4 : CELLS / 2;
    fused_readback<CELLS, HALF>(band, nx, n_own, rows_lds, [&](int kk, float v) {
        if (MODE == FUSED_KEEP || MODE == FUSED_READ1) {
            va[kk] = v;
        } else if (MODE == FUSED_MID) {
            va[kk] = fuse_op<OP>(0.f + va[kk], v);
        } else {
            // process1.cpp:126-158: fused = 0; fused += dsi0; fused.<op>TwoGrids(dsi1)
            // process1.cpp:169-191: fused.minTwoGrids / harmonicMeanTwoGrids(dsi2, 3) / maxTwoGrids(dsi2)
            // (FUSED_LAST4: gm_tree<4> of the value GmTree -- t0 = va = sqrt(c0 c1), t1 = sqrt(c2 c3), sqrt(t0 t1))
            const float f = MODE == FUSED_LAST2   ? fuse_op<OP>(0.f + va[kk], v)
                            : MODE == FUSED_LAST3 ? (OP == 2 ? harmonic_mean_n(va[kk], v, 3.f, 2.f) : fuse_op<OP>(va[kk], v))
                            : MODE == FUSED_LAST4 ? fuse_op<3>(va[kk], fuse_op<3>(vpair[kk], v))
                                                  : v;
            const bool better = fb.best[kk] < f;  // strict: the first maximum wins (cartesian3dgrid.cpp:132-134)
            fb.best[kk] = better ? f : fb.best[kk];
            const int sh = (kk & 3) * 8;
            const uint32_t with_z = (fb.idx4[kk >> 2] & ~(0xffu << sh)) | ((uint32_t)z << sh);
            fb.idx4[kk >> 2] = better ? with_z : fb.idx4[kk >> 2];
        }
    });
}

// DEFER (round 6, the one-workgroup-per-CU kernel with the packed stream): with two cameras, camera 1's read-back only
// reads, clears and converts (FUSED_READ1); its fusion op and arg-max update -- ~60 % of that read-back's vector
// instructions, the IEEE division of the harmonic mean among them -- are run by every wave at the end of its NEXT voting
// stream, i.e. in the time it would otherwise wait at the phase barrier for the slowest wave (the waves of a phase end
// up to one pass = 2-4 us apart), while the others still vote.  Same values, same order per cell: same bits.
// FOUR (round 6): four cameras fused by the balanced tree of the reference's 2-ary geometric mean (DSI_ACC_GM_TREE,
// cartesian3dgrid.h:150-156 applied pairwise: BASELINE configs[4]) -- camera 0 kept, camera 1 folded into it, camera 2 kept in
// a second register array, camera 3 closes both pairs and the root; same bits as k_collapse_max_z<GmTree<4>, 2> on the four DSIs.
template <int MAPPING, int CELLS, bool DEFER = false, bool FOUR = false, bool DEAL = true>
__device__ __forceinline__ void vote_fuse_argmax_body(const FusedCameras& cams, const Geom& g, const BandPlan& bp, int op,
                                                      const uint32_t* __restrict__ splits,
                                                      unsigned long long* __restrict__ keys,
                                                      unsigned long long* __restrict__ trace)
{
    constexpr int BLOCK = 1024;
    extern __shared__ acc_t band[];
    __shared__ int s_pass;  // the next pass of the item to hand out
    // (the vector fill pre-assigns two units = one pass per wave, the dealt packed stream two passes)
    constexpr int kPass0 = 2 * (BLOCK / kWave);
    const int nx = g.nx;
    // Workgroup b runs on XCD b % 8: each XCD gets one contiguous eighth of the (band-major) pair list,
    // so that a band's records stream through at most two XCDs' L2s, and splits it evenly over its
    // workgroups -- or by `splits` (gridDim.x + 1 pair indices in XCD-major workgroup order) when
    // k_fused_splits has balanced the partition by the records each pair holds.
    const int P = bp.bands * g.nz;
    int q_begin, q_end, q_step = 1;
#ifdef DSI_TIMING_EXPERIMENTS
    // test hook dsi_test_fused_solo (experiments flavour only): bp.experiment 310 + k -- ONE workgroup, launched alone
    // (gridDim.x == 1, so `per` is 0), acts as workgroup 0 of XCD k of the dealt mode: it begins at pair P k / 8, draws that
    // pair once more, runs to the end of the list, wraps to pair 0 and ends at P k / 8 - 1 -- a draw order that is the same
    // on every run and descends inside a band at the wrap
    const unsigned wg = (bp.experiment >= 310 && bp.experiment < 318) ? (unsigned)(bp.experiment - 310) : blockIdx.x;
#else
    const unsigned wg = blockIdx.x;
#endif
    // DEALT (bp.interleave == 2, round 6): as "in turn", but only a workgroup's FIRST pair is fixed; every further pair is drawn
    // from its XCD's counter (one global atomic per pair, by thread 0, while the other waves finish camera 0's stream), and a
    // workgroup whose XCD has run dry draws from the next XCD's counter.  The pairs a workgroup draws from ONE counter ascend
    // (few band changes), the workgroups of an XCD still share one band's records at a time, and the kernel no
    // longer lasts as long as the workgroup whose FIXED share was the slowest (span / mean busy time 1.11 with fixed
    // shares: the dense middle bands are slow per record).  Across counters the pairs do NOT ascend: a workgroup whose XCD
    // is dry moves on to XCD (xcd + tries) & 7, round the ring, and may be handed a LOWER plane of the band it is in (any
    // two neighbouring stretches share a band when bands < 8; the straggler may be any XCD, not only 0 after 7).  The
    // running first maximum is a strict compare and needs ascending planes, so the pair loop keeps this invariant: z ascends
    // between two emits, or the band is re-opened (emit + reset, as at a band change; the keys' atomic MAX then takes the
    // first maximum over the pieces).  With it, which workgroup votes a pair -- and in which order -- changes no bit.
    // Counters: 8 words behind the keys, zero at launch (k_unpack_argmax re-zeroes them with the keys).
    // (DEAL = false: the two-workgroups-per-CU kernel, at 64 registers, takes its pairs in turn instead)
    const bool dealt = DEAL && !splits && bp.interleave == 2;
    __shared__ int s_next_q[2];
    __shared__ int s_deal_tries;
    if (splits) {
        // rank = position of this workgroup in XCD-major order: XCD x still covers one contiguous stretch
        const int rank = (int)(wg & 7) * (int)(gridDim.x >> 3) + (int)(wg >> 3);
        q_begin = (int)splits[rank];
        q_end = (int)splits[rank + 1];
    } else {
        const int x = wg & 7, l = wg >> 3, per = gridDim.x >> 3;
        const int lo = (int)(((long long)P * x) / 8), hi = (int)(((long long)P * (x + 1)) / 8);
        if (dealt) {
            q_begin = lo + l;
            q_end = hi;
        } else if (bp.interleave) {
            // the XCD's workgroups take the pairs of its stretch in turn: 32 workgroups on 32 consecutive planes of ONE band at a
            // time, so that the band's records (all cameras') stay in that XCD's L2 while they are read once per plane --
            // with contiguous pieces 32 workgroups work on ~9 bands at once at 1024 x 1024 x 256 (four cameras x 375 KB each:
            // 13 MB against 4 MB of L2, 4.6 TB/s from the Infinity Cache).  A workgroup then meets a band change every
            // nz / 32 pairs (one atomicMax per owned pixel each: microseconds).
            q_begin = lo + l;
            q_end = hi;
            q_step = per;
        } else {
        q_begin = lo + (int)(((long long)(hi - lo) * l) / per);
        q_end = lo + (int)(((long long)(hi - lo) * (l + 1)) / per);
        }
    }
    if (q_begin >= q_end) return;
    {
        const int all_cells = (bp.band_rows + 2) * nx;
        for (int i = threadIdx.x; i < all_cells; i += BLOCK) band[i] = 0;
        if (threadIdx.x == 0) {
            s_pass = kPass0;
            s_deal_tries = 0;
        }
    }
    __syncthreads();
    if (dealt) q_end = P;  // (a drawn pair may lie in another XCD's stretch; "none" is beyond every pair)

    // The cameras' table is read where it lies, in the kernel-argument segment, with scalar loads at the (uniform)
    // camera index: indexing the by-value array dynamically made the compiler keep all three cameras' pointers in
    // registers next to the ~40 the voting loops name (or copy the table to scratch).  `cams` is the FIRST argument,
    // so cam[0] starts the segment.
    // (layout lock: dsi_kernels.h, next to FusedCameras)
    typedef const FusedCamera __attribute__((address_space(4))) * KernargCameras;
    const KernargCameras kcam = (KernargCameras)__builtin_amdgcn_kernarg_segment_ptr();
    auto camera = [&](int c) -> FusedCamera {
        FusedCamera o;
        o.sxy = kcam[c].sxy;
        o.coef = kcam[c].coef;
        o.cuts = kcam[c].cuts;
        o.slow_any = kcam[c].slow_any;
        o.np = kcam[c].np;
        return o;
    };
    float va[CELLS];
    static_assert(!(DEFER && FOUR), "one use of the second register array");
    float vb[(DEFER || FOUR) ? CELLS : 1];  // DEFER: camera 1's values of the pair whose arg-max update is pending; FOUR: camera 2's
    int pend_z = -1;              // its plane (wave-uniform); -1: nothing pending
    FusedBest<CELLS> fb;
    auto run_pending = [&]() {
        if (!DEFER || pend_z < 0) return;
        switch (op) {
        case 1: fused_deferred_argmax<CELLS, 1>(va, vb, fb, pend_z); break;
        case 2: fused_deferred_argmax<CELLS, 2>(va, vb, fb, pend_z); break;
        case 3: fused_deferred_argmax<CELLS, 3>(va, vb, fb, pend_z); break;
        case 4: fused_deferred_argmax<CELLS, 4>(va, vb, fb, pend_z); break;
        case 5: fused_deferred_argmax<CELLS, 5>(va, vb, fb, pend_z); break;
        default: fused_deferred_argmax<CELLS, 6>(va, vb, fb, pend_z); break;
        }
        pend_z = -1;
    };
    int cur_j = -1, prev_z = -1, r0 = 0, r1 = 0, n_own = 0;
    // the cut words of this wave's first pass of phase (pair q, camera c) -- see packed_stream_asm_dealt
    constexpr bool kPrefetchCuts = MAPPING == 1;
    auto first_cuts_of = [&](int q, int c) -> uint32_t {
        if (!kPrefetchCuts) return 0u;
        const FusedCamera cam = camera(c);
        if (cam.np <= 0) return 0u;
        const int j = q / g.nz, z = q - j * g.nz;
        int lg = cam.np >= (BLOCK / kWave) * 16 ? 3 : 2;  // (the rule of stream_item's dealt stream)
        while (lg < 5 && cam.np >= (((BLOCK / kWave) * 16) << (lg + 1))) ++lg;
        if (bp.pass_lg > 0) lg = bp.pass_lg;
        const int p = min((int)((threadIdx.x / kWave) << lg) + (int)(threadIdx.x & 63), cam.np - 1);
        return cam.cuts[((size_t)j * g.nz + z) * cam.np + p];
    };
    uint32_t cuts_next = first_cuts_of(q_begin, 0);
    auto emit = [&]() {
        // one key per owned pixel (the owned rows are contiguous in the image)
        unsigned long long* kp = keys + (size_t)r0 * nx;
        int t = (int)threadIdx.x;
        asm volatile("" : "+v"(t));  // see fused_consume
#pragma unroll
        for (int k = 0; k < CELLS; ++k) {
            const int i = t + k * 1024;
            if (i < n_own) {
                const uint32_t zi = (fb.idx4[k >> 2] >> ((k & 3) * 8)) & 0xffu;
                const unsigned long long key = ((unsigned long long)__float_as_uint(fb.best[k]) << 8) | (255u - zi);
                atomicMax(kp + i, key);
            }
        }
    };
    int it = 0;  // pairs this workgroup has begun
    for (int q = q_begin; q < q_end; ++it) {
        const int j = q / g.nz, z = q - j * g.nz;
        int q_next = q + q_step;  // (DEALT: read from s_next_q behind the last phase's first barrier)
        // a band change -- or a pair that does not ascend within the band (DEALT: drawn from another XCD's counter), which
        // re-opens the band: the strict compare below keeps the FIRST maximum only while z ascends
        if (j != cur_j || z <= prev_z) {
            run_pending();  // (the last pair of the band that ends here)
            if (cur_j >= 0) emit();
            cur_j = j;
            r0 = j * bp.band_rows;
            r1 = min(g.ny, r0 + bp.band_rows);
            n_own = (r1 - r0) * nx;
#pragma unroll
            for (int k = 0; k < CELLS; ++k) fb.best[k] = -1.f;  // below every DSI value (>= 0)
#pragma unroll
            for (int k = 0; k < (CELLS + 3) / 4; ++k) fb.idx4[k] = 0u;
        }
        prev_z = z;
        const int rows_lds = r1 - r0 + 2;
        // events with floor(Y) in [r0 - 1, r1 - 1] (and in [0, ny - 2], cartesian3dgrid.h:255-259)
        const int Li = max(r0 - 1, 0), Ui = min(r1, g.ny - 1);
        // (the DEFER instantiation is launched for two cameras only: the other camera counts' read-backs are not in it)
        const int n_cams = DEFER ? 2 : (FOUR ? 4 : cams.n);
#pragma nounroll
        for (int c = 0; c < n_cams; ++c) {
            const FusedCamera cam = camera(c);
#ifdef DSI_TIMING_EXPERIMENTS
            // development aid (experiments flavour only, dsi_test_fused_trace_*): 100 MHz time stamps per (workgroup,
            // phase, wave): stream begins, stream ends, after the barrier + the read-back / clear, after the closing barrier
            int tr = -1;  // (wave-uniform: lives in a scalar register)
            if (trace) {
                const int phase = it * cams.n + c;
                if (phase < kFusedTracePhases)
                    tr = __builtin_amdgcn_readfirstlane((((int)wg * kFusedTracePhases + phase) * (BLOCK / kWave) + (int)(threadIdx.x / kWave)) * 4);
            }
#define DSI_FUSED_STAMP(k) do { if (tr >= 0 && (threadIdx.x & 63) == 0) trace[tr + (k)] = wall_clock64(); } while (0)
#else
#define DSI_FUSED_STAMP(k) do { } while (0)
#endif
            DSI_FUSED_STAMP(0);
            const uint32_t cuts_now = cuts_next;
            stream_item<BLOCK, MAPPING, true, true>(cam.sxy, cam.coef, cam.cuts, cam.slow_any, cam.np, g, bp, j, z, 0, cam.np,
                                        reinterpret_cast<char*>(band), Li, Ui, r0 - 1, &s_pass, cuts_now);
            // the next phase's first cut words travel during this phase's barrier and read-back
            const bool last = c == n_cams - 1;
            if (c + 1 < n_cams)
                cuts_next = first_cuts_of(q, c + 1);
            else if (!dealt && q + q_step < q_end)
                cuts_next = first_cuts_of(q + q_step, 0);
            run_pending();  // the previous pair's fusion + arg-max update, while the other waves finish their passes
            if (dealt && c == 0 && __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) {
                // the next pair of this workgroup: its XCD's counter first, then the other XCDs' in turn (the first `per`
                // pairs of every stretch are the workgroups' fixed first pairs).  Wave 0, scalar code but for the atomic.
                // (P < 2^24: at most 2^16 rows -- 16-bit row tables -- and 256 planes -- 8-bit plane indices in the keys)
                const int xcd = (int)(wg & 7), per = (int)(gridDim.x >> 3);
                unsigned* const ctr = reinterpret_cast<unsigned*>(keys + (size_t)g.nx * g.ny);
                int tries = __builtin_amdgcn_readfirstlane(s_deal_tries);  // XCDs this workgroup has found dry
                int nq = 0x7fffffff;
                while (tries < 8) {
                    const int xx = (xcd + tries) & 7;
                    unsigned got = 0u;
                    if ((threadIdx.x & 63) == 0) got = atomicAdd(&ctr[xx], 1u);
                    const int cand = (P * xx) / 8 + per + (int)__builtin_amdgcn_readfirstlane(got);
                    if (cand < (P * (xx + 1)) / 8) {
                        nq = cand;
                        break;
                    }
                    ++tries;
                }
                if ((threadIdx.x & 63) == 0) {
                    s_deal_tries = tries;
                    s_next_q[it & 1] = nq;
                }
            }
            DSI_FUSED_STAMP(1);
            __syncthreads();
            if (threadIdx.x == 0) s_pass = kPass0;
            if (dealt && last) {
                // (written before the first barrier of this pair's camera-0 phase; slot it & 1 is next written two pairs on)
                q_next = __builtin_amdgcn_readfirstlane(s_next_q[it & 1]);
                if (q_next < P) cuts_next = first_cuts_of(q_next, 0);
            }
            if constexpr (FOUR) {
                if (c == 0)
                    fused_consume<CELLS, 3, FUSED_KEEP>(band, nx, n_own, rows_lds, va, fb, z);
                else if (c == 1)
                    fused_consume<CELLS, 3, FUSED_MID>(band, nx, n_own, rows_lds, va, fb, z);
                else if (c == 2)
                    fused_consume<CELLS, 3, FUSED_KEEP>(band, nx, n_own, rows_lds, vb, fb, z);
                else
                    fused_consume<CELLS, 3, FUSED_LAST4>(band, nx, n_own, rows_lds, va, fb, z, vb);
            } else if constexpr (DEFER) {
                if (!last) {
                    fused_consume<CELLS, 1, FUSED_KEEP>(band, nx, n_own, rows_lds, va, fb, z);
                } else {
                    fused_consume<CELLS, 1, FUSED_READ1>(band, nx, n_own, rows_lds, vb, fb, z);
                    pend_z = z;
                }
            } else if (!last) {
                if (c == 0) {
                    fused_consume<CELLS, 1, FUSED_KEEP>(band, nx, n_own, rows_lds, va, fb, z);
                } else {  // camera 1 of 3: only the ops whose third step exists get here (1, 2, 6)
                    switch (op) {
                    case 1: fused_consume<CELLS, 1, FUSED_MID>(band, nx, n_own, rows_lds, va, fb, z); break;
                    case 2: fused_consume<CELLS, 2, FUSED_MID>(band, nx, n_own, rows_lds, va, fb, z); break;
                    default: fused_consume<CELLS, 6, FUSED_MID>(band, nx, n_own, rows_lds, va, fb, z); break;
                    }
                }
            } else if (cams.n == 1) {
                fused_consume<CELLS, 1, FUSED_LAST1>(band, nx, n_own, rows_lds, va, fb, z);
            } else if (cams.n == 2) {
                switch (op) {
                case 1: fused_consume<CELLS, 1, FUSED_LAST2>(band, nx, n_own, rows_lds, va, fb, z); break;
                case 2: fused_consume<CELLS, 2, FUSED_LAST2>(band, nx, n_own, rows_lds, va, fb, z); break;
                case 3: fused_consume<CELLS, 3, FUSED_LAST2>(band, nx, n_own, rows_lds, va, fb, z); break;
                case 4: fused_consume<CELLS, 4, FUSED_LAST2>(band, nx, n_own, rows_lds, va, fb, z); break;
                case 5: fused_consume<CELLS, 5, FUSED_LAST2>(band, nx, n_own, rows_lds, va, fb, z); break;
                default: fused_consume<CELLS, 6, FUSED_LAST2>(band, nx, n_own, rows_lds, va, fb, z); break;
                }
            } else {
                switch (op) {
                case 1: fused_consume<CELLS, 1, FUSED_LAST3>(band, nx, n_own, rows_lds, va, fb, z); break;
                case 2: fused_consume<CELLS, 2, FUSED_LAST3>(band, nx, n_own, rows_lds, va, fb, z); break;
                default: fused_consume<CELLS, 6, FUSED_LAST3>(band, nx, n_own, rows_lds, va, fb, z); break;
                }
            }
            DSI_FUSED_STAMP(2);
            __syncthreads();
            DSI_FUSED_STAMP(3);
        }
        q = q_next;
    }
    run_pending();
    emit();
#undef DSI_FUSED_STAMP
}

// one workgroup per CU: the band takes (almost) the whole LDS, up to 128 VGPRs
template <int MAPPING, int CELLS, bool DEFER = false, bool FOUR = false>
__global__ __launch_bounds__(1024) void k_vote_fuse_argmax(FusedCameras cams, Geom g, BandPlan bp, int op,
                                                           const uint32_t* __restrict__ splits,
                                                           unsigned long long* __restrict__ keys,
                                                           unsigned long long* __restrict__ trace)
{
    vote_fuse_argmax_body<MAPPING, CELLS, DEFER, FOUR>(cams, g, bp, op, splits, keys, trace);
}

// TWO workgroups per CU (round 4): bands of at most half the LDS, half the cells per thread, <= 64 VGPRs -- while one
// workgroup's 16 waves stand at a phase barrier or read a band back, the other's vote.  Same body, same bits.
// (`cams` stays the FIRST parameter: the body reads the camera table from the start of the kernel-argument segment.)
template <int MAPPING, int CELLS>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_vote_fuse_argmax_2cu(
    FusedCameras cams, Geom g, BandPlan bp, int op, const uint32_t* __restrict__ splits,
    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ trace)
{
    vote_fuse_argmax_body<MAPPING, CELLS, false, false, false>(cams, g, bp, op, splits, keys, trace);
}

// Balanced partition of the (band-major) pair list for the fused kernel: pair q costs work0[q] + work1[q]
// records (counted by k_plane_coef from the runs the voting loop will walk) plus a fixed cost per pair (the
// set-up, barriers and read-back of its phases, in record units); the n_wg + 1 split points cut the list
// into stretches of equal cost.  One block; P <= 1024 * kSplitSlice pairs.
constexpr int kSplitSlice = 64;

__global__ __launch_bounds__(1024) void k_fused_splits(const uint32_t* __restrict__ work0, const uint32_t* __restrict__ work1,
                                                       int P, uint32_t fixed_per_pair, int n_wg,
                                                       unsigned long long* __restrict__ prefix /* [P] scratch */,
                                                       uint32_t* __restrict__ splits)
{
    __shared__ unsigned long long wave_tot[16];
    const int per = (P + 1023) / 1024;
    const int b0 = min(P, (int)threadIdx.x * per), b1 = min(P, b0 + per);
    unsigned long long local = 0;
    for (int i = b0; i < b1; ++i) local += (unsigned long long)work0[i] + (work1 ? work1[i] : 0u) + fixed_per_pair;
    unsigned long long incl = local;
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned long long base = incl - local, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < (int)(threadIdx.x >> 6)) base += wave_tot[w];
        total += wave_tot[w];
    }
    for (int i = b0; i < b1; ++i) {
        base += (unsigned long long)work0[i] + (work1 ? work1[i] : 0u) + fixed_per_pair;
        prefix[i] = base;  // cost of pairs 0 .. i
    }
    __syncthreads();
    for (int r = threadIdx.x; r <= n_wg; r += 1024) {
        // first pair index whose inclusive prefix reaches r / n_wg of the total: that many pairs lie before the cut
        const unsigned long long target = (total * (unsigned long long)r + (unsigned long long)n_wg - 1) / (unsigned long long)n_wg;
        int lo = 0, hi = P;  // smallest i in [0, P] with (i == P or prefix[i] >= target) -> pairs [0, i] ... cut after i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] >= target) hi = mid; else lo = mid + 1;
        }
        // pairs before the r-th cut: those whose inclusive prefix is <= target (so that the last cut takes all)
        int cut = (r == 0) ? 0 : (r == n_wg ? P : min(P, lo + 1));
        splits[r] = (uint32_t)cut;
    }
}

// (3c) GROUPED mapping: S consecutive packets (a "group"; their poses are microseconds apart)
//     are sorted TOGETHER by z0 row, every event keeping its packet's index within the group.
//     The events a band needs from the whole group are then one long contiguous run (the
//     union of the S packets' row ranges), so a wave walks a few hundred events per run with
//     a plain loop -- almost no scalar bookkeeping per batch (the CU's one-per-clock scalar
//     unit is what limits the packed mapping) -- and fetches each lane's coefficients with a
//     gather that stays inside a 32*S-byte window of the plane-major table.
__global__ __launch_bounds__(256) void k_sort_groups(const float2* __restrict__ xy, int np, int S,
                                                     int ny, int nz, int pad, EvRec* __restrict__ sxy,
                                                     uint8_t* __restrict__ spk,
                                                     uint32_t* __restrict__ nvalid,
                                                     uint16_t* __restrict__ rowstart)
{
    extern __shared__ uint32_t hist[];  // nb + 1 counters -> exclusive offsets -> running cursors
    __shared__ uint32_t wave_tot[4];
    const int nb = ny + 2 * pad + 2;
    const int gidx = blockIdx.x;
    const int p0 = gidx * S;
    const int n_ev = min(S, np - p0) * kPacket;
    const float2* __restrict__ src = xy + (size_t)p0 * kPacket;
    if (gidx == 0) {
        for (int i = threadIdx.x; i < nz + 8; i += 256) nvalid[np + i] = 0;  // see k_sort_packets
        if (threadIdx.x == 0) {
            const EvRec none = {0.f, 0.f, 0u};
            sxy[(size_t)np * kPacket] = none;  // the multiplicity-0 record
        }
    }
    for (int i = threadIdx.x; i <= nb; i += 256) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n_ev; i += 256) {
        const float2 e = src[i];
        if (finitef(e.x) && finitef(e.y)) atomicAdd(&hist[row_bin(e.y, ny, pad)], 1u);
    }
    __syncthreads();
    const int per = (nb + 255) / 256;
    const int b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    uint32_t local = 0;
    for (int i = b0; i < b1; ++i) local += hist[i];
    uint32_t incl = local;
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - local;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) base += wave_tot[w];
    const uint32_t total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
    for (int i = b0; i < b1; ++i) {
        const uint32_t c = hist[i];
        hist[i] = base;
        base += c;
    }
    if (threadIdx.x == 0) hist[nb] = total;
    __syncthreads();
    uint16_t* rs = rowstart + (size_t)gidx * (nb + 1);
    for (int i = threadIdx.x; i <= nb; i += 256) rs[i] = (uint16_t)hist[i];  // S*1024 <= 32768
    __syncthreads();
    EvRec* __restrict__ dst = sxy + (size_t)p0 * kPacket;
    uint8_t* __restrict__ dpk = spk + (size_t)p0 * kPacket;
    for (int i = threadIdx.x; i < n_ev; i += 256) {
        const float2 e = src[i];
        if (finitef(e.x) && finitef(e.y)) {
            const uint32_t pos = atomicAdd(&hist[row_bin(e.y, ny, pad)], 1u);
            // multiplicity 1 in the low half, packet index within the group in the high half (the
            // hand-scheduled loop finds the record's coefficients through it)
            const EvRec r = {e.x, e.y, 1u | ((uint32_t)(i >> 10) << 16)};
            dst[pos] = r;
            dpk[pos] = (uint8_t)(i >> 10);  // packet index within the group
        }
    }
    if (threadIdx.x == 0) nvalid[gidx] = total;
}

// union of the row-bin ranges of a group's packets -> the run [lo, hi) of the group
__global__ __launch_bounds__(256) void k_group_cuts(const uint32_t* __restrict__ prow,
                                                    const uint16_t* __restrict__ rowstart, int np,
                                                    int ngroups, int S, int nz, int bands, int nb,
                                                    uint32_t* __restrict__ gcuts)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)ngroups * nz * bands;
    if (tid >= total) return;
    const int gidx = (int)(tid % ngroups);  // group fastest: coalesced writes
    const size_t jz = tid / ngroups;        // = band * nz + z
    const int p0 = gidx * S, p1 = min(np, p0 + S);
    uint32_t blo = 0xffffu, bhi = 0;
    const uint32_t* __restrict__ row = prow + jz * np;
    for (int p = p0; p < p1; ++p) {
        const uint32_t w = row[p];
        const uint32_t l = w & 0xffffu, h = w >> 16;
        if (l <= h && !(l == 0xffffu)) {
            blo = min(blo, l);
            bhi = max(bhi, h);
        }
    }
    uint32_t lo = 0, hi = 0;
    if (blo <= bhi && blo != 0xffffu) {
        const uint16_t* rs = rowstart + (size_t)gidx * (nb + 1);
        lo = rs[blo];
        hi = rs[bhi];
    }
    gcuts[jz * ngroups + gidx] = lo | (hi << 16);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_vote_groups(const EvRec* __restrict__ sxy,
                                                       const uint8_t* __restrict__ spk,
                                                       const PlaneCoef* __restrict__ coef,
                                                       const uint32_t* __restrict__ gcuts,
                                                       const uint32_t* __restrict__ slow_any, int np,
                                                       int ngroups, int S, Geom g, BandPlan bp,
                                                       void* __restrict__ out,
                                                       acc_t* __restrict__ seam)
{
    extern __shared__ acc_t band[];
    const int b = blockIdx.x;
    const int pairs = bp.chunks * bp.bands;
    int q, z;
    if (!item_of(b, pairs, g.nz, q, z, bp.experiment == 200)) return;
    const int c = q / bp.bands, j = q % bp.bands;
    const int r0 = j * bp.band_rows;
    const int r1 = min(g.ny, r0 + bp.band_rows);
    const int nx = g.nx;
    const int cells = (r1 - r0 + 1) * nx;  // owned rows + the carry row
    for (int i = threadIdx.x; i < cells; i += BLOCK) band[i] = 0;
    __syncthreads();

    const int g_begin = (int)(((long long)ngroups * c) / bp.chunks);
    const int g_end = (int)(((long long)ngroups * (c + 1)) / bp.chunks);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int lane = threadIdx.x & (kWave - 1);
    const int Li = r0, Ui = min(r1, g.ny - 1);
    const int row_base = r0;
    const uint4* __restrict__ coef4 = reinterpret_cast<const uint4*>(coef) + 2 * (size_t)z * np;
    const uint32_t* __restrict__ cutz = gcuts + ((size_t)j * g.nz + z) * ngroups;

    if (bp.packed == 4 && slow_any[z] == 0) {
        // lane mapping 4: the hand-scheduled stream over groups (runs of all the wave's groups
        // packed back to back into the lanes); planes that need the IEEE divide take the loop below
        constexpr int kWaves = BLOCK / kWave;
        int lg_pass = 6;
        while (lg_pass > 0 && (g_end - g_begin) < ((kWaves * 4) << lg_pass)) --lg_pass;
        if (bp.pass_lg > 0) lg_pass = bp.pass_lg;
        const int pass = 1 << lg_pass;
        group_stream_asm(sxy, coef4, cutz, reinterpret_cast<char*>(band), g_begin + wave * pass, g_end,
                         lg_pass, kWaves * pass, lane, nx, Li, Ui, row_base,
                         (uint32_t)np * (uint32_t)kPacket, S);
    } else
    for (int gi = g_begin + wave; gi < g_end; gi += BLOCK / kWave) {
        const uint32_t cu = cutz[gi];
        const int lo = (int)(cu & 0xffffu), hi = (int)(cu >> 16);
        if (lo >= hi) continue;
        const size_t ev0 = (size_t)gi * S * kPacket;
        const EvRec* __restrict__ ev = sxy + ev0;
        const uint8_t* __restrict__ pk = spk + ev0;
        const uint4* __restrict__ cg = coef4 + 2 * (size_t)gi * S;  // the group's coefficient window
        // Two batches per trip with two register sets (A, B): the gathers of batch b+1 (event +
        // coefficients, which need that batch's packet indices) and the packet indices of
        // batch b+2 are in flight while batch b is voted.  All loads are straight-line with
        // indices clamped into the run, so the compiler counts outstanding loads exactly and no
        // register copy waits for a load.
        auto vote_one = [&](EvRec e, uint4 va, uint2 vb, bool act) {
            const float ka = __uint_as_float(va.x), kbx = __uint_as_float(va.y);
            const float kby = __uint_as_float(va.z), kd = __uint_as_float(va.w);
            const float kr = __uint_as_float(vb.x);
            const float nxv = e.x * ka + kbx;  // mapper_emvs_stereo.cpp:194-195
            const float nyv = e.y * ka + kby;
            float X, Y, nmax;
            if (__builtin_amdgcn_ballot_w64((vb.y & kCoefSlow) != 0) != 0) {  // rare, whole wave
                X = nxv / kd;
                Y = nyv / kd;
                nmax = __builtin_inff();
            } else {
                X = div_rc(nxv, kd, kr);
                Y = div_rc(nyv, kd, kr);
                nmax = 1e30f;
            }
            // cartesian3dgrid.h:255-259 restricted to this band's rows as one integer test
            // (see k_vote_bands_packed); dead packets of the group carry kCoefSkip
            const float xf = __builtin_floorf(X), yf = __builtin_floorf(Y);
            const int xi = (int)xf, yi = (int)yf;
            int sgn = xi | (nx - 2 - xi) | (yi - Li) | (Ui - 1 - yi);
            sgn |= (act && !(vb.y & kCoefSkip) && fabsf(nxv) < nmax && fabsf(nyv) < nmax) ? 0 : -1;
            if (sgn >= 0) {
                const int idx = __mul24(yi - row_base, nx) + xi;
                vote4(band, idx, nx, X - xf, Y - yf, e.m & 0xffffu);  // cartesian3dgrid.h:261-270
            }
        };
        const int last = hi - 1;
        int i0 = lo + lane, i1 = i0 + kWave;
        int k0 = pk[min(i0, last)], k1 = pk[min(i1, last)];
        EvRec eA = ev[min(i0, last)], eB;
        uint4 vaA = cg[2 * k0], vaB;
        uint2 vbA = *reinterpret_cast<const uint2*>(cg + 2 * k0 + 1), vbB;
        for (int base = lo; base < hi; base += 2 * kWave) {
            // set B <- batch b+1, packet indices of b+2; vote batch b (set A)
            eB = ev[min(i1, last)];
            vaB = cg[2 * k1];
            vbB = *reinterpret_cast<const uint2*>(cg + 2 * k1 + 1);
            k0 = pk[min(i0 + 2 * kWave, last)];
            vote_one(eA, vaA, vbA, i0 < hi);
            // set A <- batch b+2, packet indices of b+3; vote batch b+1 (set B)
            eA = ev[min(i0 + 2 * kWave, last)];
            vaA = cg[2 * k0];
            vbA = *reinterpret_cast<const uint2*>(cg + 2 * k0 + 1);
            k1 = pk[min(i1 + 2 * kWave, last)];
            vote_one(eB, vaB, vbB, i1 < hi);
            i0 += 2 * kWave;
            i1 += 2 * kWave;
        }
    }
    __syncthreads();
    const size_t vol = partial_stride((size_t)g.nx * g.ny * g.nz);
    const size_t off = (size_t)c * vol + ((size_t)z * g.ny + r0) * nx;
    flush_band<BLOCK>(band, nx, (r1 - r0) * nx, out, off, bp.raw_out, seam_rows(seam, c, z, j, g, bp), j, bp.bands);
}

// (4) seam rows: the first row of band j >= 1 of every plane of every chunk's volume is the exact
// fixed-point sum of the band's own votes (head) and of the band above's votes into the row below
// it (carry), rounded to fp32 ONCE: out[c][z][j * band_rows][x] = fl((head + carry) * 2^-31).
// Runs after the voting kernel and before the chunk volumes are summed.
// block x = one (plane, seam) row, block y = a 512-voxel stretch of it, block z = chunk; two voxels
// per thread (16-byte loads, 8-byte stores) when nx is even
template <bool RAW>
__global__ __launch_bounds__(256) void k_seam_rows(const acc_t* __restrict__ seam, Geom g, int bands, int band_rows,
                                                   void* __restrict__ out, size_t vol_stride)
{
    const int j = (int)(blockIdx.x % (unsigned)(bands - 1)) + 1;
    const int z = (int)(blockIdx.x / (unsigned)(bands - 1));
    const int c = (int)blockIdx.z;
    const size_t row = ((size_t)c * g.nz + z) * bands;
    const acc_t* head = seam + ((row + j) * 2) * g.nx;
    const acc_t* carry = seam + ((row + j - 1) * 2 + 1) * g.nx;
    const size_t off = (size_t)c * vol_stride + ((size_t)z * g.ny + (size_t)j * band_rows) * g.nx;
    float* dstf = reinterpret_cast<float*>(out) + off;
    acc_t* dstr = reinterpret_cast<acc_t*>(out) + off;
    if ((g.nx & 1) == 0) {
        const int x = ((int)blockIdx.y * 256 + (int)threadIdx.x) * 2;
        if (x >= g.nx) return;
        const ulonglong2 h = *reinterpret_cast<const ulonglong2*>(head + x);
        const ulonglong2 k = *reinterpret_cast<const ulonglong2*>(carry + x);
        if (RAW) {
            *reinterpret_cast<ulonglong2*>(dstr + x) = make_ulonglong2(h.x + k.x, h.y + k.y);
        } else {
            float2 r;
            r.x = fix_to_float(h.x + k.x);  // one rounding to f32
            r.y = fix_to_float(h.y + k.y);
            *reinterpret_cast<float2*>(dstf + x) = r;
        }
    } else {
        for (int x = (int)blockIdx.y * 512 + (int)threadIdx.x; x < min(g.nx, ((int)blockIdx.y + 1) * 512); x += 256) {
            if (RAW)
                dstr[x] = head[x] + carry[x];
            else
                dstf[x] = fix_to_float(head[x] + carry[x]);
        }
    }
}

// (5) DSI = fl(sum over the chunks of their raw 64-bit partial volumes * 2^-31) [+ the grid's previous
// contents: fillVoxelGrid accumulates, mapper_emvs_stereo.cpp:151-205 has no reset]: the integer sum is
// exact and order-free, so the DSI does not depend on the number of chunks.  Two voxels per thread.
__global__ __launch_bounds__(256) void k_reduce_partials(const acc_t* __restrict__ partials,
                                                         int chunks, size_t n,
                                                         float* __restrict__ dsi, int accumulate,
                                                         const acc_t* __restrict__ seam, int nx, int ny, int nz, int bands,
                                                         int band_rows)
{
    // seam != nullptr: the seam rows (first row of every band but the first) are taken from the bands' head and
    // carry sums instead of the partial volumes (k_seam_rows folded in: one launch less per evaluateDSI);
    // requires an even nx (two voxels per thread never straddle a row)
    const size_t n2 = n / 2;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t vs = partial_stride(n);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        ulonglong2 acc = make_ulonglong2(0ull, 0ull);
        bool from_seam = false;
        if (seam) {
            const unsigned v = (unsigned)(2 * i);          // voxel index < 2^32 (checked by the launcher)
            const unsigned rowi = v / (unsigned)nx;        // z * ny + y
            const unsigned y = rowi % (unsigned)ny;
            const unsigned j = y / (unsigned)band_rows;
            if (j >= 1 && y == j * (unsigned)band_rows) {
                from_seam = true;
                const unsigned z = rowi / (unsigned)ny, x = v - rowi * (unsigned)nx;
                for (int c = 0; c < chunks; ++c) {
                    const size_t row = ((size_t)c * nz + z) * bands;
                    const ulonglong2 h = *reinterpret_cast<const ulonglong2*>(seam + ((row + j) * 2) * nx + x);
                    const ulonglong2 k = *reinterpret_cast<const ulonglong2*>(seam + ((row + j - 1) * 2 + 1) * nx + x);
                    acc.x += h.x + k.x;
                    acc.y += h.y + k.y;
                }
            }
        }
        if (!from_seam)
            for (int c = 0; c < chunks; ++c) {
                const ulonglong2 v = reinterpret_cast<const ulonglong2*>(partials + (size_t)c * vs)[i];
                acc.x += v.x;
                acc.y += v.y;
            }
        float2 r = make_float2(fix_to_float(acc.x), fix_to_float(acc.y));
        float2* d2 = reinterpret_cast<float2*>(dsi) + i;  // (grids are 16-byte aligned, also wrapped ones)
        if (accumulate) {
            const float2 old = *d2;
            r.x = old.x + r.x;
            r.y = old.y + r.y;
        }
        *d2 = r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
        const size_t i = n - 1;
        acc_t acc = 0;
        for (int c = 0; c < chunks; ++c) acc += partials[(size_t)c * vs + i];
        const float r = fix_to_float(acc);
        dsi[i] = accumulate ? dsi[i] + r : r;
    }
}

// ------------------------------------------------------------ Grid3D ops ---
// the per-voxel kinds of ew_op
enum { EW_HM_N = 0, EW_ADD = 1, EW_ADD_INV = 2, EW_FIN_AM = 3, EW_FIN_HM = 4,
       EW_ADD_LOG = 5, EW_ADD_SQ = 6, EW_MIN = 7, EW_MAX = 8, EW_FIN_GM = 9, EW_FIN_RMS = 10 };

// ---- n-ary geometric mean: exp(mean(log v)), 0 as soon as one factor is 0 (SURVEY 8d cfg 5).
// The reference only has the 2-ary sqrt(a*g) (cartesian3dgrid.h:150-156).  log and exp are
// spelled out in IEEE double operations (+, *, /, floor, bit moves, explicit fused multiply-adds;
// no libm, nothing fused implicitly: -ffp-contract=off) so that the CPU oracle, which repeats
// exactly this sequence, gets the same bits.
//
// log v = e ln2 + log c_i + log1p(r):  v = 2^e m, m in [1, 2); the top 7 mantissa bits pick
// c_i = 1 + (2 i + 1) / 256 (the centre of m's 1/128 interval), r = (m - c_i) / c_i with |r| <= 2^-8,
// log1p(r) by its degree-5 Taylor polynomial (next term r^6 / 6 < 6e-16).  {1 / c_i, log c_i} come
// from a 128-entry table in LDS that every block fills for itself with the division-based series
// below (full double accuracy; 128 threads x ~60 operations per block), so the per-voxel path has
// no division: ~25 instructions per log instead of ~60 (4-camera fusion at 1024 x 1024 x 256:
// 2.09 -> 1.37 ms, still bound by fp64 issue rather than by the 5.4 GB it streams).
// The absolute error of the log is ~1e-15; its fp32 rounding and the fp32 sum of logs
// dominate (the accumulator is a float grid).
__device__ __forceinline__ double det_log_series(double m)  // m in [1, 2); table set-up only
{
    double e = 0.0;
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e = 1.0;
    }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;  // <= 0.0295
    double p = 0.047619047619047616;         // 1/21
    p = p * z + 0.05263157894736842;         // 1/19
    p = p * z + 0.058823529411764705;        // 1/17
    p = p * z + 0.06666666666666667;         // 1/15
    p = p * z + 0.07692307692307693;         // 1/13
    p = p * z + 0.09090909090909091;         // 1/11
    p = p * z + 0.1111111111111111;          // 1/9
    p = p * z + 0.14285714285714285;         // 1/7
    p = p * z + 0.2;                         // 1/5
    p = p * z + 0.3333333333333333;          // 1/3
    p = p * z + 1.0;
    const double t1 = e * 0.6931471805599453;
    const double t2 = 2.0 * s;
    return t1 + t2 * p;
}

constexpr int kLogTabSize = 128;

__device__ __forceinline__ void det_log_table_fill(double2* tab)  // whole block; ends with a barrier
{
    for (int i = threadIdx.x; i < kLogTabSize; i += blockDim.x) {
        const double c = 1.0 + (double)(2 * i + 1) * 0.00390625;  // exact
        tab[i] = make_double2(1.0 / c, det_log_series(c));
    }
    __syncthreads();
}

__device__ __forceinline__ float det_logf(float v, const double2* __restrict__ tab)
{
    // (selects instead of early returns: the special cases are rare and a wave would take both
    //  sides anyway)
    const bool positive = v > 0.f, regular = positive && finitef(v);
    const double x = (double)(regular ? v : 1.f);  // every positive float is a normal double
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const int e = (int)((b >> 52) & 0x7ffull) - 1023;
    const unsigned i = (unsigned)(b >> 45) & 127u;
    const double m = __longlong_as_double((long long)((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull));
    const double c = __longlong_as_double((long long)(0x3ff0000000000000ull | ((unsigned long long)(2u * i + 1u) << 44)));
    const double2 t = tab[i];
    const double r = (m - c) * t.x;          // m - c is exact
    double p = __builtin_fma(r, 0.2, -0.25);  // fused multiply-adds, spelled out (IEEE 754 fma)
    p = __builtin_fma(p, r, 0.3333333333333333);
    p = __builtin_fma(p, r, -0.5);
    p = __builtin_fma(p, r, 1.0);
    p = p * r;
    const float res = (float)__builtin_fma((double)e, 0.6931471805599453, t.y + p);
    const float special = positive ? v /* +inf */ : (v == 0.f ? -__builtin_inff() : __builtin_nanf(""));
    return regular ? res : special;
}

// exp(y) rounded to float: y = k ln2 + r, |r| <= 0.347, degree-9 Taylor polynomial (next term
// r^10 / 10! < 7e-12 relative, far below the float rounding)
__device__ __forceinline__ float det_expf(double y)
{
    const bool regular = y >= -104.0 && y <= 89.0;  // false for NaN
    const float special = (y != y) ? __builtin_nanf("") : (y > 89.0 ? __builtin_inff() : 0.f);  // (-inf: a factor was 0)
    y = regular ? y : 0.0;
    const double kd = __builtin_floor(y * 1.4426950408889634 + 0.5);
    double r = __builtin_fma(kd, -0.6931471803691238, y);      // ln2 split as in fdlibm (hi part has 32 bits)
    r = __builtin_fma(kd, -1.9082149292705877e-10, r);
    double p = 2.7557319223985893e-06;           // 1/9!
    p = __builtin_fma(p, r, 2.48015873015873e-05);
    p = __builtin_fma(p, r, 0.0001984126984126984);
    p = __builtin_fma(p, r, 0.001388888888888889);
    p = __builtin_fma(p, r, 0.008333333333333333);
    p = __builtin_fma(p, r, 0.041666666666666664);
    p = __builtin_fma(p, r, 0.16666666666666666);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    const long long k = (long long)kd;           // |k| <= 151: 2^k is a normal double
    const double sc = __longlong_as_double((k + 1023) << 52);
    return regular ? (float)(p * sc) : special;
}

template <int KIND>
__device__ __forceinline__ float ew_op(float a, float g, float fn, float fn1, const double2* __restrict__ log_tab = nullptr)
{
    if (KIND == EW_HM_N) return harmonic_mean_n(a, g, fn, fn1);  // cartesian3dgrid.h:130-139
    if (KIND == EW_ADD) return a + g;                       // :68
    if (KIND == EW_ADD_INV) return a + 1.0f / (0.01f + g);  // :76, eps = 1e-2f
    if (KIND == EW_FIN_AM) return a / fn;                   // :91
    if (KIND == EW_FIN_HM) return fn / a;                   // :84
    // n-ary extensions of the 2-ary camera-fusion ops (cartesian3dgrid.h:111-190) in
    // accumulate / finalize form; sum-, min- and max-reducible across GPUs
    if (KIND == EW_ADD_LOG) return a + det_logf(g, log_tab);  // GM: sum of log v (-inf once a v is 0)
    if (KIND == EW_ADD_SQ) return a + g * g;                // RMS: sum of v^2
    if (KIND == EW_MIN) return (g < a) ? g : a;             // std::min, :115
    if (KIND == EW_MAX) return (a < g) ? g : a;             // std::max, :188
    if (KIND == EW_FIN_GM) return det_expf((double)a * (1.0 / (double)fn));  // (the reciprocal is loop-invariant)
    // EW_FIN_RMS: mean square in double rounded to float, then sqrt like rmsTwoGrids (:145-146)
    const float ms = (float)((double)a / (double)fn);
    return __builtin_sqrtf(ms);
}

constexpr int kMaxFuseSources = 8;
struct FuseSources {
    const float* p[kMaxFuseSources];
};

// A VALUE says what one voxel of a result is.  A small struct, handed to the kernels by value, with
//   kSources    how many source volumes it reads at most (sources(): how many in this launch),
//   kInPlace    whether it also reads the destination's own voxel: then x[0], the sources follow,
//   kLogTable   whether it needs det_logf's table in LDS,
//   operator()  the voxel from the loaded floats x[], through the per-voxel functions above.
// The kernels ask for K voxels at a time through voxels(), just below: the generic one calls operator() per voxel; a value
// whose voxels share work has no operator() and its own overload instead (FuseN, right after the generic one).
// k_voxelwise writes a value's volume; k_collapse_max_z takes its arg-max over the planes without writing it -- the same
// function of the same floats, hence the same bits.
template <int SOURCES, bool IN_PLACE = false, bool LOG_TABLE = false>
struct VoxelValue {
    static constexpr int kSources = SOURCES;
    static constexpr bool kInPlace = IN_PLACE, kLogTable = LOG_TABLE;
    __device__ int sources() const { return SOURCES; }
};

// det_logf's table for the values that ask for it (whole block; ends with a barrier), no LDS and no barrier for the others
template <bool NEEDED>
__device__ __forceinline__ const double2* log_table()
{
    if constexpr (NEEDED) {
        __shared__ double2 tab[kLogTabSize];
        det_log_table_fill(tab);
        return tab;
    } else {
        return nullptr;
    }
}

template <int K, int L, class V>
__device__ __forceinline__ void voxels(const V& v, float* r, const float (*x)[L], const double2* log_tab)
{
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = v(x[k], log_tab);
}

// The accumulate modes DSI_ACC_SUM, _INV_SUM, _LOG_SUM, _SQ_SUM, _MIN, _MAX (0..5): the kind that accumulates a map, the
// kind that finalizes the accumulator (-1: none) and the identity element the accumulator starts from.
template <int MODE>
struct AccMode {
    static_assert(MODE >= 0 && MODE <= 5, "an accumulate mode");
    static constexpr int kAcc = MODE == 0 ? EW_ADD : MODE == 1 ? EW_ADD_INV : MODE == 2 ? EW_ADD_LOG : MODE == 3 ? EW_ADD_SQ : MODE == 4 ? EW_MIN : EW_MAX;
    static constexpr int kFin = MODE == 0 ? EW_FIN_AM : MODE == 1 ? EW_FIN_HM : MODE == 2 ? EW_FIN_GM : MODE == 3 ? EW_FIN_RMS : -1;
    static constexpr float kIdentity = MODE == 4 ? __builtin_inff() : MODE == 5 ? -__builtin_inff() : 0.f;
};

// n-ary fusion in ONE pass: dst = finalize(accumulate(... accumulate(identity, src[0]) ..., src[n-1]))
// with exactly the operations, in exactly the order, of dsi_grid_accumulate_begin / n x
// dsi_grid_accumulate / dsi_grid_finalize (so the bits are the same), reading every source once:
// (n + 1) * 4 B per voxel instead of (3 n + 2) * 4 B.
template <int MODE>
struct FuseN : VoxelValue<kMaxFuseSources, false, AccMode<MODE>::kAcc == EW_ADD_LOG> {
    int n_src;
    float fn;
    __device__ int sources() const { return n_src; }
};

// FuseN's voxels(): source by source for the K voxels together, one test of n_src per source
template <int K, int MODE>
__device__ __forceinline__ void voxels(const FuseN<MODE>& v, float* r, const float (*x)[kMaxFuseSources], const double2* log_tab)
{
    using M = AccMode<MODE>;
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = M::kIdentity;
#pragma unroll
    for (int c = 0; c < kMaxFuseSources; ++c)
        if (c < v.n_src) {
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] = ew_op<M::kAcc>(r[k], x[k][c], 0.f, 0.f, log_tab);
        }
    if constexpr (M::kFin >= 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = ew_op<M::kFin>(r[k], 0.f, v.fn, 0.f);
    }
}

// 128-bit grid-stride body, scalar tail of n & 3 voxels in block 0; launched on grid_for(n / 4 + 1, 256) blocks
// (launch_voxelwise).  An in-place value's voxel is loaded and then stored by the same thread.
template <class V>
__global__ __launch_bounds__(256) void k_voxelwise(float* dst, FuseSources src, size_t n, V v)
{
    constexpr int kOwn = V::kInPlace ? 1 : 0, kLoaded = kOwn + V::kSources;
    const double2* log_tab = log_table<V::kLogTable>();
    const int n_src = v.sources();
    const size_t n4 = n / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float x[4][kLoaded], r[4];  // all loads of a voxel group in flight before the arithmetic
        const auto put = [&](int c, const float4 q) {
            x[0][c] = q.x;
            x[1][c] = q.y;
            x[2][c] = q.z;
            x[3][c] = q.w;
        };
        if (V::kInPlace) put(0, reinterpret_cast<const float4*>(dst)[i]);
#pragma unroll
        for (int c = 0; c < V::kSources; ++c)
            if (c < n_src) put(kOwn + c, reinterpret_cast<const float4*>(src.p[c])[i]);
        voxels<4>(v, r, x, log_tab);
        reinterpret_cast<float4*>(dst)[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = n4 * 4 + threadIdx.x;
        float x[1][kLoaded], r[1];
        if (V::kInPlace) x[0][0] = dst[i];
#pragma unroll
        for (int c = 0; c < V::kSources; ++c)
            if (c < n_src) x[0][kOwn + c] = src.p[c][i];
        voxels<1>(v, r, x, log_tab);
        dst[i] = r[0];
    }
}

// 2-ary camera fusion.  In place: dst = op(dst, g).  Else dst = op(0 + a, g): what "dst.resetGrid(); dst.addTwoGrids(a);
// dst.<op>TwoGrids(g)" (process1.cpp:126-158) leaves in dst, in one pass (0 + a == a exactly for a >= 0)
template <int OP, bool IN_PLACE>
struct Fuse2 : VoxelValue<IN_PLACE ? 1 : 2, IN_PLACE> {
    __device__ float operator()(const float* x, const double2*) const { return fuse_op<OP>(IN_PLACE ? x[0] : 0.f + x[0], x[1]); }
};

struct HarmonicMeanN : VoxelValue<1, true> {  // harmonicMeanTwoGrids(grid2, n): fn = n, fn1 = n - 1
    float fn, fn1;
    __device__ float operator()(const float* x, const double2*) const { return harmonic_mean_n(x[0], x[1], fn, fn1); }
};

template <int KIND>
struct Accumulate : VoxelValue<1, true, KIND == EW_ADD_LOG> {
    __device__ float operator()(const float* x, const double2* log_tab) const { return ew_op<KIND>(x[0], x[1], 0.f, 0.f, log_tab); }
};

template <int KIND>
struct Finalize : VoxelValue<0, true> {
    float fn;
    __device__ float operator()(const float* x, const double2*) const { return ew_op<KIND>(x[0], 0.f, fn, 0.f); }
};

// (3e) FUSED Alg. 2: process_2 / process_5 of one window (process2.cpp:98-289) without a DSI.
//
// The (band, plane) pairs of k_vote_fuse_argmax, each voted in 2N phases in the reference's order -- sub-interval k
// ascending, camera 0 before camera 1 -- with the zeroed-band LDS stream and the read-back of that kernel.  Per cell a
// thread keeps camera 0's value c0_k of the running sub-interval and the temporal accumulator of the fused volume A_tc
// (camera_time: also A_l, A_r of the two cameras) in registers across the pair's phases:
//   s_k = fuse_op<sf>(0 + c0_k, c1_k)                                         (process2.cpp:159-189, Fuse2)
//   tf 2: A = A + 1 / (0.01 + x), then N / A; tf 4: A = A + x, then A / N      (ew_op EW_ADD_INV / EW_ADD, EW_FIN_*)
//   time_camera = fin(A_tc); camera_time = fuse_op<sf'>(0 + fin(A_l), fin(A_r)) (process2.cpp:266-289, 3 <-> 4 swapped)
// -- the functions k_voxelwise<Fuse2 / Accumulate / Finalize> apply to the grids, in the same order per cell: the
// same bits.  After the last phase each output's running (maximum, first index) is updated; keys leave as in
// k_vote_fuse_argmax (atomicMax of conf bits << 8 | 255 - plane, k_unpack_argmax).
__host__ __device__ constexpr int alg2_converse_op(int sf) { return sf == 3 ? 4 : (sf == 4 ? 3 : sf); }

template <int TF>
__device__ __forceinline__ float alg2_accumulate(float a, float x)
{
    return ew_op<TF == 2 ? EW_ADD_INV : EW_ADD>(a, x, 0.f, 0.f);
}

template <int TF>
__device__ __forceinline__ float alg2_finalize(float a, float fn)
{
    return ew_op<TF == 2 ? EW_FIN_HM : EW_FIN_AM>(a, 0.f, fn, 0.f);
}

template <int CELLS>
__device__ __forceinline__ void alg2_better(FusedBest<CELLS>& fb, int kk, float f, int z)
{
    const bool better = fb.best[kk] < f;  // strict: the first maximum wins (cartesian3dgrid.cpp:132-134)
    fb.best[kk] = better ? f : fb.best[kk];
    const int sh = (kk & 3) * 8;
    const uint32_t with_z = (fb.idx4[kk >> 2] & ~(0xffu << sh)) | ((uint32_t)z << sh);
    fb.idx4[kk >> 2] = better ? with_z : fb.idx4[kk >> 2];
}

// camera 1's read-back of sub-interval k (fused_readback, as fused_consume): the camera fusion and the temporal
// accumulators per cell, then -- after the last sub-interval -- the finalisation and the arg-max update
template <int CELLS, int SF, int TF, bool CT>
__device__ __forceinline__ void alg2_consume_c1(acc_t* __restrict__ band, int nx, int n_own, int rows_lds,
                                                const float* __restrict__ c0, float* __restrict__ atc, float* __restrict__ al,
                                                float* __restrict__ ar, FusedBest<CELLS>& fb_tc, FusedBest<CELLS>& fb_ct, int z,
                                                bool last, float fn)
{
    fused_readback<CELLS, CELLS / 2>(band, nx, n_own, rows_lds, [&](int kk, float v) {
        atc[kk] = alg2_accumulate<TF>(atc[kk], fuse_op<SF>(0.f + c0[kk], v));
        if (CT) {
            al[kk] = alg2_accumulate<TF>(al[kk], c0[kk]);
            ar[kk] = alg2_accumulate<TF>(ar[kk], v);
        }
    });
    if (last) {
#pragma unroll
        for (int kk = 0; kk < CELLS; ++kk) {
            alg2_better(fb_tc, kk, alg2_finalize<TF>(atc[kk], fn), z);
            if (CT)
                alg2_better(fb_ct, kk, fuse_op<alg2_converse_op(SF)>(0.f + alg2_finalize<TF>(al[kk], fn), alg2_finalize<TF>(ar[kk], fn)), z);
        }
    }
}

template <int MAPPING, int CELLS, bool CT>
__global__ __launch_bounds__(1024) void k_vote_fuse_argmax_alg2(Alg2Batches bt, Geom g, BandPlan bp, int sf, int tf,
                                                           unsigned long long* __restrict__ keys_tc,
                                                           unsigned long long* __restrict__ keys_ct)
{
    constexpr int BLOCK = 1024;
    extern __shared__ acc_t band[];
    __shared__ int s_pass;
    constexpr int kPass0 = 2 * (BLOCK / kWave);
    const int nx = g.nx;
    // contiguous pieces of the band-major pair list: XCD x takes the x-th eighth, split evenly over its workgroups
    const int P = bp.bands * g.nz;
    const int x = blockIdx.x & 7, l = blockIdx.x >> 3, per = gridDim.x >> 3;
    const int lo = (int)(((long long)P * x) / 8), hi = (int)(((long long)P * (x + 1)) / 8);
    const int q_begin = lo + (int)(((long long)(hi - lo) * l) / per);
    const int q_end = lo + (int)(((long long)(hi - lo) * (l + 1)) / per);
    if (q_begin >= q_end) return;
    {
        const int all_cells = (bp.band_rows + 2) * nx;
        for (int i = threadIdx.x; i < all_cells; i += BLOCK) band[i] = 0;
        if (threadIdx.x == 0) s_pass = kPass0;
    }
    __syncthreads();
    // the batch table is read where it lies, in the kernel-argument segment (`bt` is the FIRST parameter; layout lock:
    // dsi_kernels.h, next to Alg2Batches), with scalar loads at the uniform batch index -- as k_vote_fuse_argmax does
    typedef const FusedCamera __attribute__((address_space(4))) * KernargBatches;
    const KernargBatches kb = (KernargBatches)__builtin_amdgcn_kernarg_segment_ptr();
    auto batch = [&](int b) -> FusedCamera {
        FusedCamera o;
        o.sxy = kb[b].sxy;
        o.coef = kb[b].coef;
        o.cuts = kb[b].cuts;
        o.slow_any = kb[b].slow_any;
        o.np = kb[b].np;
        return o;
    };
    float c0[CELLS], atc[CELLS];
    float al[CT ? CELLS : 1], ar[CT ? CELLS : 1];
    FusedBest<CELLS> fb_tc;
    FusedBest<CELLS> fb_ct;  // (unused without camera_time: the compiler drops it)
    int cur_j = -1, r0 = 0, r1 = 0, n_own = 0;
    auto emit_one = [&](unsigned long long* keys, auto& fb) {
        unsigned long long* kp = keys + (size_t)r0 * nx;
        int t = (int)threadIdx.x;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int k = 0; k < CELLS; ++k) {
            const int i = t + k * 1024;
            if (i < n_own) {
                const uint32_t zi = (fb.idx4[k >> 2] >> ((k & 3) * 8)) & 0xffu;
                atomicMax(kp + i, ((unsigned long long)__float_as_uint(fb.best[k]) << 8) | (255u - zi));
            }
        }
    };
    for (int q = q_begin; q < q_end; ++q) {
        const int j = q / g.nz, z = q - j * g.nz;
        if (j != cur_j) {
            if (cur_j >= 0) {
                emit_one(keys_tc, fb_tc);
                if constexpr (CT) emit_one(keys_ct, fb_ct);
            }
            cur_j = j;
            r0 = j * bp.band_rows;
            r1 = min(g.ny, r0 + bp.band_rows);
            n_own = (r1 - r0) * nx;
#pragma unroll
            for (int k = 0; k < CELLS; ++k) fb_tc.best[k] = -1.f;  // below every DSI value (>= 0)
#pragma unroll
            for (int k = 0; k < (CELLS + 3) / 4; ++k) fb_tc.idx4[k] = 0u;
            if constexpr (CT) {
#pragma unroll
                for (int k = 0; k < CELLS; ++k) fb_ct.best[k] = -1.f;
#pragma unroll
                for (int k = 0; k < (CELLS + 3) / 4; ++k) fb_ct.idx4[k] = 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < CELLS; ++k) {
            atc[k] = 0.f;  // the reference's accumulators start from reset grids (process2.cpp:90, fresh left / right)
            if (CT) {
                al[k] = 0.f;
                ar[k] = 0.f;
            }
        }
        const int rows_lds = r1 - r0 + 2;
        const int Li = max(r0 - 1, 0), Ui = min(r1, g.ny - 1);
#pragma nounroll
        for (int p = 0; p < 2 * bt.n_sub; ++p) {
            const FusedCamera cam = batch(p);
            uint32_t first_cuts = 0u;
            if (MAPPING == 1 && cam.np > 0) {  // (the rule of k_vote_fuse_argmax's first_cuts_of)
                int lg = cam.np >= (BLOCK / kWave) * 16 ? 3 : 2;
                while (lg < 5 && cam.np >= (((BLOCK / kWave) * 16) << (lg + 1))) ++lg;
                if (bp.pass_lg > 0) lg = bp.pass_lg;
                const int pk = min((int)((threadIdx.x / kWave) << lg) + (int)(threadIdx.x & 63), cam.np - 1);
                first_cuts = cam.cuts[((size_t)j * g.nz + z) * cam.np + pk];
            }
            stream_item<BLOCK, MAPPING, true, true>(cam.sxy, cam.coef, cam.cuts, cam.slow_any, cam.np, g, bp, j, z, 0, cam.np,
                                                    reinterpret_cast<char*>(band), Li, Ui, r0 - 1, &s_pass, first_cuts);
            __syncthreads();
            if (threadIdx.x == 0) s_pass = kPass0;
            if ((p & 1) == 0) {
                fused_consume<CELLS, 1, FUSED_KEEP>(band, nx, n_own, rows_lds, c0, fb_tc, z);
            } else {
                const bool last = p == 2 * bt.n_sub - 1;
                const float fn = (float)bt.n_sub;
#define DSI_ALG2_C1(SF, TF) alg2_consume_c1<CELLS, SF, TF, CT>(band, nx, n_own, rows_lds, c0, atc, al, ar, fb_tc, fb_ct, z, last, fn)
#define DSI_ALG2_SF(TF)            \
    switch (sf) {                  \
    case 1: DSI_ALG2_C1(1, TF); break; \
    case 2: DSI_ALG2_C1(2, TF); break; \
    case 3: DSI_ALG2_C1(3, TF); break; \
    case 4: DSI_ALG2_C1(4, TF); break; \
    case 5: DSI_ALG2_C1(5, TF); break; \
    default: DSI_ALG2_C1(6, TF); break; \
    }
                if (tf == 2) {
                    DSI_ALG2_SF(2)
                } else {
                    DSI_ALG2_SF(4)
                }
#undef DSI_ALG2_SF
#undef DSI_ALG2_C1
            }
            __syncthreads();
        }
    }
    emit_one(keys_tc, fb_tc);
    if constexpr (CT) emit_one(keys_ct, fb_ct);
}

// ---- n-ary geometric mean as the balanced TREE of the reference's own 2-ary op (DSI_ACC_GM_TREE):
//   n = 2: sqrt(a b)                     = Grid3D::geometricMeanTwoGrids, cartesian3dgrid.h:150-156, bit for bit
//   n = 4: sqrt(sqrt(a b) sqrt(c d))     n = 8: one level more
// i.e. what a user of the reference gets by calling geometricMeanTwoGrids on pairs of grids and then on the
// results.  ~2 fp32 operations per source and voxel: a pure HBM stream, where exp(mean(log v)) of
// DSI_ACC_LOG_SUM (any n, sum-reducible across GPUs) costs ~100 fp64 operations per voxel.
template <int N>
__device__ __forceinline__ float gm_tree(const float* v)
{
    float t[N];
#pragma unroll
    for (int c = 0; c < N; ++c) t[c] = v[c];
#pragma unroll
    for (int w = N; w > 1; w >>= 1)
#pragma unroll
        for (int c = 0; c < w / 2; ++c) t[c] = fuse_op<3>(t[2 * c], t[2 * c + 1]);
    return t[0];
}

template <int N>
struct GmTree : VoxelValue<N> {
    __device__ float operator()(const float* x, const double2*) const { return gm_tree<N>(x); }
};

struct Identity : VoxelValue<1> {  // the volume itself
    __device__ float operator()(const float* x, const double2*) const { return x[0]; }
};

// cartesian3dgrid.cpp:115-137 on a value's volume without materialising it: thread = pixel, planes walked in order from
// plane 0's value, strict '<' keeps the first maximum (std::max_element); U planes' loads in flight before the
// arithmetic (a last group of fewer than U planes reads the last plane again in their place and does not take it).
// Lanes of a wave read consecutive x of one plane row: coalesced 256-B segments.
// Identity: collapseMaxZSlice of a grid.  Fuse2<OP, false>: of "fused.resetGrid(); fused.addTwoGrids(a);
// fused.<op>TwoGrids(b)" (process1.cpp:126-158 + mapper_emvs_stereo.cpp:368) with 8 instead of 12 + 4 bytes per voxel of
// traffic, for streams of windows that only need the depth map (main.cpp:177).  FuseN, GmTree: of the n-ary fusion of up
// to 8 volumes, n * 4 B per voxel read, nothing written but the maps.
template <class V, int U>
__global__ __launch_bounds__(256) void k_collapse_max_z(FuseSources src, int npix, int nz, V v, float* __restrict__ conf,
                                                        uint8_t* __restrict__ idx, const float* __restrict__ planes,
                                                        float* __restrict__ depth)
{
    static_assert(!V::kInPlace, "there is no destination volume");
    const double2* log_tab = log_table<V::kLogTable>();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int n_src = v.sources();
    const auto load = [&](float (*x)[V::kSources], int k) {
        size_t at[U];
#pragma unroll
        for (int u = 0; u < U; ++u) at[u] = (size_t)min(k + u, nz - 1) * npix + p;
#pragma unroll
        for (int c = 0; c < V::kSources; ++c)
            if (c < n_src) {
#pragma unroll
                for (int u = 0; u < U; ++u) x[u][c] = src.p[c][at[u]];
            }
    };
    float best = 0.f;
    int best_k = 0;
    for (int k = 0; k < nz; k += U) {
        float x[U][V::kSources], f[U];
        load(x, k);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            voxels<1>(v, &f[u], &x[u], log_tab);
            // plane 0 starts the maximum; a select, no branch: the loads stay ahead of the arithmetic
            const bool better = (k + u < nz) & ((k + u == 0) | (best < f[u]));
            best = better ? f[u] : best;
            best_k = better ? k + u : best_k;
        }
    }
    conf[p] = best;
    idx[p] = (uint8_t)best_k;
    if (depth) depth[p] = planes[best_k];  // mapper_emvs_stereo.cpp:302-313
}

// cartesian3dgrid.cpp:164-174: sum of squares in double (order differs from the
// sequential loop; relative difference ~1e-16 * log n)
__global__ __launch_bounds__(256) void k_mean_square(const float* __restrict__ dsi, size_t n,
                                                     double* __restrict__ accum)
{
    __shared__ double part[4];
    double acc = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v = (double)dsi[i];
        acc += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = (part[0] + part[1]) + (part[2] + part[3]);
        unsafeAtomicAdd(accum, t);
    }
}

// --------------------------------------------------- post-arg-max filters ---
// Device side of MapperEMVS::getDepthMapFromDSI after the arg-max
// (mapper_emvs_stereo.cpp:390-436; the Telea inpainting of the dense map stays out).
// All of it is integer / exactly representable float work on a W x H image.
__device__ __forceinline__ uint32_t float_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // monotone float -> uint
}
__device__ __forceinline__ float key_float(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// :393 conf(0,0) = max_confidence, then min / max for cv::normalize(NORM_MINMAX)
__global__ __launch_bounds__(256) void k_conf_minmax(float* __restrict__ conf, int n,
                                                     float max_confidence,
                                                     uint32_t* __restrict__ mm /* [min,max] keys */)
{
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float v = conf[i];
        if (i == 0) {
            v = max_confidence;
            conf[0] = v;
        }
        const uint32_t k = float_key(v);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (uint32_t)__shfl_down((int)lo, off, 64));
        hi = max(hi, (uint32_t)__shfl_down((int)hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

__device__ __forceinline__ uint8_t saturate_u8(float v)
{
    const float r = __builtin_rintf(v);  // cvRound: half to even
    return (uint8_t)(r < 0.f ? 0 : (r > 255.f ? 255 : (int)r));
}

// :394-397 normalize to [0,255] (scale/shift in double, applied in float), (0,0) = 0, to u8
__global__ __launch_bounds__(256) void k_conf8(const float* __restrict__ conf, int n,
                                               const uint32_t* __restrict__ mm,
                                               uint8_t* __restrict__ conf8)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double smin = (double)key_float(mm[0]), smax = (double)key_float(mm[1]);
    const double range = smax - smin;
    const double scale = 255.0 * (range > 2.220446049250313e-16 ? 1. / range : 0.);
    const double shift = 0.0 - smin * scale;
    const float a = (float)scale, b = (float)shift;
    float v = conf[i] * a + b;
    if (i == 0) v = 0.f;
    conf8[i] = saturate_u8(v);
}

struct GaussK {
    float w[64];
};

// :403-409 cv::adaptiveThreshold(ADAPTIVE_THRESH_GAUSSIAN_C, THRESH_BINARY, ksize, delta = -C)
__global__ __launch_bounds__(256) void k_adaptive_mask(const uint8_t* __restrict__ conf8, int nx,
                                                       int ny, int ksize, GaussK kern, int idelta,
                                                       uint8_t* __restrict__ mask)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const int r = ksize / 2;
    float acc = 0.f;
    for (int ty = -r; ty <= r; ++ty) {  // column pass over row-pass results, BORDER_REPLICATE
        const int yy = min(max(y + ty, 0), ny - 1);
        float row = 0.f;
        for (int tx = -r; tx <= r; ++tx)
            row += kern.w[tx + r] * (float)conf8[(size_t)yy * nx + min(max(x + tx, 0), nx - 1)];
        acc += kern.w[ty + r] * row;
    }
    const int mean = saturate_u8(acc);
    mask[(size_t)y * nx + x] = ((int)conf8[(size_t)y * nx + x] - mean > -idelta) ? 1 : 0;
}

// :420-423 huangMedianFilter (median_filtering.cpp:33-158): for every pixel the median
// (compute_median_histogram: smallest v whose cumulative count reaches (num+1)/2) of the
// masked in-image values of its window; 0 when the window holds none
__global__ __launch_bounds__(256) void k_masked_median(const uint8_t* __restrict__ idx,
                                                       const uint8_t* __restrict__ mask, int nx,
                                                       int ny, int p, uint8_t* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const int y0 = max(y - p, 0), y1 = min(y + p, ny - 1), x0 = max(x - p, 0), x1 = min(x + p, nx - 1);
    int num = 0;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) num += mask[(size_t)yy * nx + xx] > 0 ? 1 : 0;
    const int middle = (num + 1) / 2;
    int best = 256;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
            if (!(mask[(size_t)yy * nx + xx] > 0)) continue;
            const int v = idx[(size_t)yy * nx + xx];
            if (v >= best) continue;
            int c = 0;  // values <= v in the window
            for (int y2 = y0; y2 <= y1; ++y2)
                for (int x2 = x0; x2 <= x1; ++x2)
                    c += (mask[(size_t)y2 * nx + x2] > 0 && idx[(size_t)y2 * nx + x2] <= v) ? 1 : 0;
            if (c >= middle) best = v;
        }
    out[(size_t)y * nx + x] = (uint8_t)(num == 0 ? 0 : best);
}

// :426-427 removeMaskBoundary (:316-329) and :435 convertDepthIndicesToValues
__global__ __launch_bounds__(256) void k_finish_depth(uint8_t* __restrict__ mask,
                                                      const uint8_t* __restrict__ idxf, int nx,
                                                      int ny, int border,
                                                      const float* __restrict__ planes,
                                                      float* __restrict__ depth)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nx * ny) return;
    const int x = i % nx, y = i / nx;
    if (x <= border || x >= nx - border || y <= border || y >= ny - border) mask[i] = 0;
    depth[i] = planes[idxf[i]];
}

__global__ void k_div_probe(const float* __restrict__ n, const float* __restrict__ d,
                            size_t count, float* __restrict__ q, float* __restrict__ ref)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float r = 1.f / d[i];
    q[i] = div_rc(n[i], d[i], r);
    ref[i] = n[i] / d[i];
}

// ---------------------------------------------------------------- exact tie resolver --
// The banded kernels sum a voxel's votes exactly (64-bit fixed point, one rounding); the reference adds them in
// fp32, in event order, rounding after every vote (cartesian3dgrid.h:261-270 inside mapper_emvs_stereo.cpp:197-201).
// Both are within ~1e-5 of each other, so the arg-max over Z can differ only where a column's two best planes are
// closer than that.  For those columns the resolver re-sums the contending voxels in the REFERENCE's order:
//   k_tie_columns      per pixel: does the column have >= 2 planes within rel_gap of its maximum (one streaming sweep)
//   k_tie_contenders   wave = such a column, lane = plane: the contending voxels
//   k_tie_hits_binned  every (packet, contending voxel): the events the plane transfer takes into the voxel's 2 x 2
//                      neighbourhood, voted with the reference's coordinates (IEEE divide), accept test and weights;
//                      a vote is recorded as (voxel, event order, weight)
//   (partition by voxel, per-voxel order in LDS, one-by-one fp32 sums: k_tie_partition, k_tie_sort_runs, k_tie_add_runs below)
//   k_tie_pick         thread = column: camera fusion, first maximum (cartesian3dgrid.cpp:132-134), patch
template <int OP>
__device__ __forceinline__ float tie_value(const float* __restrict__ a, const float* __restrict__ b, size_t i)
{
    if (OP == 0) return a[i];
    return fuse_op<OP>(0.f + a[i], b[i]);  // as the value Fuse2<OP, false> computes the fused voxel
}

// (1) thread = pixel, ONE streaming sweep over the column(s): the largest and second largest (fused) value; a column has
// >= 2 planes within rel_gap of its maximum iff the second largest is one of them.  The near-tie columns' pixels and maxima go
// to cols[] (x = pixel, y = float bits of the maximum), slots reserved per workgroup; counters[1] = their number (it keeps
// counting beyond cols_cap: the host retries with more room).
template <int OP>
__global__ __launch_bounds__(256) void k_tie_columns(const float* __restrict__ a, const float* __restrict__ b, int npix, int nz,
                                                     float rel_gap, unsigned* __restrict__ counters, uint4* __restrict__ cols,
                                                     uint32_t cols_cap)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    float best = 0.f, second = -__builtin_inff();
    if (p < npix) {
        best = tie_value<OP>(a, b, p);
        int k = 1;
        for (; k + 8 <= nz; k += 8) {  // eight planes' loads in flight before the arithmetic (as k_collapse_max_z streams)
            float va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                va[u] = a[(size_t)(k + u) * npix + p];
                vb[u] = OP == 0 ? 0.f : b[(size_t)(k + u) * npix + p];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float v = OP == 0 ? va[u] : fuse_op<OP>(0.f + va[u], vb[u]);
                second = best < v ? best : (second < v ? v : second);
                best = best < v ? v : best;
            }
        }
        for (; k < nz; ++k) {
            const float v = tie_value<OP>(a, b, (size_t)k * npix + p);
            second = best < v ? best : (second < v ? v : second);
            best = best < v ? v : best;
        }
    }
    // (an empty column is exactly zero in either summation order)
    const bool tie = p < npix && best > 0.f && second >= best - rel_gap * best;
    __shared__ unsigned s_n, s_base;
    if (threadIdx.x == 0) s_n = 0u;
    __syncthreads();
    const unsigned mine = tie ? atomicAdd(&s_n, 1u) : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && s_n) s_base = atomicAdd(&counters[1], s_n);
    __syncthreads();
    if (tie && s_base + mine < cols_cap) cols[s_base + mine] = make_uint4((unsigned)p, __float_as_uint(best), 0u, 0u);
}

// (2) WAVE = near-tie column, lane = plane: the contenders (value >= the column's threshold) by ballot -- two load
// instructions per 64 planes instead of a thread walking its column three times behind dependent loads.  cand[] <- the
// column's contending voxels (z * npix + p), one contiguous run, planes ascending; cols[j] <- (first entry of the run,
// pixel, contenders, 0); counters[0] = voxels (keeps counting beyond cap: nothing is written there, the host retries)
template <int OP>
__global__ __launch_bounds__(1024) void k_tie_contenders(const float* __restrict__ a, const float* __restrict__ b, int npix, int nz,
                                                         float rel_gap, unsigned* __restrict__ counters, uint32_t* __restrict__ cand,
                                                         uint32_t cap, uint4* __restrict__ cols, uint32_t cols_cap)
{
    // (a workgroup's 16 columns reserve their runs with ONE global atomic: thousands on one address serialise at ~13 ns apiece)
    __shared__ unsigned s_n, s_base;
    const unsigned n_cols = min(counters[1], cols_cap);
    const int lane = threadIdx.x & 63;
    for (unsigned j0 = blockIdx.x * 16u; j0 < n_cols; j0 += gridDim.x * 16u) {
        const unsigned j = j0 + (threadIdx.x >> 6);
        const bool live = j < n_cols;  // (wave-uniform)
        if (threadIdx.x == 0) s_n = 0u;
        __syncthreads();
        unsigned long long mask[4] = {0ull, 0ull, 0ull, 0ull};  // dimZ <= 256 (main.cpp:156)
        unsigned cnt = 0u, p = 0u, off = 0u;
        if (live) {
            const uint4 col = cols[j];
            p = col.x;
            const float best = __uint_as_float(col.y), thr = best - rel_gap * best;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int z = i * 64 + lane;
                if (i * 64 < nz) {
                    const bool in = z < nz && tie_value<OP>(a, b, (size_t)z * npix + p) >= thr;
                    mask[i] = __ballot(in);
                    cnt += (unsigned)__popcll(mask[i]);
                }
            }
            if (lane == 0) off = atomicAdd(&s_n, cnt);  // (LDS)
            off = (unsigned)__builtin_amdgcn_readfirstlane((int)off);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_n) s_base = atomicAdd(&counters[0], s_n);
        __syncthreads();
        if (live) {
            const unsigned base = s_base + off;
            if (lane == 0) cols[j] = make_uint4(base, p, cnt, 0u);
            if ((unsigned long long)base + cnt <= cap) {
                unsigned before = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int z = i * 64 + lane;
                    if ((mask[i] >> lane) & 1ull) {
                        const unsigned at = before + (unsigned)__builtin_amdgcn_mbcnt_hi((unsigned)(mask[i] >> 32),
                                                                                          __builtin_amdgcn_mbcnt_lo((unsigned)mask[i], 0u));
                        cand[base + at] = (uint32_t)((size_t)z * npix + p);
                    }
                    before += (unsigned)__popcll(mask[i]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_tie_patch(const uint32_t* __restrict__ pix, const uint8_t* __restrict__ new_idx,
                                                   const float* __restrict__ new_conf, int n,
                                                   const float* __restrict__ planes, float* __restrict__ conf,
                                                   uint8_t* __restrict__ idx, float* __restrict__ depth)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pix[i];
    conf[p] = new_conf[i];
    idx[p] = new_idx[i];
    depth[p] = planes[new_idx[i]];  // mapper_emvs_stereo.cpp:302-313
}

// ---- the resolver's event pass, INVERTED: (packet, contending voxel) pairs instead of (event, contending plane) pairs ----
// Walking every event over every contending plane (1 G event-planes per configs[1] camera, two IEEE divides each: round
// 4's k_tie_hits, 4.9 ms) finds the ~0.7 % of them that reach a contending voxel.  This kernel turns the loop around: a block
// takes a packet, bins its 1024 z0 locations by 2-D tile in LDS (counting sort), and every thread asks, for one
// contending voxel (x, y, z) at a time, WHICH z0 locations the transfer of mapper_emvs_stereo.cpp:177-195 can take into
// the 2 x 2 integer locations whose bilinear vote touches that voxel: X = (x0 a + bx) / d is affine in x0, so the
// pre-image of X in [x - 1, x + 1) is an interval of x0 (widened by a rigorous bound on the fp32 rounding of both
// directions), i.e. a few tiles of the packet.  The records of those tiles are then voted EXACTLY -- the reference's
// operations in the reference's order, IEEE divide, accept test of cartesian3dgrid.h:255-259, weights of :261-270 --
// so the tile test only has to be a superset.  Work: voxels x packets cheap rejections (5.5 k x 9,765 at configs[1] =
// 54 M, against 1 G event-planes) + the few records near a voxel.
// A (packet, plane) whose transfer is degenerate (a = 0: every event lands on one location; non-finite or extreme
// coefficients) scans all records of the packet; d = 0 gives no finite X: no votes.
// Output: (key, weight) records, key = rank << pos_bits | position of the vote in the reference's loop over events
// (packet * 1024 + slot); rank = rank_base + index of the voxel in `desc`.  Slots: a block owns SEGMENTS of kTieSeg
// records; a hit takes the next position of its block's virtual cursor (one LDS atomic), the hit that opens a segment
// reserves it with ONE global atomic (7.5 M hits -> ~8 k global atomics; one per hit or per wave instruction
// serialises at the memory side: ~50 ns each, 331 ms at configs[1] in round 4) and publishes its index in LDS, where the other hits of that segment
// wait for it.  A block pads its last segment with sentinel keys (rank = sentinel_rank, beyond every voxel's), so that
// the array [0, segments * kTieSeg) can be sorted as it is.
constexpr int kTieSegShift = 10;
constexpr int kTieSeg = 1 << kTieSegShift;
constexpr int kTieMaxSegs = 512;  // per block: 512 k hits
constexpr unsigned kTieSegEmpty = 0xffffffffu;
constexpr int kTieMaxTiles = 16384;  // tile starts are 16-bit halves of LDS words: 32 KB

struct alignas(16) TiePlane {  // per (packet, plane), in LDS
    float a, bx, by, d;  // mapper_emvs_stereo.cpp:177-182
    float ia, qx, qy;    // z0 location of integer X: x0 = X * ia + qx (ia = d / a, qx = -bx / a), same for y
    float hw;            // half width of the pre-image of [X - 1, X + 1) in z0 pixels, rounding included; < 0: no votes;
                         // +inf (with ia = qx = qy = 0): scan the whole packet
    float c_lo, c_hi;    // tile of the box's edges: floor(fma(centre, 1 / tile, c_lo | c_hi)), c = (margin -+ hw) / tile
    float pad_[2];
};

struct TieBinGeom {
    int shift;         // log2 of the tile side
    int margin;        // the tiles cover [-margin, n + margin) in x and y; locations outside clamp to the border tiles
    int tx_n, ty_n;    // tiles per row / column
};

__host__ __device__ inline TieBinGeom tie_bin_geom(int nx, int ny)
{
    TieBinGeom b;
    b.margin = 32;
    for (b.shift = 2;; ++b.shift) {
        b.tx_n = (nx + 2 * b.margin + (1 << b.shift) - 1) >> b.shift;
        b.ty_n = (ny + 2 * b.margin + (1 << b.shift) - 1) >> b.shift;
        if (b.tx_n * b.ty_n <= kTieMaxTiles) break;
    }
    return b;
}

__device__ __forceinline__ int tie_tile_coord(float v, int margin, float inv_tile, int n_tiles)
{
    // monotone in v (add, multiply by a positive constant, floor, clamp): lo <= v <= hi implies tile(lo) <= tile(v) <= tile(hi)
    const float t = __builtin_floorf((v + (float)margin) * inv_tile);
    return (int)fminf(fmaxf(t, 0.f), (float)(n_tiles - 1));
}

struct TieEvents {  // the raw events of a camera's batch + what stage A needs per packet
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* first;  // first event of packet k (nullptr: k * 1024)
    const float* H;         // [np][9] (k_packet_geometry)
    const float2* lut;
    int sensor_w, sensor_h;
};

struct TieOut {
    unsigned* s_vpos;          // LDS: the block's virtual cursor
    unsigned* s_seg;           // LDS: segment table [kTieMaxSegs]
    unsigned* seg_counter;     // global: segments handed out
    unsigned* flags;           // global: bit 0 = a block ran out of table entries, bit 1 = out of segments (cap)
    unsigned cap_segs;
    unsigned long long* keys;
    float* wts;
};

__device__ __forceinline__ void tie_emit(const TieOut& o, unsigned long long key, float w)
{
    const unsigned vp = atomicAdd(o.s_vpos, 1u);  // (LDS)
    const unsigned j = vp >> kTieSegShift, off = vp & (unsigned)(kTieSeg - 1);
    if (j >= (unsigned)kTieMaxSegs) {  // (one global atomic per event of this kind, not per hit: they serialise)
        if (vp == (unsigned)kTieMaxSegs * (unsigned)kTieSeg) atomicOr(o.flags, 1u);
        return;
    }
    // step 1, all lanes of the wave that hit: the lane that opens a segment reserves and publishes it ...
    if (off == 0u) {
        const unsigned b = atomicAdd(o.seg_counter, 1u);
        if (b >= o.cap_segs) atomicOr(o.flags, 2u);
        __hip_atomic_store(&o.s_seg[j], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // ... step 2: everybody reads it.  A lane can only wait here for a lane of ANOTHER wave (one of its own wave has
    // finished step 1 before any lane starts step 2), and that lane depends on nobody.
    unsigned b;
    while ((b = __hip_atomic_load(&o.s_seg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == kTieSegEmpty)
        __builtin_amdgcn_s_sleep(1);
    if (b >= o.cap_segs) return;  // (flagged by the lane that opened the segment; the host repeats the pass with more room)
    const size_t at = ((size_t)b << kTieSegShift) + off;
    o.keys[at] = key;
    o.wts[at] = w;
}

constexpr int kTieQueue = 128;  // queued (voxel, record) pairs per wave

// The exact vote of record r of packet k on voxel c: the reference's coordinates (mapper_emvs_stereo.cpp:194-195), accept test
// (cartesian3dgrid.h:255-259, see vote_global) and the bilinear weight of the corner the voxel is (:261-270)
__device__ __forceinline__ void tie_vote_pair(const TieOut& out, const uint2* __restrict__ desc, const TiePlane* __restrict__ tp,
                                              const float* __restrict__ rec_x, const float* __restrict__ rec_y,
                                              const unsigned* __restrict__ rec_slot, int c, unsigned r, int k, unsigned rank_base,
                                              unsigned pos_bits, float xmax, float ymax)
{
    const uint2 dsc = desc[c];
    const int vx = (int)(dsc.x & 0xffffu), vy = (int)(dsc.x >> 16), vz = (int)dsc.y;
    const float a = tp[vz].a, bx = tp[vz].bx, by = tp[vz].by, d = tp[vz].d;
    const float x0 = rec_x[r], y0 = rec_y[r];
    const float X = (x0 * a + bx) / d;
    const float Y = (y0 * a + by) / d;
    if (!(X >= 0.f && Y >= 0.f && X < xmax && Y < ymax)) return;
    const int xi = (int)X, yi = (int)Y;
    const unsigned dx = (unsigned)(vx - xi), dy = (unsigned)(vy - yi);
    if (dx > 1u || dy > 1u) return;
    const float fx = X - (float)xi, fy = Y - (float)yi, fx1 = 1.f - fx, fy1 = 1.f - fy;
    const float w = (dx ? fx : fx1) * (dy ? fy : fy1);  // fx1*fy1, fx*fy1, fx1*fy, fx*fy
    tie_emit(out, ((unsigned long long)(rank_base + (unsigned)c) << pos_bits) | ((unsigned long long)k * kPacket + rec_slot[r]), w);
}

// dynamic LDS: rec_x[1024] rec_y[1024] (f32) | rec_slot[1024] (u32) | tile starts, tiles + 1 of them as the 16-bit halves
// of (tiles + 2) / 2 words | TiePlane[nz] | seg[kTieMaxSegs] (u32)
// (a multiple of four words, so that the TiePlane table behind them is 16-byte aligned: one ds_read_b128 per look-up)
__host__ __device__ inline int tie_tile_words(int tiles) { return ((tiles + 2) / 2 + 3) & ~3; }
__host__ __device__ inline size_t tie_hits_lds_bytes(int tiles, int nz)
{
    return (size_t)kPacket * 12 + (size_t)tie_tile_words(tiles) * 4 + (size_t)nz * sizeof(TiePlane) + (size_t)kTieMaxSegs * 4;
}
__device__ __forceinline__ unsigned tie_tile_start(const unsigned* __restrict__ tw, int t)
{
    // half (t & 1) of word t >> 1 = 16-bit element t (little endian): ONE ds_read_u16 instead of a word read + shift + mask --
    // four of these per (voxel, packet) pair, 54 M pairs per camera
    return reinterpret_cast<const uint16_t*>(tw)[t];
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_tie_hits_binned(TieEvents ev, const float* __restrict__ centers,
                                                         const float* __restrict__ planes, Geom g, int np,
                                                         const uint2* __restrict__ desc, int nsv, unsigned rank_base,
                                                         unsigned pos_bits, unsigned sentinel_rank, TieBinGeom bg,
                                                         unsigned* __restrict__ seg_counter, unsigned cap_segs,
                                                         unsigned* __restrict__ flags,
                                                         unsigned long long* __restrict__ total_hits,
                                                         unsigned long long* __restrict__ keys, float* __restrict__ wts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ unsigned s_vpos;
    __shared__ unsigned s_wave_tot[BLOCK / 64];
    constexpr int PER = kPacket / BLOCK;  // events of a packet per thread
    __shared__ unsigned s_q[BLOCK / 64][kTieQueue];  // per wave: (voxel - v_beg) << 10 | record, pairs that passed the box test
    __shared__ unsigned s_qn[BLOCK / 64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < BLOCK / 64) s_qn[threadIdx.x] = 0u;
    float* rec_x = reinterpret_cast<float*>(s_raw);
    float* rec_y = rec_x + kPacket;
    unsigned* rec_slot = reinterpret_cast<unsigned*>(rec_y + kPacket);
    const int tiles = bg.tx_n * bg.ty_n, twords = tie_tile_words(tiles);
    unsigned* tstart = rec_slot + kPacket;  // tile t: half (t & 1) of word t >> 1; entry `tiles` = the packet's records
    TiePlane* tp = reinterpret_cast<TiePlane*>(__builtin_assume_aligned(tstart + twords, 16));  // (kPacket * 12 + 4 * twords: 16 | both)
    unsigned* s_seg = reinterpret_cast<unsigned*>(tp + g.nz);
    const int tid = threadIdx.x;
    const float inv_tile = 1.f / (float)(1 << bg.shift);
    const float xmax = (float)(g.nx - 1), ymax = (float)(g.ny - 1);
    TieOut out{&s_vpos, s_seg, seg_counter, flags, cap_segs, keys, wts};
    if (tid == 0) s_vpos = 0u;
    for (int i = tid; i < kTieMaxSegs; i += BLOCK) s_seg[i] = kTieSegEmpty;

    // this block's share of the voxels (blockIdx.y): few packets (a 50 ms window: ~490) do not fill the chip by themselves
    const int v_per = (nsv + (int)gridDim.y - 1) / (int)gridDim.y;
    const int v_beg = (int)blockIdx.y * v_per, v_end = min(nsv, v_beg + v_per);
    for (int k = blockIdx.x; k < np; k += gridDim.x) {
        __syncthreads();  // the previous packet's voxel loop has left the tables
        for (int i = tid; i < twords; i += BLOCK) tstart[i] = 0u;
        {
            const float cx_ = centers[3 * k], cy_ = centers[3 * k + 1], cz_ = centers[3 * k + 2];
            for (int z = tid; z < g.nz; z += BLOCK) {
                TiePlane P;
                plane_coefficients(cx_, cy_, cz_, planes[z], g, P.a, P.bx, P.by, P.d);
                P.ia = P.d / P.a;
                P.qx = -P.bx / P.a;
                P.qy = -P.by / P.a;
                // |X~ - X| <= 3u (nx + 2 |bx / d| + 1), the centre x * ia + qx is off by <= 6u (nx + |bx / d|) |ia|, u = 2^-24:
                // 2^-16 (...) is more than 16 times their sum
                const float beta = fabsf(P.bx / P.d) + fabsf(P.by / P.d);
                const float delta = 1.52587890625e-5f * ((float)(g.nx + g.ny + 2) + beta);
                P.hw = fabsf(P.ia) * (1.f + delta) * 1.001f + 1e-6f;
                const bool finite = __builtin_isfinite(P.a) && __builtin_isfinite(P.bx) && __builtin_isfinite(P.by) &&
                                    __builtin_isfinite(P.d);
                if (finite && P.d == 0.f) {
                    P.hw = -1.f;  // n / 0 is +-inf or NaN: no event is accepted on this plane
                } else if (!finite || !__builtin_isfinite(P.hw) || !__builtin_isfinite(P.qx) || !__builtin_isfinite(P.qy) ||
                           !__builtin_isfinite(beta) || !(fabsf(P.ia) >= 1e-6f && fabsf(P.ia) <= 1e6f) || !(delta < 0.5f)) {
                    P.ia = P.qx = P.qy = 0.f;
                    P.hw = __builtin_inff();
                }
                // (widened by 1e-3 tile: the fused multiply-add, these constants' own roundings and the two roundings of a
                //  record's tile (tie_tile_coord) are each below 3e-5 tile wherever a tile index is not clamped, so a record
                //  with edge <= x has tile(edge) <= tile(x) whatever |ia| is; hw = +inf: -inf / +inf -- the clamps take the row)
                P.c_lo = ((float)bg.margin - P.hw) * inv_tile - 1e-3f;
                P.c_hi = ((float)bg.margin + P.hw) * inv_tile + 1e-3f;
                P.pad_[0] = P.pad_[1] = 0.f;
                tp[z] = P;
            }
        }
        // the packet's z0 locations, counted per tile; a non-finite location votes on no plane
        float2 e[PER];
        int tile[PER];
        unsigned off[PER];
        {
            // stage A of the packet's events here (mapper_emvs_stereo.cpp:129-142, the function k_warp_z0 applies: same bits)
            // instead of a z0 array written and read back per call (80 MB and 28 us per camera at configs[1])
            const size_t first = ev.first ? (size_t)ev.first[k] : (size_t)k * kPacket;
            float hh[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) hh[i] = ev.H[9 * (size_t)k + i];
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const size_t at = first + (size_t)(tid + BLOCK * i);
                e[i] = warp_event_z0(ev.x[at], ev.y[at], hh, ev.lut, ev.sensor_w, ev.sensor_h);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const bool ok = __builtin_isfinite(e[i].x) && __builtin_isfinite(e[i].y);
            tile[i] = ok ? tie_tile_coord(e[i].y, bg.margin, inv_tile, bg.ty_n) * bg.tx_n +
                               tie_tile_coord(e[i].x, bg.margin, inv_tile, bg.tx_n)
                         : -1;
            // (LDS; a packet holds 1024 events: a half word cannot carry into its neighbour)
            off[i] = ok ? (atomicAdd(&tstart[tile[i] >> 1], 1u << ((tile[i] & 1) << 4)) >> ((tile[i] & 1) << 4)) & 0xffffu : 0u;
        }
        __syncthreads();
        // exclusive scan of the tile counts -> tile starts (thread t owns a contiguous stretch of tiles)
        {
            const int per = (twords + BLOCK - 1) / BLOCK;
            const int t0 = tid * per, t1 = min(twords, t0 + per);
            unsigned sum = 0u;
            for (int t = t0; t < t1; ++t) {
                const unsigned c = tstart[t];
                sum += (c & 0xffffu) + (c >> 16);
            }
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(incl, o, 64);
                if ((tid & 63) >= o) incl += v;
            }
            if ((tid & 63) == 63) s_wave_tot[tid >> 6] = incl;
            __syncthreads();
            unsigned base = incl - sum;
            for (int w = 0; w < (tid >> 6); ++w) base += s_wave_tot[w];
            for (int t = t0; t < t1; ++t) {
                const unsigned c = tstart[t], lo_n = c & 0xffffu;
                tstart[t] = base | ((base + lo_n) << 16);
                base += lo_n + (c >> 16);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (tile[i] >= 0) {
                const unsigned r = tie_tile_start(tstart, tile[i]) + off[i];
                rec_x[r] = e[i].x;
                rec_y[r] = e[i].y;
                rec_slot[r] = (unsigned)(tid + BLOCK * i);
            }
        __syncthreads();
        // Every contending voxel of this block against this packet.  A thread scans the records of its voxel's tiles
        // against the exact pre-image box; the ~10 % of (voxel, record) pairs that pass are QUEUED (per wave, in LDS) and
        // voted 64 at a time with all lanes busy -- voted where they are found, the two IEEE divisions, the weights and
        // the output slot would run for the few lanes that have a hit while the rest of the wave waits.
        // (a voxel's descriptor is loaded one turn ahead: read where it is used, its two words -- the plane first, for the
        //  early exit -- were two dependent L2 round trips per turn, in a loop whose waves are parked 69 % of the time)
        uint2 dsc_next = make_uint2(0u, 0u);
        if (v_beg + tid < v_end) dsc_next = desc[v_beg + tid];
        for (int c0 = v_beg; c0 < v_end; c0 += BLOCK) {
            const int c = c0 + tid;
            const uint2 dsc = dsc_next;
            if (c + BLOCK < v_end) dsc_next = desc[c + BLOCK];
            if (c < v_end) {
                const int vx = (int)(dsc.x & 0xffffu), vy = (int)(dsc.x >> 16), vz = (int)dsc.y;
                const float4 look = *reinterpret_cast<const float4*>(&tp[vz].ia);  // ia, qx, qy, hw
                const float hw = look.w;
                if (hw >= 0.f) {
                    const float ia = look.x, qx = look.y, qy = look.z;
                    // the box's tiles from the centre with ONE fused multiply-add per edge and per-plane constants (this is the
                    // superset filter, not the reference's arithmetic; its roundings are covered by the constants' widening,
                    // see where they are made): 18 vector instructions per (voxel, packet) instead of the 32 of
                    // centre -+ hw, (edge + margin) / tile, floor, two clamps (same box: 305 -> 296 us per camera)
                    const float cx0 = __builtin_fmaf((float)vx, ia, qx), cy0 = __builtin_fmaf((float)vy, ia, qy);
                    const float2 cc = *reinterpret_cast<const float2*>(&tp[vz].c_lo);
                    const float fx_n = (float)(bg.tx_n - 1), fy_n = (float)(bg.ty_n - 1);
                    const int txlo = (int)__builtin_amdgcn_fmed3f(__builtin_floorf(__builtin_fmaf(cx0, inv_tile, cc.x)), 0.f, fx_n);
                    const int txhi = (int)__builtin_amdgcn_fmed3f(__builtin_floorf(__builtin_fmaf(cx0, inv_tile, cc.y)), 0.f, fx_n);
                    const int tylo = (int)__builtin_amdgcn_fmed3f(__builtin_floorf(__builtin_fmaf(cy0, inv_tile, cc.x)), 0.f, fy_n);
                    const int tyhi = (int)__builtin_amdgcn_fmed3f(__builtin_floorf(__builtin_fmaf(cy0, inv_tile, cc.y)), 0.f, fy_n);
                    // (measured and dropped: both tile rows' starts read together and one loop over the records of both --
                    //  313 against 304 us)
                    for (int ty = tylo; ty <= tyhi; ++ty) {
                        const unsigned rb = tie_tile_start(tstart, ty * bg.tx_n + txlo), re = tie_tile_start(tstart, ty * bg.tx_n + txhi + 1);
                        // (the loop variable is the record's LDS address itself: no index -> address step per record)
                        for (const float* px = rec_x + rb; px < rec_x + re; ++px) {
                            const float x0 = px[0], y0 = px[kPacket];  // (rec_y = rec_x + kPacket)
                            // the pre-image test proper (the tiles are coarser), as max(|x0 - cx0|, |y0 - cy0|) <= hw: two
                            // subtractions, one maximum with |.| operands and ONE comparison, where four comparisons against
                            // xlo / xhi / ylo / yhi took four compares + three scalar mask operations -- in the loop whose trip count
                            // is the longest lane's, i.e. where most of this kernel's instructions are.  The subtraction's own
                            // rounding (<= 2^-24 hw) moves the cut by 1e-7 hw; hw carries 16 times the bound it needs (above).
                            // Never NaN: records are finite, ia and q finite, hw finite or +inf.
                            if (!(fmaxf(fabsf(x0 - cx0), fabsf(y0 - cy0)) <= hw)) continue;
                            const unsigned pos = atomicAdd(&s_qn[wv], 1u);  // (LDS)
                            const unsigned r = (unsigned)(px - rec_x);
                            if (pos < (unsigned)kTieQueue)
                                s_q[wv][pos] = ((unsigned)(c - v_beg) << 10) | r;
                            else  // a full queue (a burst of events on one pixel): vote in place
                                tie_vote_pair(out, desc, tp, rec_x, rec_y, rec_slot, c, r, k, rank_base, pos_bits, xmax, ymax);
                        }
                    }
                }
            }
            // (the wave is whole again) full batches of the queue
            unsigned n = min(*(volatile unsigned*)&s_qn[wv], (unsigned)kTieQueue);
            while (n >= 64u) {
                n -= 64u;
                const unsigned e = *(volatile unsigned*)&s_q[wv][n + (unsigned)lane];
                tie_vote_pair(out, desc, tp, rec_x, rec_y, rec_slot, v_beg + (int)(e >> 10), e & 1023u, k, rank_base, pos_bits, xmax, ymax);
            }
            if (lane == 0) *(volatile unsigned*)&s_qn[wv] = n;
        }
        {  // the rest of the queue: its entries point into this packet's records
            const unsigned n = min(*(volatile unsigned*)&s_qn[wv], (unsigned)kTieQueue);
            if ((unsigned)lane < n) {
                const unsigned e = *(volatile unsigned*)&s_q[wv][lane];
                tie_vote_pair(out, desc, tp, rec_x, rec_y, rec_slot, v_beg + (int)(e >> 10), e & 1023u, k, rank_base, pos_bits, xmax, ymax);
            }
            if (lane == 0) *(volatile unsigned*)&s_qn[wv] = 0u;
        }
    }
    __syncthreads();
    // pad the last segment with sentinels; report the block's hits
    const unsigned total = s_vpos;
    if (total != 0u && total <= (unsigned)kTieMaxSegs * (unsigned)kTieSeg) {
        const unsigned j = (total - 1u) >> kTieSegShift;
        const unsigned b = s_seg[j];
        const unsigned first = total - (j << kTieSegShift);  // records of the last segment in use: 1 .. kTieSeg
        if (b != kTieSegEmpty && b < cap_segs)
            for (unsigned o = first + (unsigned)tid; o < (unsigned)kTieSeg; o += (unsigned)BLOCK) {
                keys[((size_t)b << kTieSegShift) + o] = (unsigned long long)sentinel_rank << pos_bits;
                wts[((size_t)b << kTieSegShift) + o] = 0.f;
            }
    }
    if (tid == 0 && total != 0u) atomicAdd(total_hits, (unsigned long long)total);
}

// desc[c] = (x | y << 16, z) of voxel vox[c] = z * npix + y * nx + x
// plane_bits (optional, 8 zeroed words): bit z <- plane z holds one of the voxels (statistics; collected per workgroup in LDS)
__global__ __launch_bounds__(256) void k_tie_desc(const uint32_t* __restrict__ vox, int n, int nx, int npix, uint2* __restrict__ desc,
                                                  unsigned* __restrict__ plane_bits)
{
    __shared__ unsigned s_bits[8];
    if (threadIdx.x < 8) s_bits[threadIdx.x] = 0u;
    __syncthreads();
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) {
        const uint32_t v = vox[c];
        const uint32_t z = v / (uint32_t)npix, p = v - z * (uint32_t)npix, y = p / (uint32_t)nx, x = p - y * (uint32_t)nx;
        desc[c] = make_uint2(x | (y << 16), z);
        if (plane_bits && z < 256u && !((s_bits[z >> 5] >> (z & 31u)) & 1u)) atomicOr(&s_bits[z >> 5], 1u << (z & 31u));
    }
    __syncthreads();
    if (plane_bits && threadIdx.x < 8 && s_bits[threadIdx.x] && (s_bits[threadIdx.x] & ~plane_bits[threadIdx.x]))
        atomicOr(&plane_bits[threadIdx.x], s_bits[threadIdx.x]);
}

// ---- round 6: the recorded votes PARTITIONED by (camera, voxel) and ordered per voxel in LDS, instead of one device-wide
// radix sort of 38-bit keys (rocPRIM: 5 passes over 15.7 M pairs, 0.74 ms at configs[1] -- the last library call of the engine).
// Nothing needs the votes of DIFFERENT voxels in any order, and a voxel has a few thousand of them:
//   k_tie_partition<false>   votes per rank r = camera * nsv + voxel (a workgroup counts its stretch in LDS first: one global
//                            atomic per (workgroup, rank), not per vote -- same-address atomics serialise at the memory side)
//   k_tie_scan               exclusive prefix -> where each rank's run begins
//   k_tie_partition<true>    every vote into its rank's run, as ONE 64-bit word (event position << 32 | weight bits), in any order
//   k_tie_sort_runs          workgroup = rank: the run put in event order in LDS (a bucket sort by event position: tie_block_sort),
//                            its weights written back in that order.  Runs beyond 4,096 votes (configs[4]: ~30 k in a voxel)
//                            go through the same LDS in windows of event positions.
//   k_tie_add_runs           wave = rank: the weights added one by one in fp32 -- resetGrid (mapper_emvs_stereo.cpp:145),
//                            "grid[i] += w" per vote in event order (cartesian3dgrid.h:261-270)
constexpr int kTiePartLdsRanks = 30720;  // 120 KB of counters
constexpr unsigned long long kTiePartStretches = 256ull;  // stretches of the recorded votes per partition launch (at most)
constexpr int kTieRunLds = 4096;         // words of a wave's sorting buffer (32 KB)

template <bool SCATTER>
__global__ __launch_bounds__(1024) void k_tie_partition(const unsigned long long* __restrict__ keys, const float* __restrict__ wts,
                                                        unsigned long long n_rec, unsigned long long per_block, unsigned pos_bits,
                                                        unsigned n_ranks, int use_lds, uint32_t* __restrict__ counts_or_cursor,
                                                        const uint32_t* __restrict__ starts, unsigned long long* __restrict__ runs)
{
    extern __shared__ uint32_t s_rank[];  // use_lds: n_ranks counters, then (SCATTER) the next free slot of each rank's run
    const unsigned long long b0 = (unsigned long long)blockIdx.x * per_block, b1 = min(n_rec, b0 + per_block);
    if (b0 >= b1) return;
    const unsigned long long pos_mask = (1ull << pos_bits) - 1ull;
    if (!use_lds) {  // too many ranks for the LDS: one global atomic per vote (they spread over that many addresses)
        for (unsigned long long i = b0 + threadIdx.x; i < b1; i += 1024) {
            const unsigned long long key = keys[i];
            const unsigned r = (unsigned)(key >> pos_bits);
            if (r >= n_ranks) continue;  // (the sentinel tails of the blocks' last segments)
            const uint32_t at = atomicAdd(&counts_or_cursor[r], 1u);
            if (SCATTER) runs[(size_t)starts[r] + at] = ((key & pos_mask) << 32) | (unsigned long long)__float_as_uint(wts[i]);
        }
        return;
    }
    if (SCATTER) {
        // where this stretch's votes of rank r go: the run's start + the votes of r in the stretches before this one
        // (k_tie_colscan turned the table of counts into these offsets)
        const uint32_t* const before = counts_or_cursor + (size_t)blockIdx.x * n_ranks;
        for (unsigned r = threadIdx.x; r < n_ranks; r += 1024) s_rank[r] = starts[r] + before[r];
    } else {
        for (unsigned r = threadIdx.x; r < n_ranks; r += 1024) s_rank[r] = 0u;
        __syncthreads();
        for (unsigned long long i = b0 + threadIdx.x; i < b1; i += 1024) {
            const unsigned r = (unsigned)(keys[i] >> pos_bits);
            if (r < n_ranks) atomicAdd(&s_rank[r], 1u);  // (LDS)
        }
    }
    __syncthreads();
    if (!SCATTER) {  // this stretch's row of the table [stretch][rank] (launch_tie_partition_sums)
        uint32_t* const row = counts_or_cursor + (size_t)blockIdx.x * n_ranks;
        for (unsigned r = threadIdx.x; r < n_ranks; r += 1024) row[r] = s_rank[r];
        return;
    }
    // Four records per thread and turn, their loads in flight together.  What this launch costs is its 8-byte stores: a
    // stretch holds ~5 votes per rank, so nearly every store is its own partial-line write into a 125 MB array (0.24 ms at
    // configs[1] = 65 G stores/s; the counting launch reads the same keys in 0.04 ms).  Measured: one record per turn 0.287,
    // four 0.277, without the returning atomics on the runs' cursors (the table) 0.240 ms; 512 / 1,024 stretches 0.287 / 0.265.
    constexpr int U = 4;
    for (unsigned long long i0 = b0 + threadIdx.x; i0 < b1; i0 += 1024ull * U) {
        unsigned long long key[U];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned long long i = i0 + 1024ull * u;
            const bool in = i < b1;
            key[u] = in ? keys[i] : ~0ull;  // (rank bits all ones: >= n_ranks)
            w[u] = in ? wts[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned r = (unsigned)(key[u] >> pos_bits);
            if (r >= n_ranks) continue;
            const uint32_t slot = atomicAdd(&s_rank[r], 1u);  // (LDS)
            runs[slot] = ((key[u] & pos_mask) << 32) | (unsigned long long)__float_as_uint(w[u]);
        }
    }
}

// starts[r] = votes of the ranks below r (starts[n_ranks] = all of them); cursor[r] = 0.  One workgroup.
__global__ __launch_bounds__(1024) void k_tie_scan(const uint32_t* __restrict__ counts, unsigned n_ranks, uint32_t* __restrict__ starts,
                                                   uint32_t* __restrict__ cursor)
{
    __shared__ uint32_t wave_tot[16];
    const unsigned per = (n_ranks + 1023u) / 1024u;
    const unsigned r0 = min(n_ranks, threadIdx.x * per), r1 = min(n_ranks, r0 + per);
    uint32_t local = 0;
    for (unsigned r = r0; r < r1; ++r) local += counts[r];
    uint32_t incl = local;
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - local, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < (int)(threadIdx.x >> 6)) base += wave_tot[w];
        total += wave_tot[w];
    }
    for (unsigned r = r0; r < r1; ++r) {
        starts[r] = base;
        base += counts[r];
        if (cursor) cursor[r] = 0u;
    }
    if (threadIdx.x == 0) starts[n_ranks] = total;
}

// table[b][r] = votes of rank r in stretch b  ->  votes of rank r in the stretches BEFORE b; counts[r] = all of them.
// Thread = rank (consecutive threads read consecutive words of a row); eight rows' loads in flight.
__global__ __launch_bounds__(64) void k_tie_colscan(uint32_t* __restrict__ table, unsigned n_ranks, unsigned n_stretches,
                                                    uint32_t* __restrict__ counts)
{
    const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_ranks) return;
    uint32_t running = 0u;
    unsigned b = 0;
    for (; b + 8 <= n_stretches; b += 8) {
        uint32_t c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = table[(size_t)(b + u) * n_ranks + r];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            table[(size_t)(b + u) * n_ranks + r] = running;
            running += c[u];
        }
    }
    for (; b < n_stretches; ++b) {
        const uint32_t c = table[(size_t)b * n_ranks + r];
        table[(size_t)b * n_ranks + r] = running;
        running += c;
    }
    counts[r] = running;
}

// The n <= kTieRunLds words of a run (any order; event position << 32 | weight bits) -> ascending in tmp[0 .. n), by the whole
// workgroup (T threads).  The words are dealt to nb >= n buckets of equal position width (one LDS atomic each: count and
// rank in the bucket), the bucket starts are a prefix sum, every word goes to its bucket's stretch, and inside a bucket every
// word finds its place by counting the smaller ones.  ~6 passes over the run instead of a 66-stage bitonic network (which cost
// 2 ms at configs[1] with a wave per run).  A burst -- all events of ONE packet on a voxel -- is one bucket of 1,024 words:
// 1,024 reads per word, spread over the workgroup: slow, correct, rare.
template <int CAP, int T>
__device__ __forceinline__ void tie_block_sort(const unsigned long long* __restrict__ src, int n,
                                               unsigned long long* __restrict__ tmp, uint32_t* __restrict__ bcnt, uint32_t* __restrict__ wave_tot)
{
    constexpr int PER = CAP / T, W = T / 64;  // (wave_tot: 2 * W words)
    const int tid = (int)threadIdx.x;
    int nb = 64;
    while (nb < n) nb <<= 1;
    for (int i = tid; i < nb; i += T) bcnt[i] = 0u;
    unsigned long long key[PER];
    uint32_t rank[PER], bucket[PER];
    // the run's own span of event positions (a voxel is voted while the camera looks past it: its votes sit in a stretch of
    // the stream, and buckets over the WHOLE stream would put them into a few): min and max over the workgroup
    uint32_t pmin = 0xffffffffu, pmax = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * T;
        if (i < n) {
            key[k] = src[i];
            const uint32_t p = (uint32_t)(key[k] >> 32);
            pmin = min(pmin, p);
            pmax = max(pmax, p);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        pmin = min(pmin, (uint32_t)__shfl_xor((int)pmin, off, 64));
        pmax = max(pmax, (uint32_t)__shfl_xor((int)pmax, off, 64));
    }
    if ((tid & 63) == 0) {
        wave_tot[tid >> 6] = pmin;
        wave_tot[W + (tid >> 6)] = pmax;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < W; ++w) {
        pmin = min(pmin, wave_tot[w]);
        pmax = max(pmax, wave_tot[W + w]);
    }  // (wave_tot is written again by the prefix sum below, behind the next barrier)
    // bucket = floor((p - pmin) * scale), scale a little below nb / (span + 1): monotone in p, < nb
    const float scale = (float)nb / ((float)(pmax - pmin) + 1.f) * 0.99999f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * T;
        if (i < n) {
            const uint32_t p = (uint32_t)(key[k] >> 32);
            bucket[k] = min((uint32_t)((float)(p - pmin) * scale), (uint32_t)(nb - 1));
            rank[k] = atomicAdd(&bcnt[bucket[k]], 1u);  // (LDS)
        }
    }
    __syncthreads();
    // exclusive prefix of the bucket counts, in place (thread t owns a contiguous stretch of nb / 256 buckets)
    {
        const int per = max(1, nb / T), b0 = tid * per, b1 = min(nb, b0 + per);
        uint32_t local = 0;
        for (int b = b0; b < b1; ++b) local += bcnt[b];
        uint32_t incl = local;
        const int lane = tid & 63;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_tot[tid >> 6] = incl;
        __syncthreads();
        uint32_t base = incl - local;
        for (int w = 0; w < (tid >> 6); ++w) base += wave_tot[w];
        // the stretch's buckets with several words are ordered below by this thread: remember (start, count) in place as
        // start | count << 16 (n <= 4096: 13 bits each)
        for (int b = b0; b < b1; ++b) {
            const uint32_t c = bcnt[b];
            bcnt[b] = base | (c << 16);
            base += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * T;
        if (i < n) tmp[(bcnt[bucket[k]] & 0xffffu) + rank[k]] = key[k];
    }
    __syncthreads();
    // order inside the buckets: every word counts the smaller words of its bucket (a voxel is voted while the camera looks
    // past it, so its votes CLUSTER in time: buckets of tens of words are the rule, and a serial sort of a bucket by one
    // thread made this kernel 0.6 ms; counted by their own threads, a bucket of c words costs c reads per word, in parallel)
    uint32_t final_at[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * T;
        if (i < n) {
            const uint32_t e = bcnt[bucket[k]], c = e >> 16, s0 = e & 0xffffu;
            uint32_t smaller = 0;
            if (c > 1u)
                for (uint32_t q = 0; q < c; ++q) smaller += tmp[s0 + q] < key[k] ? 1u : 0u;  // (positions are unique within a voxel)
            final_at[k] = s0 + smaller;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * T;
        if (i < n) tmp[final_at[k]] = key[k];
    }
    __syncthreads();
}

// workgroup = rank: its run in event order -> sorted_w[starts[r] .. + counts[r]) (the weights only, 4 bytes per vote); all T
// threads work all the time -- the one-by-one additions, which only one wave can do, are k_tie_add_runs' (with them in here three
// waves of four held 48 KB of LDS idle for ~5 us per run: 0.42 ms at configs[1])
// CAP: the runs of (CAP / 2, CAP] votes (CAP = 1024: of up to 1,024; CAP = kTieRunLds: also the longer ones, in windows) -- a
// workgroup of the wrong class leaves at once; three launches, so that the many short runs do not each hold 48 KB of LDS
// T threads: 256 for the shortest class, 512 for the others -- the longest's 48 KB of LDS allow three workgroups per CU whatever
// their size, so twice the threads sort a run in about two thirds of the time (same-box: k_tie_sort_runs<4096> 152 -> 99 us with
// 512 threads, 106 with 1,024; <2048> 30.8 -> 28.5 us)
template <int CAP, int T = (CAP > 1024 ? 512 : 256)>
__global__ __launch_bounds__(T) void k_tie_sort_runs(const unsigned long long* __restrict__ runs, const uint32_t* __restrict__ starts,
                                                       const uint32_t* __restrict__ counts, unsigned pos_bits, int n_ranks,
                                                       float* __restrict__ sorted_w)
{
    __shared__ unsigned long long tmp[CAP];
    __shared__ uint32_t bcnt[CAP];
    __shared__ uint32_t wave_tot[2 * (T / 64)];
    __shared__ uint32_t s_n;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (r >= n_ranks) return;
    const uint32_t first = starts[r], cnt = counts[r];
    if (cnt == 0u || cnt <= (uint32_t)(CAP == 1024 ? 0 : CAP / 2) || (CAP != kTieRunLds && cnt > (uint32_t)CAP)) return;
    if (cnt <= (uint32_t)CAP) {
        tie_block_sort<CAP, T>(runs + first, (int)cnt, tmp, bcnt, wave_tot);
        for (uint32_t i = (uint32_t)tid; i < cnt; i += T) sorted_w[(size_t)first + i] = __uint_as_float((uint32_t)tmp[i]);
        return;
    }
    // Longer runs (configs[4]: ~30 k votes in a voxel): windows [lo, lo + 2^span_bits) of event positions; the run is scanned
    // once per window, the window's votes compacted into the upper half of tmp (the window is aimed at CAP / 4 votes), sorted
    // into the lower half and appended.  Positions are unique within a voxel: a window of one position holds one vote at most.
    unsigned span_bits = pos_bits;
    while (span_bits > 0 && ((unsigned long long)cnt >> (pos_bits - span_bits)) > (unsigned long long)(CAP / 4)) --span_bits;
    unsigned long long lo = 0;
    const unsigned long long pos_range = 1ull << pos_bits;
    unsigned long long* stage = tmp + CAP / 2;
    uint32_t done = 0;
    while (lo < pos_range) {
        const unsigned long long hi = lo + (1ull << span_bits);
        if (tid == 0) s_n = 0u;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < cnt; i0 += T) {
            const uint32_t i = i0 + (uint32_t)tid;
            const unsigned long long key = i < cnt ? runs[(size_t)first + i] : ~0ull;
            const unsigned long long p = key >> 32;
            if (i < cnt && p >= lo && p < hi) {
                const uint32_t at = atomicAdd(&s_n, 1u);  // (LDS; order is irrelevant here)
                if (at < (uint32_t)(CAP / 2)) stage[at] = key;
            }
        }
        __syncthreads();
        const uint32_t n = s_n;
        if (n > (uint32_t)(CAP / 2)) {  // denser than expected here: a narrower window
            --span_bits;
            __syncthreads();
            continue;
        }
        if (n) {
            tie_block_sort<CAP, T>(stage, (int)n, tmp, bcnt, wave_tot);
            for (uint32_t i = (uint32_t)tid; i < n; i += T) sorted_w[(size_t)first + done + i] = __uint_as_float((uint32_t)tmp[i]);
            done += n;
        }
        __syncthreads();
        lo = hi;
        if (n < (uint32_t)(CAP / 16) && span_bits < pos_bits && (lo & ((1ull << (span_bits + 1)) - 1ull)) == 0ull) ++span_bits;
    }
}

// ROW of 16 lanes = (camera, contending voxel): its weights, in event order by now, added one by one in fp32 -- resetGrid
// (mapper_emvs_stereo.cpp:145), then "grid[i] += w" per vote (cartesian3dgrid.h:261-270).  A row loads 4 x 16 consecutive weights
// (the next 64 in flight meanwhile) and its lane 0 adds them in order, lane j's weight reaching it through the
// add's own DPP operand (row_shl:j): ONE vector instruction per vote step, and the four rows of a wave walk four runs with it.
// (Round 6, first version: a wave per run, v_readlane + v_add per vote -- 2.3 instructions per vote, 34 M per call at
// configs[1], 0.12 ms with eight such waves sharing a SIMD.)  A row whose run has ended, and the lanes behind a run's last
// weight, add +0: x + 0 = x for every x this sum can hold (weights >= 0, denormals kept), so padding changes no bit.
// diff[r] (optional) = |engine value - reference-order value| / max(1, |reference-order value|)
#define DSI_TIE_ADD16(SUM, W)                                                             \
    asm volatile("s_nop 4\n\t" /* (W / EXEC may have been written by the vector unit just before: DPP read hazards) */ \
                 "v_add_f32 %0, %1, %0\n\t"                                                \
                 "v_add_f32_dpp %0, %1, %0 row_shl:1 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:2 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:3 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:5 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:6 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:7 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:8 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:9 row_mask:0xf bank_mask:0xf\n\t"       \
                 "v_add_f32_dpp %0, %1, %0 row_shl:10 row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_add_f32_dpp %0, %1, %0 row_shl:11 row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_add_f32_dpp %0, %1, %0 row_shl:12 row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_add_f32_dpp %0, %1, %0 row_shl:13 row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_add_f32_dpp %0, %1, %0 row_shl:14 row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_add_f32_dpp %0, %1, %0 row_shl:15 row_mask:0xf bank_mask:0xf"            \
                 : "+v"(SUM)                                                               \
                 : "v"(W))

__global__ __launch_bounds__(256) void k_tie_add_runs(const float* __restrict__ sorted_w, const uint32_t* __restrict__ starts,
                                                      const uint32_t* __restrict__ counts, const uint32_t* __restrict__ vox, int nsv,
                                                      int n_cams, const float* __restrict__ grid0, const float* __restrict__ grid1,
                                                      float* __restrict__ exact, uint32_t* __restrict__ count, float* __restrict__ diff)
{
    const int n_ranks = nsv * n_cams;
    const int r = blockIdx.x * 16 + (int)(threadIdx.x >> 4);  // this row's run
    const unsigned j = threadIdx.x & 15u;                      // lane within the row
    const bool have_run = r < n_ranks;
    const unsigned long long first = have_run ? starts[r] : 0ull, last = have_run ? first + counts[r] : 0ull;
    float sum = 0.f;  // (only lane 0 of the row holds the run's sum)
    // 64 weights per row and turn: lane j holds weights base + 16 c + j, c = 0..3.  The loads are UNCONDITIONAL (a lane past its
    // run's end reads weight 0 of the array and keeps +0 instead): with a branch around them the compiler has to wait for
    // every load in flight before the additions, the next turn's included
    auto fetch = [&](unsigned long long at, float (&w)[4]) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned long long i = at + 16u * (unsigned)c + j;
            const float v = sorted_w[i < last ? i : 0ull];
            w[c] = i < last ? v : 0.f;
        }
    };
    if (__builtin_amdgcn_ballot_w64(first < last) == 0ull) {  // (no run with a vote in this wave: the array may be empty)
        if (j == 0 && have_run) {
            exact[r] = 0.f;
            count[r] = 0u;
            if (diff) {
                const int cam = r / nsv;
                diff[r] = fabsf((cam == 0 ? grid0 : grid1)[vox[r - cam * nsv]]);
            }
        }
        return;
    }
    float w[4];
    fetch(first, w);
    unsigned long long base = first;
    while (__builtin_amdgcn_ballot_w64(base < last) != 0ull) {  // (wave-uniform: until the longest of the four runs is through)
        float cur[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) cur[c] = w[c];
        fetch(base + 64, w);  // the next 64, in flight during these additions
        // one by one, in order (no reassociation; lanes and rows past their run's end add +0)
        DSI_TIE_ADD16(sum, cur[0]);
        DSI_TIE_ADD16(sum, cur[1]);
        DSI_TIE_ADD16(sum, cur[2]);
        DSI_TIE_ADD16(sum, cur[3]);
        base += 64;
    }
    if (j != 0 || !have_run) return;
    exact[r] = sum;
    count[r] = counts[r];
    if (diff) {
        const int cam = r / nsv;
        const float* grid = cam == 0 ? grid0 : grid1;
        const float have = grid[vox[r - cam * nsv]];
        diff[r] = fabsf(have - sum) / fmaxf(1.f, fabsf(sum));
    }
}
#undef DSI_TIE_ADD16

// thread = near-tie column: camera fusion of the reference-order values (fuse_op, what Fuse2<OP, false> computes), first
// maximum over the column's contending planes (std::max_element, cartesian3dgrid.cpp:132-134), patch of the depth map
// (index -> depth: mapper_emvs_stereo.cpp:302-313).  cols[j] = (first entry in vox / exact, pixel, contenders); a column's
// contenders are contiguous there, planes ascending.  stats[2] += pixels whose plane changed
template <int OP>
__global__ __launch_bounds__(256) void k_tie_pick(const uint4* __restrict__ cols, int n_cols, const uint32_t* __restrict__ vox,
                                                  int nsv, int npix, const float* __restrict__ exact,
                                                  const uint32_t* __restrict__ count, const float* __restrict__ diff,
                                                  const float* __restrict__ planes, float* __restrict__ conf,
                                                  uint8_t* __restrict__ idx, float* __restrict__ depth,
                                                  unsigned* __restrict__ stats, float rel_gap)
{
    // stats[0] = max float bits of diff[], stats[1] = max votes of a voxel, stats[2] += changed pixels, stats[3] += columns whose
    // gap exceeds the worst-case reordering bound of their own most-voted contender (see below): one global atomic each per
    // WORKGROUP (thousands on one address serialise at ~50 ns apiece)
    __shared__ unsigned s_stats[4];
    if (threadIdx.x < 4) s_stats[threadIdx.x] = 0u;
    __syncthreads();
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cols) {
        const uint4 col = cols[j];
        float best = 0.f;
        int best_z = -1;
        unsigned dmax = 0u, cmax = 0u;
        for (unsigned i = col.x; i < col.x + col.z; ++i) {
            const float v = OP == 0 ? exact[i] : fuse_op<OP>(0.f + exact[i], exact[(size_t)nsv + i]);
            if (best_z < 0 || best < v) {
                best = v;
                best_z = (int)(vox[i] / (uint32_t)npix);
            }
            // (non-negative floats order like their bits; a NaN ranks above everything and fails the premise)
            dmax = max(dmax, __float_as_uint(diff[i]));
            cmax = max(cmax, count[i]);
            if (OP != 0) {
                dmax = max(dmax, __float_as_uint(diff[(size_t)nsv + i]));
                cmax = max(cmax, count[(size_t)nsv + i]);
            }
        }
        const uint32_t p = col.y;
        if (idx[p] != (uint8_t)best_z) atomicAdd(&s_stats[2], 1u);
        conf[p] = best;
        idx[p] = (uint8_t)best_z;
        depth[p] = planes[best_z];
        atomicMax(&s_stats[0], dmax);
        atomicMax(&s_stats[1], cmax);
        // The column's own worst case: a value summed in fp32 from n positive votes is within (n - 1) 2^-24 of the exact sum
        // (relative), the engine's value within 2^-24 + n 2^-31; the 2-ary op adds a few ulps.  With n = the most votes any of the
        // column's CONTENDERS has (either camera), a plane outside the gap could overtake the engine's best only if its error and
        // the best's together exceeded the gap: gap >= 2 (n 2^-24 + 2^-22) rules that out for planes with no more votes than n.
        // (Planes outside the gap with MORE votes than every contender are not covered: their counts are not known.  A
        // statistic beside the measured premise check, not a proof.)
        const float bound = 2.f * ((float)cmax * 5.9604644775390625e-8f + 2.384185791015625e-7f);
        if (rel_gap >= bound) atomicAdd(&s_stats[3], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_stats[0]) atomicMax(&stats[0], s_stats[0]);
        if (s_stats[1]) atomicMax(&stats[1], s_stats[1]);
        if (s_stats[2]) atomicAdd(&stats[2], s_stats[2]);
        if (s_stats[3]) atomicAdd(&stats[3], s_stats[3]);
    }
}

int grid_for(size_t work_items, int block, int max_blocks = 256 * 8)
{
    size_t b = (work_items + block - 1) / block;
    if (b < 1) b = 1;
    if (b > (size_t)max_blocks) b = max_blocks;
    return (int)b;
}

// f(std::integral_constant<int, v>()) for a runtime v in [LO, HI]: the one op / mode ladder of the launchers
template <int LO, int HI, class F>
hipError_t dispatch_int(int v, const F& f)
{
    if constexpr (LO <= HI) {
        if (v == LO) return f(std::integral_constant<int, LO>());
        return dispatch_int<LO + 1, HI>(v, f);
    } else {
        return hipErrorInvalidValue;
    }
}

template <class V>
hipError_t launch_voxelwise(hipStream_t s, float* dst, const FuseSources& src, size_t n, V v)
{
    hipLaunchKernelGGL(k_voxelwise<V>, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, s, dst, src, n, v);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

template <int U, class V>
hipError_t launch_collapse(hipStream_t s, const FuseSources& src, int nx, int ny, int nz, V v, float* conf, uint8_t* idx,
                           const float* planes, float* depth)
{
    const int npix = nx * ny;
    hipLaunchKernelGGL((k_collapse_max_z<V, U>), dim3((npix + 255) / 256), dim3(256), 0, s, src, npix, nz, v, conf, idx, planes, depth);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

FuseSources fuse_sources(const float* const* srcs, int n_src)
{
    FuseSources fs{};
    for (int c = 0; c < n_src; ++c) fs.p[c] = srcs[c];
    return fs;
}

// f(the value of an n-ary fusion of n_src volumes): modes 0..5 accumulate and finalize (AccMode), mode 6 is the tree of
// 2-ary geometric means, n = 2, 4, 8
template <class F>
hipError_t dispatch_fuse_n(int mode, int n_src, const F& f)
{
    if (mode != 6) return dispatch_int<0, 5>(mode, [&](auto MODE) { return f(FuseN<MODE>{{}, n_src, (float)n_src}); });
    if (n_src == 2) return f(GmTree<2>());
    if (n_src == 4) return f(GmTree<4>());
    if (n_src == 8) return f(GmTree<8>());
    return hipErrorInvalidValue;
}

}  // namespace

// 160 KB per CU, minus a little room for the kernels' static __shared__ variables
size_t max_dynamic_lds() { return 160 * 1024 - 128; }

// The dynamic-LDS limit of a kernel is a per-device function attribute: set it for the CURRENT
// device whenever this (kernel, device) pair has not been given at least `bytes` yet.  The table is
// per process; several host threads (one context each) may launch concurrently.
static hipError_t allow_dynamic_lds(const void* kern, size_t bytes)
{
    struct Entry {
        const void* kern;
        int device;
        size_t bytes;
    };
    static std::mutex mu;
    static std::vector<Entry> table;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (Entry& t : table)
        if (t.kern == kern && t.device == dev) {
            if (t.bytes >= bytes) return hipSuccess;
            if (hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes))
                return e;
            t.bytes = bytes;
            return hipSuccess;
        }
    if (hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) return e;
    table.push_back({kern, dev, bytes});
    return hipSuccess;
}

// hipOccupancyMaxActiveBlocksPerMultiprocessor, remembered per (kernel, device, block, dynamic LDS): a runtime query has
// no place on the path of every launch.  0 when the runtime cannot tell.
static int resident_blocks_cached(const void* kern, int block, size_t lds_bytes)
{
    struct Entry {
        const void* kern;
        int device, block;
        size_t bytes;
        int resident;
    };
    static std::mutex mu;
    static std::vector<Entry> table;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(mu);
    for (const Entry& t : table)
        if (t.kern == kern && t.device == dev && t.block == block && t.bytes == lds_bytes) return t.resident;
    int resident = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, block, lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        resident = 0;
    }
    table.push_back({kern, dev, block, lds_bytes, resident});
    return resident;
}

hipError_t launch_packet_geometry(hipStream_t s, const float* Rt, int np, const Geom& g,
                                  float* centers, float* H)
{
    if (np <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_packet_geometry, dim3((np + 63) / 64), dim3(64), 0, s, Rt, np, g,
                       centers, H);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_warp_z0(hipStream_t s, const uint16_t* ex, const uint16_t* ey,
                          const uint32_t* packet_first, int np, const float* H,
                          const float2* lut, int sensor_w, int sensor_h, float2* xy)
{
    if (np <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_warp_z0, dim3(np), dim3(256), 0, s, ex, ey, packet_first, np, H, lut,
                       sensor_w, sensor_h, xy);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_vote_global(hipStream_t s, const float2* xy, const float* centers, int np,
                              const float* planes, const Geom& g, float* dsi)
{
    if (np <= 0) return hipSuccess;
    const int zgroups = (g.nz + kVgPlanes - 1) / kVgPlanes;
    // gridDim.y is limited to 65535; x carries the packets
    hipLaunchKernelGGL(k_vote_global, dim3(np, zgroups), dim3(256), 0, s, xy, centers, planes, g,
                       dsi);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_sort_packets(hipStream_t s, const float2* xy, int np, int ny, int nz, int pad,
                               EvRec* sxy, uint32_t* nvalid, uint16_t* rowstart)
{
    if (np <= 0) return hipSuccess;
    const size_t lds = (size_t)(ny + 2 * pad + 3) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_sort_packets<false>, dim3(np), dim3(256), lds, s, xy, RawEvents{}, np, ny, nz, pad, sxy, nvalid,
                       rowstart);
    return hipExtGetLastError();
}

hipError_t launch_sort_packets_raw(hipStream_t s, const float* Rt, const uint16_t* ex, const uint16_t* ey,
                                   const uint32_t* packet_first, const float2* lut, int sensor_w, int sensor_h, const Geom& g,
                                   float* centers, int np, int pad, EvRec* sxy, uint32_t* nvalid,
                                   uint16_t* rowstart, int unit_multiplicity)
{
    if (np <= 0) return hipSuccess;
    const size_t lds = (size_t)(g.ny + 2 * pad + 3) * sizeof(uint32_t);
    RawEvents raw{Rt, ex, ey, packet_first, lut, sensor_w, sensor_h, g, centers, unit_multiplicity};
    hipLaunchKernelGGL(k_sort_packets<true>, dim3(np), dim3(256), lds, s, (const float2*)nullptr, raw, np, g.ny, g.nz, pad,
                       sxy, nvalid, rowstart);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_plane_coef(hipStream_t s, const float* centers, const float* planes,
                             const uint16_t* rowstart, uint32_t* nvalid, int np,
                             const Geom& g, const BandPlan& bp, PlaneCoef* coef, uint32_t* cuts)
{
    if (np <= 0) return hipSuccess;
    const unsigned tiles_p = (unsigned)((np + kCoefTilePackets - 1) / kCoefTilePackets);
    const size_t table_bytes = ((size_t)kCoefTilePackets * (size_t)(g.ny + 2 * bp.row_pad + 3) * sizeof(uint16_t) + 7) & ~(size_t)7;
    if (bp.cuts_inline) {
        // coefficients only (16 packets x 16 planes per block, no row tables staged), then the row tables transposed:
        // `cuts` is that table, u16 [ny + 2 row_pad + 3][bp.rs_stride]
        if (grouped(bp.packed) || bp.rs_stride < np || (bp.rs_stride & 63)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_plane_coef<false>, dim3((tiles_p * (unsigned)((g.nz + 15) / 16) + 63u) & ~63u), dim3(256), 0, s, centers,
                           planes, rowstart, nvalid, np, g, bp, coef, cuts);
        if (hipError_t e = hipExtGetLastError()) return e;
        const int nb1 = g.ny + 2 * bp.row_pad + 3;
        hipLaunchKernelGGL(k_transpose_rowstart, dim3((unsigned)(bp.rs_stride / 64), (unsigned)((nb1 + 63) / 64)), dim3(256), 0, s,
                           rowstart, np, nb1, bp.rs_stride, reinterpret_cast<uint16_t*>(cuts));
        return hipExtGetLastError();
    }
    if (!grouped(bp.packed) && table_bytes <= max_dynamic_lds()) {
        // 16 packets x 64 planes per block: the tables are loaded nz / 64 times
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_plane_coef<true>), table_bytes)) return e;
        hipLaunchKernelGGL(k_plane_coef<true>, dim3((tiles_p * (unsigned)((g.nz + 63) / 64) + 63u) & ~63u), dim3(1024), table_bytes, s,
                           centers, planes, rowstart, nvalid, np, g, bp, coef, cuts);
    } else {
        hipLaunchKernelGGL(k_plane_coef<false>, dim3((tiles_p * (unsigned)((g.nz + 15) / 16) + 63u) & ~63u), dim3(256), 0, s, centers,
                           planes, rowstart, nvalid, np, g, bp, coef, cuts);
    }
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

template <int BLOCK, int MAPPING>
static hipError_t launch_vote_bands_t(hipStream_t s, const EvRec* sxy, const PlaneCoef* coef,
                                      const uint32_t* cuts, const uint32_t* slow_any, int np,
                                      const Geom& g, const BandPlan& bp, void* out, unsigned long long* seam)
{
    constexpr bool PACKED = MAPPING != 0;
    constexpr bool VFILL = MAPPING == 5 || MAPPING == 6;
    const void* kern = VFILL ? reinterpret_cast<const void*>(&k_vote_bands_vfill<BLOCK, (VFILL ? MAPPING : 5)>)
                     : PACKED ? reinterpret_cast<const void*>(&k_vote_bands_packed<BLOCK, (PACKED && !VFILL ? MAPPING : 1)>)
                              : reinterpret_cast<const void*>(&k_vote_bands<BLOCK>);
    if (hipError_t e = allow_dynamic_lds(kern, bp.lds_bytes)) return e;
    unsigned blocks = (unsigned)item_count(bp.chunks * bp.bands, g.nz, bp.experiment == 200);
    uint32_t* counters = nullptr;
    if (PACKED && bp.persistent) {
        // as many workgroups as are resident at once: per CU, what the LDS and the 2048-thread limit allow
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const unsigned per_cu = std::max<unsigned>(1, std::min<unsigned>(2048u / BLOCK, (unsigned)(max_dynamic_lds() / std::max<size_t>(1, bp.lds_bytes))));
        unsigned resident = (unsigned)cus * per_cu;
        resident -= resident % 8;
        if (resident >= 8 && blocks > resident) {
            blocks = resident;
            counters = const_cast<uint32_t*>(slow_any) + g.nz;  // 8 counters behind the per-plane flags (zeroed by the sort kernel)
        }
    }
    if constexpr (VFILL)
        hipLaunchKernelGGL((k_vote_bands_vfill<BLOCK, (VFILL ? MAPPING : 5)>), dim3(blocks), dim3(BLOCK), bp.lds_bytes, s,
                           sxy, coef, cuts, slow_any, np, g, bp, out, seam, counters);
    else if constexpr (PACKED)
        hipLaunchKernelGGL((k_vote_bands_packed<BLOCK, (PACKED && !VFILL ? MAPPING : 1)>), dim3(blocks), dim3(BLOCK), bp.lds_bytes, s,
                           sxy, coef, cuts, slow_any, np, g, bp, out, seam, counters);
    else
        hipLaunchKernelGGL(k_vote_bands<BLOCK>, dim3(blocks), dim3(BLOCK), bp.lds_bytes, s, sxy, coef,
                           cuts, np, g, bp, out, seam);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

template <int BLOCK>
static hipError_t launch_vote_bands_b(hipStream_t s, const EvRec* sxy, const PlaneCoef* coef,
                                      const uint32_t* cuts, const uint32_t* slow_any, int np, const Geom& g,
                                      const BandPlan& bp, void* out, unsigned long long* seam)
{
    switch (bp.packed) {
    case 0: return launch_vote_bands_t<BLOCK, 0>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 1: return launch_vote_bands_t<BLOCK, 1>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 3: return launch_vote_bands_t<BLOCK, 3>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 5: return launch_vote_bands_t<BLOCK, 5>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 6: return launch_vote_bands_t<BLOCK, 6>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 7: return launch_vote_bands_t<BLOCK, 7>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 8:
        if constexpr (BLOCK == 1024) return launch_vote_bands_t<BLOCK, 8>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
        return hipErrorInvalidValue;  // (the paired cells exist for 1024-thread workgroups only)
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_vote_bands(hipStream_t s, const EvRec* sxy, const PlaneCoef* coef,
                             const uint32_t* cuts, const uint32_t* slow_any, int np, const Geom& g,
                             const BandPlan& bp, void* out, unsigned long long* seam)
{
    if (np <= 0) return hipSuccess;
    switch (bp.block_threads) {
    case 256: return launch_vote_bands_b<256>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 512: return launch_vote_bands_b<512>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    case 1024: return launch_vote_bands_b<1024>(s, sxy, coef, cuts, slow_any, np, g, bp, out, seam);
    default: return hipErrorInvalidValue;
    }
}

int fused_max_pairs() { return 1024 * kSplitSlice; }

hipError_t launch_prepare_cameras(hipStream_t s, const PrepCameraArgs* args, int n, const Geom& g, const BandPlan& bp)
{
    if (n < 1 || n > kFusedMaxCameras) return hipErrorInvalidValue;
    const int n_pairs = bp.bands * g.nz;
    PrepCameras cams{};
    cams.n = n;
    for (int c = 0; c < n; ++c) {
        const PrepCameraArgs& a = args[c];
        cams.cam[c].raw = RawEvents{a.Rt, a.ex, a.ey, a.packet_first, a.lut, a.sensor_w, a.sensor_h, a.g, a.centers, 0};
        cams.cam[c].np = a.np;
        cams.cam[c].sxy = a.sxy;
        cams.cam[c].nvalid = a.nvalid;
        cams.cam[c].rowstart = a.rowstart;
        cams.cam[c].planes = a.planes;
        cams.cam[c].coef = a.coef;
        cams.cam[c].cuts = a.cuts;
        cams.cam[c].pair_work = a.pair_work;
    }
    unsigned total_np = 0;
    for (int c = 0; c < cams.n; ++c) total_np += (unsigned)cams.cam[c].np;
    if (total_np == 0) return hipSuccess;
    {
        const size_t lds = (size_t)(g.ny + 2 * bp.row_pad + 3) * sizeof(uint32_t);
        hipLaunchKernelGGL(k_sort_packets_multi, dim3(total_np), dim3(256), lds, s, cams, g.ny, g.nz, bp.row_pad, n_pairs);
        if (hipError_t e = hipExtGetLastError()) return e;
    }
    const size_t table_bytes = ((size_t)kCoefTilePackets * (size_t)(g.ny + 2 * bp.row_pad + 3) * sizeof(uint16_t) + 7) & ~(size_t)7;
    const bool staged = table_bytes <= max_dynamic_lds();
    const unsigned zdiv = staged ? 64u : 16u;
    PrepBlocks pb{};
    unsigned total_blocks = 0;
    for (int c = 0; c < cams.n; ++c) {
        const unsigned tiles_p = (unsigned)((cams.cam[c].np + kCoefTilePackets - 1) / kCoefTilePackets);
        pb.n[c] = (tiles_p * (((unsigned)g.nz + zdiv - 1) / zdiv) + 63u) & ~63u;
        total_blocks += pb.n[c];
    }
    if (staged) {
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_plane_coef_multi<true>), table_bytes)) return e;
        hipLaunchKernelGGL(k_plane_coef_multi<true>, dim3(total_blocks), dim3(1024), table_bytes, s, cams, bp, pb);
    } else {
        hipLaunchKernelGGL(k_plane_coef_multi<false>, dim3(total_blocks), dim3(256), 0, s, cams, bp, pb);
    }
    return hipExtGetLastError();
}

hipError_t launch_fused_splits(hipStream_t s, const uint32_t* work0, const uint32_t* work1, int n_pairs, uint32_t fixed_per_pair,
                               unsigned long long* prefix, uint32_t* splits)
{
    if (n_pairs > 1024 * kSplitSlice) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fused_splits, dim3(1), dim3(1024), 0, s, work0, work1, n_pairs, fixed_per_pair, fused_grid_blocks(), prefix,
                       splits);
    return hipExtGetLastError();
}

// test hook dsi_test_fused_solo (experiments flavour only; bp.experiment 310 + k): see vote_fuse_argmax_body
static inline bool fused_solo(const BandPlan& bp)
{
#ifdef DSI_TIMING_EXPERIMENTS
    return bp.experiment >= 310 && bp.experiment < 318;
#else
    (void)bp;
    return false;
#endif
}

#ifdef DSI_TIMING_EXPERIMENTS
// test hook dsi_test_fused_last_launch (experiments flavour only): what the last launch of a DSI-less kernel was
static std::atomic<int> g_last_blocks{0}, g_last_interleave{-1}, g_last_kernel{0}, g_last_splits{0};
void fused_last_launch(int* blocks, int* interleave, int* kernel, int* splits)
{
    *blocks = g_last_blocks.load();
    *interleave = g_last_interleave.load();
    *kernel = g_last_kernel.load();
    *splits = g_last_splits.load();
}
#define DSI_FUSED_LAUNCHED(blocks, interleave, kernel, splits) \
    (g_last_blocks.store((int)(blocks)), g_last_interleave.store(interleave), g_last_kernel.store(kernel), g_last_splits.store((splits) ? 1 : 0))
#else
#define DSI_FUSED_LAUNCHED(blocks, interleave, kernel, splits) ((void)0)
#endif

template <int MAPPING>
static hipError_t launch_vote_fuse_argmax_t(hipStream_t s, const FusedCameras& cams, const Geom& g, const BandPlan& bp,
                                            int op, const uint32_t* splits, unsigned blocks, unsigned long long* keys,
                                            unsigned long long* trace)
{
    constexpr int CELLS = fused_cells_per_thread(MAPPING);
    if ((size_t)(bp.band_rows + 2) * g.nx > (size_t)CELLS * 1024) return hipErrorInvalidValue;
    if (cams.n == 4) {
        // four cameras: the geometric-mean tree only (op 3), one workgroup per CU, a second register array per thread -- 16
        // cells per thread in every mapping (plan_fused cuts the bands accordingly)
        constexpr int CELLS4 = kFusedCellsFourCameras;
        if (op != 3 || (size_t)(bp.band_rows + 2) * g.nx > (size_t)CELLS4 * 1024) return hipErrorInvalidValue;
        const void* kern4 = reinterpret_cast<const void*>(&k_vote_fuse_argmax<MAPPING, CELLS4, false, true>);
        if (hipError_t e = allow_dynamic_lds(kern4, bp.lds_bytes)) return e;
        hipLaunchKernelGGL((k_vote_fuse_argmax<MAPPING, CELLS4, false, true>), dim3(blocks), dim3(1024), bp.lds_bytes, s, cams, g, bp, op,
                           splits, keys, trace);
        DSI_FUSED_LAUNCHED(blocks, bp.interleave, 4, splits);
        return hipExtGetLastError();
    }
    if constexpr (MAPPING == 1 || MAPPING == 3) {
        // a band of at most half the LDS and half the cells: two workgroups per CU, the variant with <= 64 VGPRs
        constexpr int HALF = kFusedCellsTwoPerCu;
        // (bp.experiment 300: experiments flavour, DSI_FUSED_2CU=0 -- the same small band with ONE workgroup per CU, for A/B)
        // (a solo launch is the one-per-CU kernel's: the two-per-CU kernel does not deal)
        if (bp.experiment != 300 && !fused_solo(bp) && bp.lds_bytes * 2 <= max_dynamic_lds() && (size_t)(bp.band_rows + 2) * g.nx <= (size_t)HALF * 1024) {
            const void* kern2 = reinterpret_cast<const void*>(&k_vote_fuse_argmax_2cu<MAPPING, HALF>);
            if (hipError_t e = allow_dynamic_lds(kern2, bp.lds_bytes)) return e;
            // ... only if the runtime agrees that two fit (static LDS and the allocation granularity also count: a band just
            // under half the LDS would otherwise run its 2 x grid of half-size assignments in two serialised waves)
            // (the answer depends on (kernel, device, LDS bytes) only: asked once, not on every window -- ADVICE r05)
            if (resident_blocks_cached(kern2, 1024, bp.lds_bytes) < 2) goto one_per_cu;
            // (the balanced partition, an experiments-flavour option, is laid out for one workgroup per CU: not used here)
            hipLaunchKernelGGL((k_vote_fuse_argmax_2cu<MAPPING, HALF>), dim3(2 * blocks), dim3(1024), bp.lds_bytes, s, cams, g, bp, op,
                               nullptr, keys, trace);
            DSI_FUSED_LAUNCHED(2 * blocks, bp.interleave, 2, nullptr);
            return hipExtGetLastError();
        }
    }
one_per_cu:
    if constexpr (MAPPING == 1) {
        // two cameras, the packed stream: the instantiation that defers camera 1's fusion + arg-max update into the waits
        // of the next phase (vote_fuse_argmax_body, DEFER).  bp.experiment 301 (experiments flavour): off, for A/B runs
        if (cams.n == 2 && bp.experiment != 301) {
            const void* kern_d = reinterpret_cast<const void*>(&k_vote_fuse_argmax<MAPPING, CELLS, true>);
            if (hipError_t e = allow_dynamic_lds(kern_d, bp.lds_bytes)) return e;
            hipLaunchKernelGGL((k_vote_fuse_argmax<MAPPING, CELLS, true>), dim3(blocks), dim3(1024), bp.lds_bytes, s, cams, g, bp, op, splits,
                               keys, trace);
            DSI_FUSED_LAUNCHED(blocks, bp.interleave, 3, splits);
            return hipExtGetLastError();
        }
    }
    const void* kern = reinterpret_cast<const void*>(&k_vote_fuse_argmax<MAPPING, CELLS>);
    if (hipError_t e = allow_dynamic_lds(kern, bp.lds_bytes)) return e;
    hipLaunchKernelGGL((k_vote_fuse_argmax<MAPPING, CELLS>), dim3(blocks), dim3(1024), bp.lds_bytes, s, cams, g, bp, op, splits, keys, trace);
    DSI_FUSED_LAUNCHED(blocks, bp.interleave, 1, splits);
    return hipExtGetLastError();
}

size_t fused_max_cells(int mapping, int n_cameras)
{
    return (size_t)(n_cameras == 4 ? std::min(kFusedCellsFourCameras, fused_cells_per_thread(mapping)) : fused_cells_per_thread(mapping)) * 1024;
}

size_t fused_trace_words() { return (size_t)2 * fused_grid_blocks() * kFusedTracePhases * 16 * 4; }  // (two workgroups per CU at most)

#ifdef DSI_TIMING_EXPERIMENTS
// test hook dsi_test_fused_grid_blocks (experiments flavour only): the workgroup count every user of fused_grid_blocks()
// sees -- the three launches, the balanced partition and the trace -- as on a CPX / QPX partition (32 / 64 CUs); 0: the device's
static std::atomic<int> g_fused_grid_blocks_forced{0};
bool fused_grid_blocks_force(int blocks)
{
    if (blocks != 0 && (blocks < 8 || blocks > 4096 || blocks % 8 != 0)) return false;
    g_fused_grid_blocks_forced.store(blocks);
    return true;
}
#endif

int fused_grid_blocks()
{
#ifdef DSI_TIMING_EXPERIMENTS
    if (const int forced = g_fused_grid_blocks_forced.load()) return forced;
#endif
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return std::max(8, cus - cus % 8);  // one 1024-thread workgroup per CU, whole groups of 8 (XCDs)
}

hipError_t launch_vote_fuse_argmax(hipStream_t s, const FusedCameras& cams, const Geom& g, const BandPlan& bp, int op,
                                   const uint32_t* splits, unsigned long long* keys, unsigned long long* trace)
{
    if (cams.n < 1 || cams.n > kFusedMaxCameras || bp.block_threads != 1024 || bp.chunks != 1 || !bp.halo) return hipErrorInvalidValue;
    // (solo: the dealing arithmetic alone is written for gridDim.x == 1 -- the other modes divide by gridDim.x / 8)
    if (fused_solo(bp) && (splits || bp.interleave != 2 || bp.bands * g.nz < 8)) return hipErrorInvalidValue;
    const unsigned blocks = fused_solo(bp) ? 1u : (unsigned)fused_grid_blocks();
    switch (bp.packed) {
    case 1: return launch_vote_fuse_argmax_t<1>(s, cams, g, bp, op, splits, blocks, keys, trace);
    case 3: return launch_vote_fuse_argmax_t<3>(s, cams, g, bp, op, splits, blocks, keys, trace);
    case 5: return launch_vote_fuse_argmax_t<5>(s, cams, g, bp, op, splits, blocks, keys, trace);
    case 6: return launch_vote_fuse_argmax_t<6>(s, cams, g, bp, op, splits, blocks, keys, trace);
    default: return hipErrorInvalidValue;
    }
}

// camera_time on: c0, A_tc, A_l, A_r and two running maxima per cell; off: c0, A_tc and one
constexpr int alg2_cells_per_thread(int mapping, bool camera_time)
{
    return camera_time ? ((mapping == 5 || mapping == 6) ? 6 : 8) : ((mapping == 5 || mapping == 6) ? 12 : 16);
}

size_t alg2_max_cells(int mapping, bool camera_time) { return (size_t)alg2_cells_per_thread(mapping, camera_time) * 1024; }

template <int MAPPING, bool CT>
static hipError_t launch_vote_alg2_argmax_t(hipStream_t s, const Alg2Batches& bt, const Geom& g, const BandPlan& bp, int sf,
                                            int tf, unsigned long long* keys_tc, unsigned long long* keys_ct)
{
    constexpr int CELLS = alg2_cells_per_thread(MAPPING, CT);
    if ((size_t)(bp.band_rows + 2) * g.nx > (size_t)CELLS * 1024) return hipErrorInvalidValue;
    const void* kern = reinterpret_cast<const void*>(&k_vote_fuse_argmax_alg2<MAPPING, CELLS, CT>);
    if (hipError_t e = allow_dynamic_lds(kern, bp.lds_bytes)) return e;
    hipLaunchKernelGGL((k_vote_fuse_argmax_alg2<MAPPING, CELLS, CT>), dim3(fused_grid_blocks()), dim3(1024), bp.lds_bytes, s, bt, g, bp,
                       sf, tf, keys_tc, keys_ct);
    DSI_FUSED_LAUNCHED(fused_grid_blocks(), bp.interleave, 5, nullptr);
    return hipExtGetLastError();
}

template <bool CT>
static hipError_t launch_vote_alg2_argmax_m(hipStream_t s, const Alg2Batches& bt, const Geom& g, const BandPlan& bp, int sf,
                                            int tf, unsigned long long* keys_tc, unsigned long long* keys_ct)
{
    switch (bp.packed) {
    case 1: return launch_vote_alg2_argmax_t<1, CT>(s, bt, g, bp, sf, tf, keys_tc, keys_ct);
    case 3: return launch_vote_alg2_argmax_t<3, CT>(s, bt, g, bp, sf, tf, keys_tc, keys_ct);
    case 5: return launch_vote_alg2_argmax_t<5, CT>(s, bt, g, bp, sf, tf, keys_tc, keys_ct);
    case 6: return launch_vote_alg2_argmax_t<6, CT>(s, bt, g, bp, sf, tf, keys_tc, keys_ct);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_vote_alg2_argmax(hipStream_t s, const Alg2Batches& bt, const Geom& g, const BandPlan& bp, int sf, int tf,
                                   unsigned long long* keys_tc, unsigned long long* keys_ct)
{
    if (bt.n_sub < 1 || bt.n_sub > kAlg2MaxSub || sf < 1 || sf > 6 || (tf != 2 && tf != 4) || !keys_tc) return hipErrorInvalidValue;
    if (bp.block_threads != 1024 || bp.chunks != 1 || !bp.halo || g.nz > 256) return hipErrorInvalidValue;
    return keys_ct ? launch_vote_alg2_argmax_m<true>(s, bt, g, bp, sf, tf, keys_tc, keys_ct)
                   : launch_vote_alg2_argmax_m<false>(s, bt, g, bp, sf, tf, keys_tc, nullptr);
}

hipError_t launch_sort_groups(hipStream_t s, const float2* xy, int np, int S, int ny, int nz, int pad,
                              EvRec* sxy, uint8_t* spk, uint32_t* nvalid, uint16_t* rowstart)
{
    if (np <= 0) return hipSuccess;
    const int ngroups = (np + S - 1) / S;
    const size_t lds = (size_t)(ny + 2 * pad + 3) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_sort_groups, dim3(ngroups), dim3(256), lds, s, xy, np, S, ny, nz, pad, sxy, spk,
                       nvalid, rowstart);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_group_cuts(hipStream_t s, const uint32_t* prow, const uint16_t* rowstart, int np,
                             int S, const Geom& g, const BandPlan& bp, uint32_t* gcuts)
{
    if (np <= 0) return hipSuccess;
    const int ngroups = (np + S - 1) / S;
    const size_t total = (size_t)ngroups * g.nz * bp.bands;
    hipLaunchKernelGGL(k_group_cuts, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, prow,
                       rowstart, np, ngroups, S, g.nz, bp.bands, g.ny + 2 * bp.row_pad + 2, gcuts);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

template <int BLOCK>
static hipError_t launch_vote_groups_t(hipStream_t s, const EvRec* sxy, const uint8_t* spk,
                                       const PlaneCoef* coef, const uint32_t* gcuts,
                                       const uint32_t* slow_any, int np, int S, const Geom& g,
                                       const BandPlan& bp, void* out, unsigned long long* seam)
{
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_vote_groups<BLOCK>), bp.lds_bytes))
        return e;
    const int ngroups = (np + S - 1) / S;
    const unsigned blocks = (unsigned)item_count(bp.chunks * bp.bands, g.nz, bp.experiment == 200);
    hipLaunchKernelGGL(k_vote_groups<BLOCK>, dim3(blocks), dim3(BLOCK), bp.lds_bytes, s, sxy, spk,
                       coef, gcuts, slow_any, np, ngroups, S, g, bp, out, seam);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_vote_groups(hipStream_t s, const EvRec* sxy, const uint8_t* spk,
                              const PlaneCoef* coef, const uint32_t* gcuts, const uint32_t* slow_any,
                              int np, int S, const Geom& g, const BandPlan& bp, void* out, unsigned long long* seam)
{
    if (np <= 0) return hipSuccess;
    switch (bp.block_threads) {
    case 256: return launch_vote_groups_t<256>(s, sxy, spk, coef, gcuts, slow_any, np, S, g, bp, out, seam);
    case 512: return launch_vote_groups_t<512>(s, sxy, spk, coef, gcuts, slow_any, np, S, g, bp, out, seam);
    case 1024: return launch_vote_groups_t<1024>(s, sxy, spk, coef, gcuts, slow_any, np, S, g, bp, out, seam);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_seam_rows(hipStream_t s, const unsigned long long* seam, int chunks, const Geom& g,
                            const BandPlan& bp, void* out)
{
    if (bp.bands < 2) return hipSuccess;
    const size_t vol = partial_stride((size_t)g.nx * g.ny * g.nz);
    const dim3 grid((unsigned)g.nz * (unsigned)(bp.bands - 1), (unsigned)((g.nx + 511) / 512), (unsigned)chunks);
    if (bp.raw_out)
        hipLaunchKernelGGL(k_seam_rows<true>, grid, dim3(256), 0, s, seam, g, bp.bands, bp.band_rows, out, vol);
    else
        hipLaunchKernelGGL(k_seam_rows<false>, grid, dim3(256), 0, s, seam, g, bp.bands, bp.band_rows, out, vol);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_reduce_partials(hipStream_t s, const unsigned long long* partials, int chunks, size_t n,
                                  float* dsi, int accumulate, const unsigned long long* seam, const Geom* g, const BandPlan* bp)
{
    // the seam rows can be folded in when two voxels never straddle a row and 32-bit voxel indices suffice
    const bool fold = seam && g && bp && bp->bands >= 2 && (g->nx & 1) == 0 && n <= 0xffffffffull;
    if (seam && !fold && bp && bp->bands >= 2) return hipErrorInvalidValue;  // the caller must run launch_seam_rows instead
    hipLaunchKernelGGL(k_reduce_partials, dim3(grid_for(n / 2 + 1, 256)), dim3(256), 0, s,
                       partials, chunks, n, dsi, accumulate, fold ? seam : nullptr, g ? g->nx : 0, g ? g->ny : 0, g ? g->nz : 0,
                       bp ? bp->bands : 0, bp ? bp->band_rows : 0);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_fuse2(hipStream_t s, float* a, const float* g, size_t n, int op)
{
    return dispatch_int<1, 6>(op, [&](auto OP) { return launch_voxelwise(s, a, FuseSources{{g}}, n, Fuse2<OP, true>()); });
}

hipError_t launch_fuse2_into(hipStream_t s, float* dst, const float* a, const float* g, size_t n, int op)
{
    return dispatch_int<1, 6>(op, [&](auto OP) { return launch_voxelwise(s, dst, FuseSources{{a, g}}, n, Fuse2<OP, false>()); });
}

hipError_t launch_fuse_hm_n(hipStream_t s, float* a, const float* g, size_t n, int n_maps)
{
    return launch_voxelwise(s, a, FuseSources{{g}}, n, HarmonicMeanN{{}, (float)n_maps, (float)(n_maps - 1)});
}

hipError_t launch_accumulate(hipStream_t s, float* acc, const float* g, size_t n, int mode)
{
    return dispatch_int<0, 5>(mode, [&](auto MODE) {
        return launch_voxelwise(s, acc, FuseSources{{g}}, n, Accumulate<AccMode<MODE>::kAcc>());
    });
}

hipError_t launch_finalize(hipStream_t s, float* acc, size_t n, int mode, int n_maps)
{
    // k_voxelwise reads float4: a slab in the middle of a volume whose plane is no multiple of 4 pixels (the
    // reduce-scattered depth map's own planes) starts 4, 8 or 12 bytes past a 16-byte boundary.  Its first 1..3
    // elements go through the kernel's scalar tail (n < 4: no float4 access), the rest start aligned.  Per element
    // the operation is the same: the same bits.  Whole grids are aligned and take the one launch below as before.
    const size_t head = (size_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(acc) & 15u)) & 15u) / sizeof(float);
    if (head && n > head) {
        if (hipError_t e = launch_finalize(s, acc, head, mode, n_maps)) return e;
        return launch_finalize(s, acc + head, n - head, mode, n_maps);
    }
    if (mode == 4 || mode == 5) return hipExtGetLastError();  // min / max need no finalisation
    return dispatch_int<0, 3>(mode, [&](auto MODE) {
        return launch_voxelwise(s, acc, FuseSources{}, n, Finalize<AccMode<MODE>::kFin>{{}, (float)n_maps});
    });
}

// plane-sharded arg-max: (confidence, local index) -> one 64-bit key per pixel whose MAX over the
// shards is the unsharded collapseMaxZSlice (cartesian3dgrid.cpp:115-137: larger value wins, the
// smaller plane index on ties).  DSI values are >= 0 (and -0.0 never occurs: sums of >= 0 terms),
// so their bit patterns order like the floats.
__global__ __launch_bounds__(256) void k_pack_argmax(const float* __restrict__ conf,
                                                     const uint8_t* __restrict__ idx, int n,
                                                     int plane_begin,
                                                     unsigned long long* __restrict__ keys, int combine)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long bits = __float_as_uint(conf[i]);
    const unsigned long long key = (bits << 8) | (unsigned long long)(255 - ((int)idx[i] + plane_begin));
    // combine: a second plane range of the same rank joins the keys of the first
    keys[i] = (combine && keys[i] > key) ? keys[i] : key;
}

__global__ __launch_bounds__(256) void k_unpack_argmax(unsigned long long* __restrict__ keys,
                                                       int n, const float* __restrict__ planes_full,
                                                       float* __restrict__ conf,
                                                       uint8_t* __restrict__ idx,
                                                       float* __restrict__ depth, int clear)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // (clear: the buffer is the fused kernel's -- n keys + kFusedKeyTail words, the tail = its pair-dealing counters)
    if (clear && i < 2 * kFusedKeyTail) reinterpret_cast<unsigned*>(keys + n)[i] = 0u;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    if (clear) keys[i] = 0ull;  // ready for the next fused vote (saves a memset launch per window)
    const int gi = 255 - (int)(k & 255ull);
    conf[i] = __uint_as_float((uint32_t)(k >> 8));
    idx[i] = (uint8_t)gi;
    depth[i] = planes_full[gi];  // mapper_emvs_stereo.cpp:302-313 over the full depth vector
}

hipError_t launch_pack_argmax(hipStream_t s, const float* conf, const uint8_t* idx, int n, int plane_begin,
                              unsigned long long* keys, int combine)
{
    hipLaunchKernelGGL(k_pack_argmax, dim3((n + 255) / 256), dim3(256), 0, s, conf, idx, n, plane_begin, keys, combine);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_unpack_argmax(hipStream_t s, unsigned long long* keys, int n, const float* planes_full,
                                float* conf, uint8_t* idx, float* depth, int clear)
{
    hipLaunchKernelGGL(k_unpack_argmax, dim3((n + 255) / 256), dim3(256), 0, s, keys, n, planes_full, conf, idx,
                       depth, clear);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_fuse_n(hipStream_t s, float* dst, const float* const* srcs, int n_src, size_t n, int mode)
{
    if (n_src < 1 || n_src > kMaxFuseSources) return hipErrorInvalidValue;
    const FuseSources fs = fuse_sources(srcs, n_src);
    return dispatch_fuse_n(mode, n_src, [&](auto v) { return launch_voxelwise(s, dst, fs, n, v); });
}

// identity element of an accumulate mode: 0 for the sums, +inf for min, -inf for max
__global__ __launch_bounds__(256) void k_fill(float* __restrict__ a, size_t n, float v)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) a[i] = v;
}

// depth map -> page-locked host memory by the CUs (the three arrays of a fetch in one launch): see launch_store_depth_map
__global__ __launch_bounds__(256) void k_store_depth_map(const float* __restrict__ depth, const float* __restrict__ conf,
                                                         const uint8_t* __restrict__ idx, size_t npix, float* __restrict__ depth_h,
                                                         float* __restrict__ conf_h, uint8_t* __restrict__ idx_h)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        if (depth_h) depth_h[i] = depth[i];
        if (conf_h) conf_h[i] = conf[i];
    }
    if (idx_h) {
        const size_t n4 = npix / 4;  // (hipMalloc'ed and hipHostMalloc'ed arrays: 4-byte aligned)
        const uint32_t* src = reinterpret_cast<const uint32_t*>(idx);
        uint32_t* dst = reinterpret_cast<uint32_t*>(idx_h);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) dst[i] = src[i];
        if (blockIdx.x == 0 && threadIdx.x < npix - 4 * n4) idx_h[4 * n4 + threadIdx.x] = idx[4 * n4 + threadIdx.x];
    }
}

// A device -> host copy queued on an SDMA engine BEHIND a kernel holds up every later copy of that engine -- the next
// window's uploads waited for the current window's kernel (profiles/r05_cpp_window_stream_timeline.txt).  A kernel that
// stores the maps into mapped page-locked memory keeps the copy engines free for the uploads.
hipError_t launch_store_depth_map(hipStream_t s, const float* depth, const float* conf, const uint8_t* idx, size_t npix,
                                  float* depth_host_dev, float* conf_host_dev, uint8_t* idx_host_dev)
{
    if (!npix) return hipSuccess;
    // (PCIe-bound: a few CUs do, the others are the next window's)
    hipLaunchKernelGGL(k_store_depth_map, dim3(grid_for(npix, 256, 64)), dim3(256), 0, s, depth, conf, idx, npix, depth_host_dev,
                       conf_host_dev, idx_host_dev);
    return hipExtGetLastError();
}

hipError_t launch_fill(hipStream_t s, float* a, size_t n, float v)
{
    hipLaunchKernelGGL(k_fill, dim3(grid_for(n, 256)), dim3(256), 0, s, a, n, v);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_collapse_max_z(hipStream_t s, const float* dsi, int nx, int ny, int nz,
                                 float* conf, uint8_t* idx, const float* planes, float* depth)
{
    return launch_collapse<8>(s, FuseSources{{dsi}}, nx, ny, nz, Identity(), conf, idx, planes, depth);
}

hipError_t launch_collapse_max_z_fused(hipStream_t s, const float* a, const float* b, int nx, int ny, int nz, int op,
                                       float* conf, uint8_t* idx, const float* planes, float* depth)
{
    return dispatch_int<1, 6>(op, [&](auto OP) {
        return launch_collapse<4>(s, FuseSources{{a, b}}, nx, ny, nz, Fuse2<OP, false>(), conf, idx, planes, depth);
    });
}

hipError_t launch_collapse_max_z_fused_n(hipStream_t s, const float* const* srcs, int n_src, int mode, int nx, int ny,
                                         int nz, float* conf, uint8_t* idx, const float* planes, float* depth)
{
    if (n_src < 1 || n_src > kMaxFuseSources) return hipErrorInvalidValue;
    const FuseSources fs = fuse_sources(srcs, n_src);
    return dispatch_fuse_n(mode, n_src, [&](auto v) { return launch_collapse<2>(s, fs, nx, ny, nz, v, conf, idx, planes, depth); });
}

hipError_t launch_mean_square(hipStream_t s, const float* dsi, size_t n, double* accum)
{
    hipLaunchKernelGGL(k_mean_square, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, dsi, n,
                       accum);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_depth_map_filters(hipStream_t s, float* conf, const uint8_t* idx, int nx, int ny,
                                    int ksize, double C, int median_size, double max_confidence,
                                    const float* planes, uint32_t* minmax_scratch, uint8_t* conf8,
                                    uint8_t* mask, uint8_t* idx_filtered, float* depth)
{
    const int n = nx * ny;
    const uint32_t init[2] = {0xffffffffu, 0u};
    hipError_t e = hipMemcpyAsync(minmax_scratch, init, sizeof init, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_conf_minmax, dim3(grid_for(n, 256, 512)), dim3(256), 0, s, conf, n,
                       (float)max_confidence, minmax_scratch);
    hipLaunchKernelGGL(k_conf8, dim3((n + 255) / 256), dim3(256), 0, s, conf, n, minmax_scratch, conf8);
    GaussK kern{};
    if (ksize > 63) ksize = 63;
    // cv::getGaussianKernel, sigma <= 0: fixed tables up to 7, else sigma from the size
    static const float k1[] = {1.f};
    static const float k3[] = {0.25f, 0.5f, 0.25f};
    static const float k5[] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    static const float k7[] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    const float* fixed = ksize == 1 ? k1 : ksize == 3 ? k3 : ksize == 5 ? k5 : ksize == 7 ? k7 : nullptr;
    if (fixed) {
        for (int i = 0; i < ksize; ++i) kern.w[i] = fixed[i];
    } else {
        const double sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;
        const double scale2x = -0.5 / (sigma * sigma);
        double sum = 0, t[64];
        for (int i = 0; i < ksize; ++i) {
            const double x = i - (ksize - 1) * 0.5;
            t[i] = exp(scale2x * x * x);
            sum += t[i];
        }
        for (int i = 0; i < ksize; ++i) kern.w[i] = (float)(t[i] * (1. / sum));
    }
    const dim3 grid2((nx + 63) / 64, (ny + 3) / 4);
    hipLaunchKernelGGL(k_adaptive_mask, grid2, dim3(256), 0, s, conf8, nx, ny, ksize, kern,
                       (int)ceil(-C), mask);
    hipLaunchKernelGGL(k_masked_median, grid2, dim3(256), 0, s, idx, mask, nx, ny, median_size / 2,
                       idx_filtered);
    const int border = ksize / 2 > 1 ? ksize / 2 : 1;
    hipLaunchKernelGGL(k_finish_depth, dim3((n + 255) / 256), dim3(256), 0, s, mask, idx_filtered, nx,
                       ny, border, planes, depth);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

hipError_t launch_div_probe(hipStream_t s, const float* n, const float* d, size_t count, float* q,
                            float* ref)
{
    hipLaunchKernelGGL(k_div_probe, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, n, d,
                       count, q, ref);
    return hipExtGetLastError();  // status of THIS launch (hipGetLastError is sticky across calls)
}

// ---- the resolver's premise as a per-column PROOF (dsi_mapper_prove_near_ties) ----
// The resolver re-sums the planes within rel_gap of a column's maximum and trusts that no plane outside can win under the
// reference's arithmetic.  That is provable once the number n of votes of every voxel is known: the reference adds a voxel's n
// non-negative weights one by one in fp32, so its value R lies within gamma_(n-1) = (n-1) u / (1 - (n-1) u), u = 2^-24, of their
// real sum (the standard bound for recursive summation), and the engine's value E is that sum with every weight rounded to 2^-31
// and ONE rounding to fp32.  The engine keeps no counts; this pass makes them:
//   k_count_votes   H[z][yi][xi] += 1 for every vote the reference casts (transfer with the IEEE divide, accept test of
//                   cartesian3dgrid.h:255-259) -- the integer location (xi, yi) of the vote's 2 x 2 footprint; a voxel's n is
//                   the sum of the four H cells whose footprint contains it.  Global atomics on a u32 volume: a verification
//                   pass, not a product kernel (~1 G atomics per camera at configs[1]).
//   k_tie_prove     thread = column: the engine's first maximum, the resolver's threshold, and for every plane BELOW the
//                   threshold an upper bound of its reference value against a lower bound of the maximum's.
// block = (packet, group of kVgPlanes planes); thread t owns events t, t + 256, ... of the packet (as k_vote_global)
__global__ __launch_bounds__(256) void k_count_votes(TieEvents ev, const float* __restrict__ centers, const float* __restrict__ planes,
                                                     Geom g, uint32_t* __restrict__ H)
{
    const int k = blockIdx.x;
    const int zbeg = blockIdx.y * kVgPlanes, zend = min(g.nz, zbeg + kVgPlanes);
    const float cx_ = centers[3 * k], cy_ = centers[3 * k + 1], cz_ = centers[3 * k + 2];
    const size_t first = ev.first ? (size_t)ev.first[k] : (size_t)k * kPacket;
    float hh[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) hh[i] = ev.H[9 * (size_t)k + i];
    float2 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t at = first + threadIdx.x + 256 * i;
        e[i] = warp_event_z0(ev.x[at], ev.y[at], hh, ev.lut, ev.sensor_w, ev.sensor_h);  // mapper_emvs_stereo.cpp:129-142
    }
    const float xmax = (float)(g.nx - 1), ymax = (float)(g.ny - 1);
    const size_t plane_sz = (size_t)g.nx * g.ny;
    for (int z = zbeg; z < zend; ++z) {
        float a, bx, by, d;
        plane_coefficients(cx_, cy_, cz_, planes[z], g, a, bx, by, d);
        uint32_t* plane = H + (size_t)z * plane_sz;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float X = (e[i].x * a + bx) / d;  // :194
            const float Y = (e[i].y * a + by) / d;  // :195
            if (X >= 0.f && Y >= 0.f && X < xmax && Y < ymax) atomicAdd(plane + (size_t)(int)Y * g.nx + (int)X, 1u);  // (see vote_global)
        }
    }
}

hipError_t launch_count_votes(hipStream_t s, const uint16_t* ex, const uint16_t* ey, const uint32_t* packet_first, const float* H9,
                              const float2* lut, int sensor_w, int sensor_h, const float* centers, const float* planes, const Geom& g,
                              int np, uint32_t* H)
{
    if (np <= 0) return hipSuccess;
    const TieEvents ev{ex, ey, packet_first, H9, lut, sensor_w, sensor_h};
    hipLaunchKernelGGL(k_count_votes, dim3(np, (g.nz + kVgPlanes - 1) / kVgPlanes), dim3(256), 0, s, ev, centers, planes, g, H);
    return hipExtGetLastError();
}

// [lo, hi] of the value the REFERENCE holds in a voxel whose engine value is E (exact sum of the weights truncated to the 2^-31
// grid, rounded once to fp32: the LDS-band mappings other than the paired one) and which received n votes.  n u >= 1/2: no bound
// (hi = +inf).
__device__ __forceinline__ void tie_reference_interval(float E, uint32_t n, double* lo, double* hi)
{
    if (n == 0u) {  // no vote: exactly zero in either arithmetic
        *lo = *hi = 0.0;
        return;
    }
    // u = 2^-24; q = n 2^-31: the voting kernels TRUNCATE a weight to the 2^-31 grid (v_cvt_u32_f32), so the sum of the real
    // weights lies between the engine's integer sum and that sum + n 2^-31 (taken on both sides here)
    const double u = 5.9604644775390625e-8, q = (double)n * 4.6566128730773926e-10;
    const double nu = (double)(n - 1u) * u;
    if (!(nu < 0.5)) {
        *lo = 0.0;
        *hi = __builtin_inf();
        return;
    }
    const double gamma = nu / (1.0 - nu);
    const double w_hi = (double)E * (1.0 + 2.0 * u) + q, w_lo = fmax(0.0, (double)E * (1.0 - 2.0 * u) - q);  // the weights' real sum
    *hi = w_hi * (1.0 + gamma);
    *lo = fmax(0.0, w_lo * (1.0 - gamma));
    // E > 0 means the truncated weights sum to at least 2^-31, so ONE weight is at least 2^-31 -- and a sequential fp32 sum of
    // non-negative terms is never below any of them (fl(s + w) >= max(s, w)): the reference's value is not zero either.  Without
    // this floor a column whose maximum is a handful of tiny weights could not even exclude its all-zero planes.
    if (E > 0.f) *lo = fmax(*lo, 1.1641532182693481e-10);  // 2^-33
}

// the fusion op as a real function (monotone non-decreasing in both arguments on [0, inf)); the fp32 chains of fuse_op stay
// within 8 u of it (at most five roundings)
template <int OP>
__device__ __forceinline__ double tie_fuse_real(double a, double g)
{
    if (OP == 0) return a;
    if (OP == 1) return fmin(a, g);
    if (OP == 2) return 2.0 * a * g / (a + g + (double)0.1f);
    if (OP == 3) return sqrt(a * g);
    if (OP == 4) return 0.5 * (a + g);
    if (OP == 5) return sqrt(0.5 * (a * a + g * g));
    return fmax(a, g);
}

__device__ __forceinline__ uint32_t tie_votes_of(const uint32_t* __restrict__ Hz, int x, int y, int nx)
{
    // the votes whose 2 x 2 footprint (xi .. xi + 1, yi .. yi + 1) contains (x, y): integer locations (x - 1 .. x, y - 1 .. y)
    uint32_t n = Hz[(size_t)y * nx + x];
    if (x > 0) n += Hz[(size_t)y * nx + x - 1];
    if (y > 0) n += Hz[(size_t)(y - 1) * nx + x];
    if (x > 0 && y > 0) n += Hz[(size_t)(y - 1) * nx + x - 1];
    return n;
}

// stats: [0] columns proven, [1] columns with a plane below the threshold that the bounds cannot exclude, [2] float bits of the
// largest (maximum - value) / maximum among those planes (the rel_gap that would have taken them all in), [3] most votes in a voxel,
// [4] entries of unproven[] (pixel, float bits of the gap the column needs)
template <int OP>
__global__ __launch_bounds__(256) void k_tie_prove(const float* __restrict__ a, const float* __restrict__ b,
                                                   const uint32_t* __restrict__ Ha, const uint32_t* __restrict__ Hb, int nx, int ny,
                                                   int nz, float rel_gap, unsigned* __restrict__ stats, uint2* __restrict__ unproven)
{
    __shared__ unsigned s_stats[4];
    if (threadIdx.x < 4) s_stats[threadIdx.x] = 0u;
    __syncthreads();
    const int npix = nx * ny;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) {
        const int y = p / nx, x = p - y * nx;
        // the engine's arg-max: first maximum of the fused exact values (k_collapse_max_z<Fuse2> / k_tie_columns)
        float best = tie_value<OP>(a, b, p);
        int zbest = 0;
        for (int z = 1; z < nz; ++z) {
            const float v = tie_value<OP>(a, b, (size_t)z * npix + p);
            if (best < v) {
                best = v;
                zbest = z;
            }
        }
        bool proven = true;
        float need = 0.f;
        unsigned most = 0u;
        if (best > 0.f) {  // (an empty column is exactly zero in either summation order)
            const float thr = best - rel_gap * best;  // k_tie_columns / k_tie_contenders
            const double c8 = 8.0 * 5.9604644775390625e-8;
            double lo0, hi0, lo1 = 0.0, hi1 = 0.0;
            {
                const size_t i = (size_t)zbest * npix + p;
                const uint32_t n0 = tie_votes_of(Ha + (size_t)zbest * npix, x, y, nx);
                tie_reference_interval(a[i], n0, &lo0, &hi0);
                most = n0;
                if (OP != 0) {
                    const uint32_t n1 = tie_votes_of(Hb + (size_t)zbest * npix, x, y, nx);
                    tie_reference_interval(b[i], n1, &lo1, &hi1);
                    most = max(most, n1);
                }
            }
            const double winner_lo = tie_fuse_real<OP>(lo0, lo1) * (1.0 - c8);
            for (int z = 0; z < nz; ++z) {
                const size_t i = (size_t)z * npix + p;
                const float v = tie_value<OP>(a, b, i);
                if (v >= thr) continue;  // within the gap: re-summed in the reference's order by the resolver (or the maximum itself)
                const uint32_t n0 = tie_votes_of(Ha + (size_t)z * npix, x, y, nx);
                double l0, h0, l1 = 0.0, h1 = 0.0;
                tie_reference_interval(a[i], n0, &l0, &h0);
                most = max(most, n0);
                if (OP != 0) {
                    const uint32_t n1 = tie_votes_of(Hb + (size_t)z * npix, x, y, nx);
                    tie_reference_interval(b[i], n1, &l1, &h1);
                    most = max(most, n1);
                }
                const double upper = tie_fuse_real<OP>(h0, h1) * (1.0 + c8);
                if (!(upper < winner_lo)) {  // cannot be excluded (strictly below: an equal value at a lower plane would win)
                    proven = false;
                    need = fmaxf(need, (best - v) / best);
                }
            }
        }
        atomicAdd(&s_stats[proven ? 0 : 1], 1u);
        if (!proven) {
            atomicMax(&s_stats[2], __float_as_uint(need));  // (non-negative floats order like their bits)
            // the column and the gap it needs, for callers that treat the few hard columns one by one (room for every pixel)
            if (unproven) unproven[atomicAdd(&stats[4], 1u)] = make_uint2((unsigned)p, __float_as_uint(need));
        }
        atomicMax(&s_stats[3], most);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
    if (threadIdx.x >= 2 && threadIdx.x < 4 && s_stats[threadIdx.x]) atomicMax(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// votes[i] <- the votes of voxel vox[i] (z * ny * nx + y * nx + x) according to the counters H (tie_votes_of)
__global__ __launch_bounds__(256) void k_tie_votes_of(const uint32_t* __restrict__ H, const uint32_t* __restrict__ vox, int n, int nx, int ny,
                                                      uint32_t* __restrict__ votes)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = vox[i], npix = (uint32_t)nx * (uint32_t)ny;
    const uint32_t z = v / npix, p = v - z * npix, y = p / (uint32_t)nx, x = p - y * (uint32_t)nx;
    votes[i] = tie_votes_of(H + (size_t)z * npix, (int)x, (int)y, nx);
}

hipError_t launch_tie_votes_of(hipStream_t s, const uint32_t* H, const uint32_t* vox, int n, int nx, int ny, uint32_t* votes)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tie_votes_of, dim3((n + 255) / 256), dim3(256), 0, s, H, vox, n, nx, ny, votes);
    return hipExtGetLastError();
}

// ---- the proof's pieces for ANY fusion topology (Alg. 2's camera-then-time fusion, process2.cpp:98-249): INTERVAL GRIDS ----
// lo / hi: two fp32 volumes that enclose, voxel by voxel, the value the reference holds -- made per camera DSI from the
// counted votes (k_interval_of_counts), carried through the SAME device ops the engine applies to the values (every one of the
// reference's voxel-wise ops is monotone non-decreasing in its operands, or the decreasing 1 / (0.01 + g) inside the harmonic
// accumulation whose final n / sum turns it around), widened after every step by that step's roundings (k_interval_widen),
// and finally compared column by column (k_prove_columns) like k_tie_prove does.
// (the next fp32 below / above a FINITE f, by its bits: there is no nextafterf on the device)
__device__ __forceinline__ float next_below(float f)
{
    const uint32_t b = __float_as_uint(f);
    if (f > 0.f) return __uint_as_float(b - 1u);
    if (f < 0.f) return __uint_as_float(b + 1u);
    return __uint_as_float(0x80000001u);  // -min denormal
}
__device__ __forceinline__ float next_above(float f)
{
    const uint32_t b = __float_as_uint(f);
    if (f > 0.f) return __uint_as_float(b + 1u);  // (max finite -> +inf: a bound that says nothing, correctly)
    if (f < 0.f) return __uint_as_float(b - 1u);
    return __uint_as_float(0x00000001u);
}
__device__ __forceinline__ float round_down(double v)
{
    const float f = (float)v;  // (round to nearest; v = +-inf or NaN pass through)
    if (f == __builtin_inff() && v < (double)__builtin_inff()) return 3.4028234663852886e38f;  // (a finite v beyond FLT_MAX)
    return ((double)f > v && f == f && fabsf(f) < __builtin_inff()) ? next_below(f) : f;
}
__device__ __forceinline__ float round_up(double v)
{
    const float f = (float)v;
    return ((double)f < v && f == f && fabsf(f) < __builtin_inff()) ? next_above(f) : f;
}

__global__ __launch_bounds__(256) void k_interval_of_counts(const float* __restrict__ dsi, const uint32_t* __restrict__ H, int nx, int ny,
                                                            int nz, float* __restrict__ lo, float* __restrict__ hi,
                                                            unsigned* __restrict__ most)
{
    const size_t npix = (size_t)nx * ny, n = npix * nz;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned votes = 0u;
    if (i < n) {
        const size_t z = i / npix, p = i - z * npix;
        const int y = (int)(p / nx), x = (int)(p - (size_t)y * nx);
        votes = tie_votes_of(H + z * npix, x, y, nx);
        double l, h;
        tie_reference_interval(dsi[i], votes, &l, &h);
        lo[i] = round_down(l);
        hi[i] = round_up(h);  // (+inf where a voxel has 2^23 votes or more: never proven)
    }
    // (most votes in a voxel: one atomic per wave)
    for (int off = 32; off > 0; off >>= 1) votes = max(votes, (unsigned)__shfl_xor((int)votes, off, 64));
    if ((threadIdx.x & 63) == 0 && votes) atomicMax(most, votes);
}

// lo <- lo (1 - k u) rounded down (never below 0), hi <- hi (1 + k u) rounded up: the k roundings of the step just applied
__global__ __launch_bounds__(256) void k_interval_widen(float* __restrict__ lo, float* __restrict__ hi, size_t n, double ku)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lo[i] = round_down(fmax(0.0, (double)lo[i] * (1.0 - ku)));
    hi[i] = round_up((double)hi[i] * (1.0 + ku));
}

// per column of `fused` (the engine's values: the resolver's threshold comes from them): every plane below
// best - rel_gap * best must have hi strictly below lo of the maximum's plane.  stats / unproven as k_tie_prove
__global__ __launch_bounds__(256) void k_prove_columns(const float* __restrict__ fused, const float* __restrict__ lo,
                                                       const float* __restrict__ hi, int npix, int nz, float rel_gap,
                                                       unsigned* __restrict__ stats, uint2* __restrict__ unproven)
{
    __shared__ unsigned s_stats[3];
    if (threadIdx.x < 3) s_stats[threadIdx.x] = 0u;
    __syncthreads();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) {
        float best = fused[p];
        int zbest = 0;
        for (int z = 1; z < nz; ++z) {
            const float v = fused[(size_t)z * npix + p];
            if (best < v) {
                best = v;
                zbest = z;
            }
        }
        bool proven = true;
        float need = 0.f;
        if (best > 0.f) {
            const float thr = best - rel_gap * best;
            const float winner_lo = lo[(size_t)zbest * npix + p];
            for (int z = 0; z < nz; ++z) {
                const size_t i = (size_t)z * npix + p;
                const float v = fused[i];
                if (v >= thr) continue;
                if (!(hi[i] < winner_lo)) {
                    proven = false;
                    need = fmaxf(need, (best - v) / best);
                }
            }
        }
        atomicAdd(&s_stats[proven ? 0 : 1], 1u);
        if (!proven) {
            atomicMax(&s_stats[2], __float_as_uint(need));
            if (unproven) unproven[atomicAdd(&stats[4], 1u)] = make_uint2((unsigned)p, __float_as_uint(need));
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
    if (threadIdx.x == 2 && s_stats[2]) atomicMax(&stats[2], s_stats[2]);
}

hipError_t launch_interval_of_counts(hipStream_t s, const float* dsi, const uint32_t* H, int nx, int ny, int nz, float* lo, float* hi,
                                     unsigned* most)
{
    const size_t n = (size_t)nx * ny * nz;
    hipLaunchKernelGGL(k_interval_of_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dsi, H, nx, ny, nz, lo, hi, most);
    return hipExtGetLastError();
}

hipError_t launch_interval_widen(hipStream_t s, float* lo, float* hi, size_t n, int roundings)
{
    hipLaunchKernelGGL(k_interval_widen, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lo, hi, n,
                       (double)roundings * 5.9604644775390625e-8);
    return hipExtGetLastError();
}

hipError_t launch_prove_columns(hipStream_t s, const float* fused, const float* lo, const float* hi, int npix, int nz, float rel_gap,
                                unsigned* stats5, uint2* unproven)
{
    hipLaunchKernelGGL(k_prove_columns, dim3((npix + 255) / 256), dim3(256), 0, s, fused, lo, hi, npix, nz, rel_gap, stats5, unproven);
    return hipExtGetLastError();
}

// ---- the same proof for n cameras fused by an n-ary mode (dsi_mapper_prove_near_ties_n: BASELINE configs[4]'s rig) ----
// fused: the grid the n-ary resolver took its near-tie columns from (dsi_grid_near_tie_voxels: the engine's fused values);
// e[c] / h[c]: camera c's DSI and vote counters.  MODE: DSI_ACC_GM_TREE (6; n = 2, 4, 8: the balanced tree of the
// reference's 2-ary sqrt(a * b), cartesian3dgrid.h:150-156), DSI_ACC_MIN (4), DSI_ACC_MAX (5), DSI_ACC_SUM (0: the arithmetic
// mean).  Every one of them is monotone non-decreasing in each camera's value, with at most 2 n + 2 roundings.
struct ProveSources {
    const float* e[8];
    const uint32_t* h[8];
    int n;
};

template <int MODE>
__device__ __forceinline__ double tie_fuse_real_n(const double* v, int n)
{
    if (MODE == 4 || MODE == 5) {
        double r = v[0];
        for (int c = 1; c < n; ++c) r = MODE == 4 ? fmin(r, v[c]) : fmax(r, v[c]);
        return r;
    }
    if (MODE == 0) {
        double r = 0.0;
        for (int c = 0; c < n; ++c) r += v[c];
        return r / (double)n;
    }
    double t[8];
    for (int c = 0; c < n; ++c) t[c] = v[c];
    for (int w = n; w > 1; w >>= 1)
        for (int c = 0; c < w / 2; ++c) t[c] = sqrt(t[2 * c] * t[2 * c + 1]);
    return t[0];
}

template <int MODE>
__global__ __launch_bounds__(256) void k_tie_prove_n(const float* __restrict__ fused, ProveSources src, int nx, int ny, int nz,
                                                     float rel_gap, unsigned* __restrict__ stats, uint2* __restrict__ unproven)
{
    __shared__ unsigned s_stats[4];
    if (threadIdx.x < 4) s_stats[threadIdx.x] = 0u;
    __syncthreads();
    const int npix = nx * ny, n = src.n;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) {
        const int y = p / nx, x = p - y * nx;
        float best = fused[p];
        int zbest = 0;
        for (int z = 1; z < nz; ++z) {
            const float v = fused[(size_t)z * npix + p];
            if (best < v) {
                best = v;
                zbest = z;
            }
        }
        bool proven = true;
        float need = 0.f;
        unsigned most = 0u;
        if (best > 0.f) {
            const float thr = best - rel_gap * best;  // k_tie_columns on the fused grid
            const double slack = (double)(2 * n + 2) * 5.9604644775390625e-8;
            double lo[8], hi[8];
            for (int c = 0; c < n; ++c) {
                const uint32_t votes = tie_votes_of(src.h[c] + (size_t)zbest * npix, x, y, nx);
                tie_reference_interval(src.e[c][(size_t)zbest * npix + p], votes, &lo[c], &hi[c]);
                most = max(most, votes);
            }
            const double winner_lo = tie_fuse_real_n<MODE>(lo, n) * (1.0 - slack);
            for (int z = 0; z < nz; ++z) {
                const size_t i = (size_t)z * npix + p;
                const float v = fused[i];
                if (v >= thr) continue;  // within the gap: re-summed in the reference's order (or the maximum itself)
                for (int c = 0; c < n; ++c) {
                    const uint32_t votes = tie_votes_of(src.h[c] + (size_t)z * npix, x, y, nx);
                    tie_reference_interval(src.e[c][i], votes, &lo[c], &hi[c]);
                    most = max(most, votes);
                }
                const double upper = tie_fuse_real_n<MODE>(hi, n) * (1.0 + slack);
                if (!(upper < winner_lo)) {
                    proven = false;
                    need = fmaxf(need, (best - v) / best);
                }
            }
        }
        atomicAdd(&s_stats[proven ? 0 : 1], 1u);
        if (!proven) {
            atomicMax(&s_stats[2], __float_as_uint(need));
            if (unproven) unproven[atomicAdd(&stats[4], 1u)] = make_uint2((unsigned)p, __float_as_uint(need));
        }
        atomicMax(&s_stats[3], most);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
    if (threadIdx.x >= 2 && threadIdx.x < 4 && s_stats[threadIdx.x]) atomicMax(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

hipError_t launch_tie_prove_n(hipStream_t s, const float* fused, const float* const* e, const uint32_t* const* h, int n, int mode, int nx,
                              int ny, int nz, float rel_gap, unsigned* stats5, uint2* unproven)
{
    if (n < 1 || n > 8) return hipErrorInvalidValue;
    if (mode == 6 && n != 2 && n != 4 && n != 8) return hipErrorInvalidValue;
    ProveSources src{};
    src.n = n;
    for (int c = 0; c < n; ++c) {
        src.e[c] = e[c];
        src.h[c] = h[c];
    }
    const dim3 grid((nx * ny + 255) / 256), block(256);
    switch (mode) {
    case 0: hipLaunchKernelGGL(k_tie_prove_n<0>, grid, block, 0, s, fused, src, nx, ny, nz, rel_gap, stats5, unproven); break;
    case 4: hipLaunchKernelGGL(k_tie_prove_n<4>, grid, block, 0, s, fused, src, nx, ny, nz, rel_gap, stats5, unproven); break;
    case 5: hipLaunchKernelGGL(k_tie_prove_n<5>, grid, block, 0, s, fused, src, nx, ny, nz, rel_gap, stats5, unproven); break;
    case 6: hipLaunchKernelGGL(k_tie_prove_n<6>, grid, block, 0, s, fused, src, nx, ny, nz, rel_gap, stats5, unproven); break;
    default: return hipErrorInvalidValue;
    }
    return hipExtGetLastError();
}

hipError_t launch_tie_prove(hipStream_t s, const float* a, const float* b, const uint32_t* Ha, const uint32_t* Hb, int op, int nx,
                            int ny, int nz, float rel_gap, unsigned* stats4, uint2* unproven)
{
    const dim3 grid((nx * ny + 255) / 256), block(256);
    return dispatch_int<0, 6>(b ? op : 0, [&](auto OP) {
        hipLaunchKernelGGL(k_tie_prove<OP>, grid, block, 0, s, a, b, Ha, Hb, nx, ny, nz, rel_gap, stats4, unproven);
        return hipExtGetLastError();
    });
}

hipError_t launch_tie_candidates(hipStream_t s, const float* a, const float* b, int op, int npix, int nz, float rel_gap,
                                 unsigned* counters, uint32_t* cand, uint32_t cap, uint4* cols, uint32_t cols_cap)
{
    if (nz > 256) return hipErrorInvalidValue;
    const dim3 grid((npix + 255) / 256), block(256);
    const dim3 grid2((unsigned)std::min<size_t>(512, ((size_t)cols_cap + 15) / 16)), block2(1024);
    return dispatch_int<0, 6>(b ? op : 0, [&](auto OP) {
        hipLaunchKernelGGL(k_tie_columns<OP>, grid, block, 0, s, a, b, npix, nz, rel_gap, counters, cols, cols_cap);
        hipLaunchKernelGGL(k_tie_contenders<OP>, grid2, block2, 0, s, a, b, npix, nz, rel_gap, counters, cand, cap, cols, cols_cap);
        return hipExtGetLastError();
    });
}

hipError_t launch_tie_desc(hipStream_t s, const uint32_t* vox, int n, int nx, int npix, uint2* desc, unsigned* plane_bits)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tie_desc, dim3((n + 255) / 256), dim3(256), 0, s, vox, n, nx, npix, desc, plane_bits);
    return hipExtGetLastError();
}

int tie_segment_records() { return kTieSeg; }
int tie_block_capacity_records() { return kTieMaxSegs * kTieSeg; }

hipError_t launch_tie_hits_binned(hipStream_t s, const uint16_t* ex, const uint16_t* ey, const uint32_t* packet_first, const float* H,
                                  const float2* lut, int sensor_w, int sensor_h, const float* centers, const float* planes, const Geom& g,
                                  int np, const uint2* desc, int nsv, unsigned rank_base, unsigned pos_bits, unsigned sentinel_rank,
                                  unsigned* seg_counter, unsigned cap_segs, unsigned* flags, unsigned long long* total_hits,
                                  unsigned long long* keys, float* wts)
{
    const TieEvents ev{ex, ey, packet_first, H, lut, sensor_w, sensor_h};
    if (np <= 0 || nsv <= 0) return hipSuccess;
    const TieBinGeom bg = tie_bin_geom(g.nx, g.ny);
    const size_t lds = tie_hits_lds_bytes(bg.tx_n * bg.ty_n, g.nz);
    if (lds > max_dynamic_lds() || g.nx > 0xffff || g.ny > 0xffff) return hipErrorInvalidValue;
    constexpr int kHitsBlock = 512;  // 8 waves per block, <= 64 VGPRs: up to 32 waves per CU next to four blocks' LDS
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(k_tie_hits_binned<kHitsBlock>), lds)) return e;
    // blocks take packets in turn (the order of the hits does not matter: they are sorted); as many as fit the chip
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, max_dynamic_lds() / lds));
    const int blocks = std::min(np, 256 * per_cu);
    // ... and when the packets alone do not (a 50 ms window), the voxels are dealt over blockIdx.y (each share bins the packet again)
    int vshares = std::max(1, std::min(std::min(16, (nsv + 1023) / 1024), (256 * per_cu) / blocks));
    vshares = std::max(vshares, (nsv + (1 << 22) - 1) >> 22);  // (a queue entry holds the voxel's index within its share in 22 bits)
    hipLaunchKernelGGL(k_tie_hits_binned<kHitsBlock>, dim3(blocks, vshares), dim3(kHitsBlock), lds, s, ev, centers, planes, g, np, desc, nsv, rank_base, pos_bits,
                       sentinel_rank, bg, seg_counter, cap_segs, flags, total_hits, keys, wts);
    return hipExtGetLastError();
}


// the recorded votes [0, n_rec) partitioned by rank into runs[starts[r] .. starts[r] + counts[r]) (any order inside a run;
// a word = event position << 32 | weight bits), then exact[] / count[] / diff[] (dsi_kernels.h).  n_ranks =
// n_cams * nsv; counts, cursor: n_ranks words, starts: n_ranks + 1 (scratch).  pos_bits <= 32, n_rec < 2^32.
size_t tie_partition_cursor_words(size_t n_ranks)
{
    return n_ranks <= (size_t)kTiePartLdsRanks ? n_ranks * (size_t)kTiePartStretches : n_ranks;
}

hipError_t launch_tie_partition_sums(hipStream_t s, const unsigned long long* keys, const float* wts, unsigned long long n_rec,
                                     unsigned pos_bits, uint32_t* counts, uint32_t* starts, uint32_t* cursor, unsigned long long* runs,
                                     const uint32_t* vox, int nsv, int n_cams, const float* grid0, const float* grid1, float* exact,
                                     uint32_t* count, float* diff)
{
    const unsigned n_ranks = (unsigned)nsv * (unsigned)n_cams;
    if (n_ranks == 0) return hipSuccess;
    if (pos_bits > 32u || n_rec >= (1ull << 32)) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_ranks * sizeof(uint32_t), s)) return e;
    if (n_rec) {
        const int use_lds = n_ranks <= (unsigned)kTiePartLdsRanks ? 1 : 0;
        const size_t lds = use_lds ? (size_t)n_ranks * sizeof(uint32_t) : 0;
        // stretches of >= 8 k votes, at most kTiePartStretches of them (one workgroup per CU's worth): a workgroup pays
        // ~n_ranks LDS words per stretch.  LDS path: NO global atomic -- the counting launch leaves its counts in a table
        // [stretch][rank] (`cursor`: tie_partition_cursor_words), k_tie_colscan turns a rank's column into the offsets of
        // the stretches inside its run (17 us), the scattering launch reads its row instead of counting again (with one
        // returning atomic per (stretch, rank) on the runs' cursors -- 256 workgroups walking the ranks in the same order --
        // the scatter took 0.277 ms at configs[1]; now 0.240)
        const unsigned long long per = std::max<unsigned long long>(8192ull, (n_rec + kTiePartStretches - 1ull) / kTiePartStretches);
        const unsigned blocks = (unsigned)((n_rec + per - 1) / per);
        if (use_lds) {
            if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_tie_partition<false>), lds)) return e;
            if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_tie_partition<true>), lds)) return e;
        }
        hipLaunchKernelGGL(k_tie_partition<false>, dim3(blocks), dim3(1024), lds, s, keys, wts, n_rec, per, pos_bits, n_ranks, use_lds,
                           use_lds ? cursor : counts, (const uint32_t*)nullptr, (unsigned long long*)nullptr);
        if (hipError_t e = hipExtGetLastError()) return e;
        if (use_lds) {
            hipLaunchKernelGGL(k_tie_colscan, dim3((n_ranks + 63) / 64), dim3(64), 0, s, cursor, n_ranks, blocks, counts);
            if (hipError_t e = hipExtGetLastError()) return e;
        }
        hipLaunchKernelGGL(k_tie_scan, dim3(1), dim3(1024), 0, s, counts, n_ranks, starts, use_lds ? (uint32_t*)nullptr : cursor);
        if (hipError_t e = hipExtGetLastError()) return e;
        hipLaunchKernelGGL(k_tie_partition<true>, dim3(blocks), dim3(1024), lds, s, keys, wts, n_rec, per, pos_bits, n_ranks, use_lds,
                           cursor, (const uint32_t*)starts, runs);
        if (hipError_t e = hipExtGetLastError()) return e;
    } else {
        hipLaunchKernelGGL(k_tie_scan, dim3(1), dim3(1024), 0, s, counts, n_ranks, starts, cursor);
        if (hipError_t e = hipExtGetLastError()) return e;
    }
    // (the unsorted weights have been consumed by the scatter: their array receives the weights in event order)
    float* sorted_w = const_cast<float*>(wts);
    if (n_rec) {
        hipLaunchKernelGGL(k_tie_sort_runs<1024>, dim3(n_ranks), dim3(256), 0, s, runs, starts, counts, pos_bits, (int)n_ranks, sorted_w);
        if (hipError_t e = hipExtGetLastError()) return e;
        hipLaunchKernelGGL(k_tie_sort_runs<2048>, dim3(n_ranks), dim3(512), 0, s, runs, starts, counts, pos_bits, (int)n_ranks, sorted_w);
        if (hipError_t e = hipExtGetLastError()) return e;
        hipLaunchKernelGGL(k_tie_sort_runs<kTieRunLds>, dim3(n_ranks), dim3(512), 0, s, runs, starts, counts, pos_bits, (int)n_ranks, sorted_w);
        if (hipError_t e = hipExtGetLastError()) return e;
    }
    hipLaunchKernelGGL(k_tie_add_runs, dim3((n_ranks + 15) / 16), dim3(256), 0, s, sorted_w, starts, counts, vox, nsv, n_cams, grid0, grid1,
                       exact, count, diff);
    return hipExtGetLastError();
}

hipError_t launch_tie_pick(hipStream_t s, int op, const uint4* cols, int n_cols, const uint32_t* vox, int nsv, int npix,
                           const float* exact, const uint32_t* count, const float* diff, const float* planes, float* conf,
                           uint8_t* idx, float* depth, unsigned* stats, float rel_gap)
{
    if (n_cols <= 0) return hipSuccess;
    const dim3 grid((n_cols + 255) / 256), block(256);
    return dispatch_int<0, 6>(op, [&](auto OP) {
        hipLaunchKernelGGL(k_tie_pick<OP>, grid, block, 0, s, cols, n_cols, vox, nsv, npix, exact, count, diff, planes, conf, idx,
                           depth, stats, rel_gap);
        return hipExtGetLastError();
    });
}

hipError_t launch_tie_patch(hipStream_t s, const uint32_t* pix, const uint8_t* new_idx, const float* new_conf, int n,
                            const float* planes, float* conf, uint8_t* idx, float* depth)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tie_patch, dim3((n + 255) / 256), dim3(256), 0, s, pix, new_idx, new_conf, n, planes, conf, idx, depth);
    return hipExtGetLastError();
}


// ---- the point cloud: MapperEMVS::getPointcloud (mapper_emvs_stereo.cpp:440-480) ----
// Back-projection of the masked pixels through the virtual camera, compacted in row-major pixel order (PCL's push_back
// order), then PCL's RadiusOutlierRemoval restated as a count: point i is kept iff at least need = min_neighbors + 1
// points j (j = i and duplicates included) have (double) d2_f32(i, j) <= (double) r * (double) r, with
// d2_f32 = ((dx*dx) + dy*dy) + dz*dz in fp32 without FMA (FLANN's L2_Simple<float> over x, y, z).
// The count runs over a uniform grid of cells of edge h = r (1 + 2^-10), hashed into a power-of-two number of buckets:
//   * an fp32-accepted pair has |xi - xj| <= r (1 + 2^-23) < h (each fp32 term is <= the rounded sum), so their cells differ
//     by at most one per axis -- the 27-cell neighbourhood holds every pair the test can accept;
//   * the cell coordinate floor(x / h) is taken in double and clamped to +-kPcCellMax: below the clamp the quotient's rounding
//     (<= 2^-32) is far inside the 2^-11 margin, beyond it far-away points share the boundary cell (more candidates, never
//     fewer); NaN lands in a boundary cell and is never within the radius of anything;
//   * a candidate of a visited bucket counts only if its OWN cell is the visited cell: hash collisions, and two neighbour
//     cells that share a bucket, cannot count a point twice or count a point of a cell outside the neighbourhood.
// The bucket fill uses atomics (the order inside a bucket varies); the keep flags do not depend on it.  Both compactions
// are a per-block count, a scan and a scatter: deterministic.  No kernel here uses scratch memory (tests audit it).
namespace {

constexpr int kPcBlock = 256;      // threads per workgroup of every k_pc_ kernel
constexpr int kPcScanTile = 1024;  // elements per workgroup of the scan kernels (4 per thread)
constexpr int kPcCellMax = (1 << 20) - 2;  // |cell coordinate| <= kPcCellMax: 21 bits per axis with the +-1 neighbours

__device__ inline uint32_t pc_wave_inclusive(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive prefix of v over the workgroup (kPcBlock threads, all of them call); *total: the workgroup's sum
__device__ inline uint32_t pc_block_exclusive(uint32_t v, uint32_t* total)
{
    __shared__ uint32_t wsum[kPcBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = pc_wave_inclusive(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < kPcBlock / 64; ++k) {
        const uint32_t s = wsum[k];
        before += k < w ? s : 0u;
        sum += s;
    }
    __syncthreads();  // (wsum is reused by the next call)
    *total = sum;
    return before + inc - v;
}

__device__ inline int pc_cell(float v, double inv_h)
{
    const double q = floor((double)v * inv_h);
    return (int)fmin(fmax(q, (double)-kPcCellMax), (double)kPcCellMax);
}

__device__ inline unsigned long long pc_key(int cx, int cy, int cz)
{
    return (unsigned long long)(cx + kPcCellMax + 1) | ((unsigned long long)(cy + kPcCellMax + 1) << 21) |
           ((unsigned long long)(cz + kPcCellMax + 1) << 42);
}

__device__ inline uint32_t pc_hash(unsigned long long k, uint32_t bmask)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & bmask;
}

// blk[b] = number of flags > 0 in [b * kPcBlock, (b + 1) * kPcBlock) of the first n
__global__ void __launch_bounds__(kPcBlock) k_pc_flag_count(const uint8_t* __restrict__ flag, uint32_t n, uint32_t* __restrict__ blk)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    const bool f = i < n && flag[i] > 0;
    uint32_t total;
    (void)pc_block_exclusive(f ? 1u : 0u, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// exclusive scan of a[0, L) in place, a[L] = the sum: tile sums, their scan (one workgroup), then each tile
__global__ void __launch_bounds__(kPcBlock) k_pc_scan_tiles(const uint32_t* __restrict__ a, uint32_t L, uint32_t* __restrict__ tiles)
{
    const size_t base = (size_t)blockIdx.x * kPcScanTile + threadIdx.x * 4;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += base + k < L ? a[base + k] : 0u;
    uint32_t total;
    (void)pc_block_exclusive(s, &total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kPcBlock) k_pc_scan_top(uint32_t* __restrict__ tiles, uint32_t T)
{
    uint32_t carry = 0;
    for (uint32_t base = 0; base < T; base += kPcScanTile) {
        const uint32_t j = base + threadIdx.x * 4;
        uint32_t v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = j + k < T ? tiles[j + k] : 0u;
            s += v[k];
        }
        uint32_t total;
        uint32_t run = carry + pc_block_exclusive(s, &total);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j + k < T) tiles[j + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) tiles[T] = carry;
}

__global__ void __launch_bounds__(kPcBlock) k_pc_scan_apply(uint32_t* __restrict__ a, uint32_t L, const uint32_t* __restrict__ tiles, uint32_t T)
{
    const size_t base = (size_t)blockIdx.x * kPcScanTile + threadIdx.x * 4;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < L ? a[base + k] : 0u;
        s += v[k];
    }
    uint32_t total;
    uint32_t run = tiles[blockIdx.x] + pc_block_exclusive(s, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < L) a[base + k] = run;
        run += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a[L] = tiles[T];
}

// mapper_emvs_stereo.cpp:455-464 in double: projectPixelTo3dRay (geometry_utils.hpp:56-59, float members), Eigen's normalize()
// (squaredNorm, then / sqrt when > 0), b / b[2] * depth; stored as float, intensity = 1.0 / z of the stored z.  IEEE divide and
// square root (no fast-math; -ffp-contract=off).  Point k of the compacted cloud: blk_off[block] + rank inside the block.
__global__ void __launch_bounds__(kPcBlock) k_pc_backproject(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                             int nx, uint32_t npix, float fx, float fy, float cx, float cy,
                                                             const uint32_t* __restrict__ blk_off, float4* __restrict__ pts)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    const bool f = i < npix && mask[i] > 0;
    uint32_t total;
    const uint32_t rank = pc_block_exclusive(f ? 1u : 0u, &total);
    if (!f) return;
    const uint32_t y = i / (uint32_t)nx, x = i - y * (uint32_t)nx;
    double bx = ((double)x - (double)cx) / (double)fx;
    double by = ((double)y - (double)cy) / (double)fy;
    double bz = 1.0;
    const double sq = (bx * bx + by * by) + bz * bz;
    if (sq > 0.0) {
        const double nrm = sqrt(sq);
        bx = bx / nrm;
        by = by / nrm;
        bz = bz / nrm;
    }
    const double d = (double)depth[i];
    const float X = (float)((bx / bz) * d), Y = (float)((by / bz) * d), Z = (float)((bz / bz) * d);
    pts[blk_off[blockIdx.x] + rank] = make_float4(X, Y, Z, (float)(1.0 / (double)Z));
}

// each point's cell key and its slot in its bucket (bcount zeroed by the caller)
__global__ void __launch_bounds__(kPcBlock) k_pc_cells(const float4* __restrict__ pts, const uint32_t* __restrict__ n_dev,
                                                       double inv_h, uint32_t bmask, unsigned long long* __restrict__ key,
                                                       uint32_t* __restrict__ bcount, uint32_t* __restrict__ slot)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    if (i >= *n_dev) return;
    const float4 p = pts[i];
    const unsigned long long k = pc_key(pc_cell(p.x, inv_h), pc_cell(p.y, inv_h), pc_cell(p.z, inv_h));
    key[i] = k;
    slot[i] = atomicAdd(&bcount[pc_hash(k, bmask)], 1u);
}

// counting sort by bucket: bstart = exclusive scan of the bucket counts
__global__ void __launch_bounds__(kPcBlock) k_pc_bucket_scatter(const float4* __restrict__ pts, const unsigned long long* __restrict__ key,
                                                                const uint32_t* __restrict__ slot, const uint32_t* __restrict__ bstart,
                                                                const uint32_t* __restrict__ n_dev, uint32_t bmask,
                                                                float4* __restrict__ spts, unsigned long long* __restrict__ skey)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    if (i >= *n_dev) return;
    const unsigned long long k = key[i];
    const uint32_t pos = bstart[pc_hash(k, bmask)] + slot[i];
    spts[pos] = pts[i];
    skey[pos] = k;
}

// keep[i] = at least `need` points within the radius (the count rule above); keep[i] = 0 for n <= i < n_max
__global__ void __launch_bounds__(kPcBlock) k_pc_count(const float4* __restrict__ pts, const unsigned long long* __restrict__ key,
                                                       const uint32_t* __restrict__ n_dev, uint32_t n_max,
                                                       const uint32_t* __restrict__ bstart, const float4* __restrict__ spts,
                                                       const unsigned long long* __restrict__ skey, uint32_t bmask, double rr,
                                                       uint32_t need, uint8_t* __restrict__ keep)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    if (i >= n_max) return;
    if (i >= *n_dev) {
        keep[i] = 0;
        return;
    }
    const float4 p = pts[i];
    const unsigned long long k = key[i];
    uint32_t cnt = 0;
    for (int dz = -1; dz <= 1 && cnt < need; ++dz)
        for (int dy = -1; dy <= 1 && cnt < need; ++dy)
            for (int dx = -1; dx <= 1 && cnt < need; ++dx) {
                const unsigned long long nb =
                    k + (unsigned long long)((long long)dx + ((long long)dy << 21) + ((long long)dz << 42));
                const uint32_t b = pc_hash(nb, bmask);
                const uint32_t e = bstart[b + 1];
                for (uint32_t j = bstart[b]; j < e; ++j) {
                    if (skey[j] != nb) continue;
                    const float4 q = spts[j];
                    const float ddx = p.x - q.x, ddy = p.y - q.y, ddz = p.z - q.z;
                    const float d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
                    if ((double)d2 <= rr && ++cnt >= need) break;
                }
            }
    keep[i] = cnt >= need ? 1 : 0;
}

// out[blk_off[block] + rank] = pts[i] for every kept i, in input order
__global__ void __launch_bounds__(kPcBlock) k_pc_compact(const float4* __restrict__ pts, const uint8_t* __restrict__ keep, uint32_t n_max,
                                                         const uint32_t* __restrict__ blk_off, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    const bool f = i < n_max && keep[i] > 0;
    uint32_t total;
    const uint32_t rank = pc_block_exclusive(f ? 1u : 0u, &total);
    if (f) out[blk_off[blockIdx.x] + rank] = pts[i];
}

uint32_t pc_blocks(size_t n) { return (uint32_t)((n + kPcBlock - 1) / kPcBlock); }

// exclusive scan of a[0, L) in place with a[L] = the sum; tiles: pc_scan_tile_words(L) words
hipError_t pc_scan(hipStream_t s, uint32_t* a, uint32_t L, uint32_t* tiles)
{
    const uint32_t T = (L + kPcScanTile - 1) / kPcScanTile;  // (L > 0: the callers skip empty inputs)
    hipLaunchKernelGGL(k_pc_scan_tiles, dim3(T), dim3(kPcBlock), 0, s, a, L, tiles);
    hipLaunchKernelGGL(k_pc_scan_top, dim3(1), dim3(kPcBlock), 0, s, tiles, T);
    hipLaunchKernelGGL(k_pc_scan_apply, dim3(T), dim3(kPcBlock), 0, s, a, L, tiles, T);
    return hipExtGetLastError();
}

}  // namespace

size_t pc_block_words(size_t n) { return pc_blocks(n) + 1; }
size_t pc_scan_tile_words(size_t L) { return (L + kPcScanTile - 1) / kPcScanTile + 1; }
uint32_t pc_buckets(size_t n)
{
    uint32_t m = 64;
    while (m < 2 * n) m <<= 1;
    return m;
}

hipError_t launch_pc_backproject(hipStream_t s, const float* depth, const uint8_t* mask, int nx, int ny, float fx, float fy,
                                 float cx, float cy, uint32_t* blk, uint32_t* tiles, float4* pts)
{
    const uint32_t npix = (uint32_t)nx * (uint32_t)ny, nb = pc_blocks(npix);
    hipLaunchKernelGGL(k_pc_flag_count, dim3(nb), dim3(kPcBlock), 0, s, mask, npix, blk);
    hipError_t e = pc_scan(s, blk, nb, tiles);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pc_backproject, dim3(nb), dim3(kPcBlock), 0, s, depth, mask, nx, npix, fx, fy, cx, cy, blk, pts);
    return hipExtGetLastError();
}

hipError_t launch_pc_radius_filter(hipStream_t s, const float4* pts, const uint32_t* n_dev, uint32_t n_max, float radius,
                                   uint32_t need, const PcScratch& w, uint8_t* keep)
{
    if (n_max == 0) return hipSuccess;
    const uint32_t nb = pc_blocks(n_max), M = pc_buckets(n_max), bmask = M - 1;
    const double h = (double)radius * (1.0 + 0x1p-10);  // (exact: 24 + 11 bits)
    const double rr = (double)radius * (double)radius;   // (exact: 48 bits)
    hipError_t e = hipMemsetAsync(w.bstart, 0, (size_t)M * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pc_cells, dim3(nb), dim3(kPcBlock), 0, s, pts, n_dev, 1.0 / h, bmask, w.key, w.bstart, w.slot);
    if ((e = pc_scan(s, w.bstart, M, w.tiles)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_pc_bucket_scatter, dim3(nb), dim3(kPcBlock), 0, s, pts, w.key, w.slot, w.bstart, n_dev, bmask, w.spts, w.skey);
    hipLaunchKernelGGL(k_pc_count, dim3(nb), dim3(kPcBlock), 0, s, pts, w.key, n_dev, n_max, w.bstart, w.spts, w.skey, bmask, rr,
                       need, keep);
    return hipExtGetLastError();
}

hipError_t launch_pc_compact(hipStream_t s, const float4* pts, const uint8_t* keep, uint32_t n_max, uint32_t* blk, uint32_t* tiles,
                             float4* out)
{
    if (n_max == 0) return hipSuccess;
    const uint32_t nb = pc_blocks(n_max);
    hipLaunchKernelGGL(k_pc_flag_count, dim3(nb), dim3(kPcBlock), 0, s, keep, n_max, blk);
    hipError_t e = pc_scan(s, blk, nb, tiles);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pc_compact, dim3(nb), dim3(kPcBlock), 0, s, pts, keep, n_max, blk, out);
    return hipExtGetLastError();
}

// ---- the world map: per-window clouds fused in a voxel hash (include/dsi_engine.h dsi_map_*) ----
// A table of 2^cap_log2 slots, open addressing with linear probing from pc_hash(key); key = pc_key of the point's world
// cell, never 0 (every packed coordinate is >= 1), so 0 marks an empty slot and a zeroed table is an empty map.  Per slot:
// n (u32 points), S[3] (u64 sums of the 32-bit cell fractions), windows (u32 calls that reached the cell) and stamp (the
// serial number of the last such call).  Everything a point does to its slot is an integer atomic, so the state does not
// depend on the order of the threads, on how the points are split into calls or on where the probing put the cell; only
// the slot ORDER does, and extraction sorts that away on the host (the key comes with every cell).
// Arithmetic (double, one rounding per operation, no FMA): X = ((r00 x + r01 y) + r02 z) + t0; q = X / leaf; c = floor(q);
// f = q - c; F = (u64) floor(f * 2^32).  f is exact except for -2^-54 < q < 0, where 1 + q rounds to 1 and F = 2^32: the
// point then counts at the cell's upper face, still inside the closed cell.  Rejected: a non-finite X, Y or Z (q is then
// non-finite too) or |c| > kPcCellMax.  ctr: [0] occupied slots, [1] accepted points, [2] rejected points, [3] != 0 when
// a probe sequence ran through the whole table (the host sizes the table so that it cannot; it is an error, not a hang).
namespace {

struct MapPose {
    double m[12];
};

__device__ inline bool map_axis(double X, double leaf, int* c, unsigned long long* F)
{
    const double q = X / leaf;
    const double cf = floor(q);
    if (!(fabs(cf) <= (double)kPcCellMax)) return false;  // (NaN included)
    const double f = q - cf;
    *c = (int)cf;
    *F = (unsigned long long)floor(f * 4294967296.0);
    return true;
}

// the slot that holds key k, claimed if no slot holds it yet (*fresh); ~0u when every slot holds another key
__device__ inline uint32_t map_slot(unsigned long long* keys, uint32_t mask, unsigned long long k, bool* fresh)
{
    uint32_t h = pc_hash(k, mask);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(&keys[h], 0ull, k);
        if (prev == 0ull || prev == k) {
            *fresh = prev == 0ull;
            return h;
        }
        h = (h + 1u) & mask;
    }
    return ~0u;
}

// rules 1-4 for one float32 point (x, y, z widened to double): the one routine every integrate kernel calls.  *ok: merged into
// its cell; *fresh: that cell is new; *full: no slot left (neither set: the point is rejected by rule 3)
__device__ inline void map_integrate_point(double x, double y, double z, const MapPose& T, double leaf, uint32_t serial, const MapTable& t,
                                           bool* ok, bool* fresh, bool* full)
{
    const double X = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    const double Y = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    const double Z = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
    int cx, cy, cz;
    unsigned long long Fx, Fy, Fz;
    if (map_axis(X, leaf, &cx, &Fx) && map_axis(Y, leaf, &cy, &Fy) && map_axis(Z, leaf, &cz, &Fz)) {
        const uint32_t slot = map_slot(t.keys, (1u << t.cap_log2) - 1u, pc_key(cx, cy, cz), fresh);
        if (slot == ~0u) {
            *full = true;
        } else {
            *ok = true;
            atomicAdd(&t.n[slot], 1u);
            atomicAdd(&t.sums[3 * (size_t)slot + 0], Fx);
            atomicAdd(&t.sums[3 * (size_t)slot + 1], Fy);
            atomicAdd(&t.sums[3 * (size_t)slot + 2], Fz);
            if (atomicExch(&t.stamp[slot], serial) != serial) atomicAdd(&t.windows[slot], 1u);
        }
    }
}

// one thread per point; pts: n points of `stride` floats, x y z first
__global__ void __launch_bounds__(kPcBlock) k_map_integrate(const float* __restrict__ pts, uint32_t stride, uint32_t n, MapPose T,
                                                            double leaf, uint32_t serial, MapTable t, unsigned long long* __restrict__ ctr)
{
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;
    bool ok = false, fresh = false, full = false;
    if (i < n) {
        const float* p = pts + (size_t)i * stride;
        map_integrate_point((double)p[0], (double)p[1], (double)p[2], T, leaf, serial, t, &ok, &fresh, &full);
    }
    // the counters: one atomic per wave and counter (every lane of the workgroup arrives here)
    const unsigned long long b_new = __ballot(fresh), b_ok = __ballot(ok), b_rej = __ballot(i < n && !ok && !full), b_full = __ballot(full);
    if ((threadIdx.x & 63) == 0) {
        if (b_new) atomicAdd(&ctr[0], (unsigned long long)__popcll(b_new));
        if (b_ok) atomicAdd(&ctr[1], (unsigned long long)__popcll(b_ok));
        if (b_rej) atomicAdd(&ctr[2], (unsigned long long)__popcll(b_rej));
        if (b_full) atomicAdd(&ctr[3], (unsigned long long)__popcll(b_full));
    }
}

// every occupied slot of `from` with its state into `to` (zeroed, larger): one thread per old slot, keys are distinct
__global__ void __launch_bounds__(kPcBlock) k_map_rehash(MapTable from, MapTable to, unsigned long long* __restrict__ ctr)
{
    const size_t i = (size_t)blockIdx.x * kPcBlock + threadIdx.x;
    if (i >= ((size_t)1 << from.cap_log2)) return;
    const unsigned long long k = from.keys[i];
    if (k == 0ull) return;
    bool fresh;
    const uint32_t slot = map_slot(to.keys, (1u << to.cap_log2) - 1u, k, &fresh);
    if (slot == ~0u) {
        atomicAdd(&ctr[3], 1ull);
        return;
    }
    to.n[slot] = from.n[i];
    to.windows[slot] = from.windows[i];
    to.stamp[slot] = from.stamp[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) to.sums[3 * (size_t)slot + a] = from.sums[3 * i + a];
}

__device__ inline bool map_passes(const MapTable& t, size_t i, uint32_t min_points, uint32_t min_windows)
{
    return i < ((size_t)1 << t.cap_log2) && t.keys[i] != 0ull && t.n[i] >= min_points && t.windows[i] >= min_windows;
}

// what pc_key packed into key k on axis a: the 21-bit coordinate (an import checks it as it comes), and the cell index it
// stands for
__device__ inline uint32_t pc_packed_of(unsigned long long k, int a) { return (uint32_t)((k >> (21 * a)) & 0x1fffffull); }
__device__ inline int pc_cell_of(unsigned long long k, int a) { return (int)pc_packed_of(k, a) - (kPcCellMax + 1); }

// axis a of the centroid of slot i (key k, n points): m =((double) c + (double) (S / n) * 2^-32) * leaf (the bracket is
// exact: 21 + 32 bits), as float -- the one expression that extraction and rendering share
__device__ inline float map_centroid(const MapTable& t, size_t i, unsigned long long k, uint32_t n, int a, double leaf)
{
    const unsigned long long Q = t.sums[3 * i + a] / (unsigned long long)n;
    return (float)(((double)pc_cell_of(k, a) + (double)Q * 0x1p-32) * leaf);
}

// ---- the map's kernel skeleton: the counted slot walk and the compaction (DESIGN.md 7j "The map's kernel skeleton") ----
// THE COUNTED SLOT WALK.  A kernel that visits every slot and counts what it saw is launched with at most
// kMapRenderMaxBlocks workgroups, which walk the table in strides:
//     MapCounts<N> cnt;                                         (before anything diverges)
//     const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
//     for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) { i = base + threadIdx.x; ... cnt.count<k>(pred); }
//     cnt.flush(ctr);
// The contract: (1) the capacity is a multiple of the workgroup (a power of two >= kPcBlock), so i < cap for every thread
// of every round (at most 2^27 / (1024 * 256) = 512 rounds) and (2) EVERY lane of a wave reaches every count() of every
// round -- count() is a ballot: no `continue`, no early return and no divergent branch around it.  A wave keeps its N
// counts in uniform registers; flush() adds them to LDS once per wave and the workgroup issues ONE global atomic per
// non-zero counter.  One thread per slot with one global atomic per wave and counter was bound by exactly those atomics
// -- 98 k of them on one cache line for a table of 2^21 slots, at the 83 per microsecond one line takes.
// Kernels that walk something else than slots (pixels, incoming cells) keep (2) and guard the element instead of (1).
constexpr uint32_t kMapRenderMaxBlocks = 1024;

template <int N>
struct MapCounts {
    uint32_t c[N] = {};  // the counts (the same in every lane of a wave)
    uint32_t t[N] = {};  // the per-thread sums

    static __device__ __forceinline__ uint32_t* lds()
    {
        __shared__ uint32_t s_cnt[N];
        return s_cnt;
    }
    // by every thread of the workgroup; a kernel's own LDS words zeroed before this are covered by the same barrier
    __device__ __forceinline__ MapCounts()
    {
        if (threadIdx.x < N) lds()[threadIdx.x] = 0u;
        __syncthreads();
    }
    template <int K>
    __device__ __forceinline__ void count(bool pred)
    {
        static_assert(K >= 0 && K < N, "no such counter");
        c[K] += (uint32_t)__popcll(__ballot(pred));
    }
    // counter K as a per-THREAD sum instead of a count (the workgroup's total must stay below 2^32); a counter is fed by
    // count<K> or by sum<K>, not by both.  The sums live here, not in a local of the kernel beside this object: with
    // k_map_pca's members in such a local the compiler kept all eight counts in vector registers, and the kernel lost a wave
    template <int K>
    __device__ __forceinline__ void sum(uint32_t v)
    {
        static_assert(K >= 0 && K < N, "no such counter");
        t[K] += v;
    }
    // the LDS stage; after it every thread may read the workgroup's totals
    __device__ __forceinline__ const uint32_t* stage()
    {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (t[k]) atomicAdd(&lds()[k], t[k]);  // (a counter that is never summed costs nothing: its t is the constant 0)
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (c[k]) atomicAdd(&lds()[k], c[k]);
        }
        __syncthreads();
        return lds();
    }
    // the workgroup's total of counter k, for every thread once a flush has staged it
    __device__ __forceinline__ uint32_t total(int k) const { return lds()[k]; }
    // counter k into ctr[k]
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ ctr)
    {
        const uint32_t* s = stage();
        if (threadIdx.x < N && s[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)s[threadIdx.x]);
    }
    // counter k into *dst[k], thread k's atomic (the indices are compile-time constants: dst stays in registers)
    __device__ __forceinline__ void flush_to(unsigned long long* const (&dst)[N])
    {
        const uint32_t* s = stage();
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)N; ++k)
            if (threadIdx.x == k && s[k]) atomicAdd(dst[k], (unsigned long long)s[k]);
    }
};

// THE COMPACTION.  Output place blk_off[tile] + rank for every slot that keep(i) keeps, in slot order: blk_off is the
// scanned count per tile of kPcBlock slots (k_map_flag_count's, or a kernel's that counts the same predicate), the rank
// comes from pc_block_exclusive, which EVERY thread of the workgroup calls EVERY round (it holds barriers), and
// write(i, at) copies the slot's row.  Walks the 2^cap_log2 slots in strides; ONE_ROUND is for the kernels that are launched
// with one workgroup per tile: the same round without the loop around it and without its test of base (the grid is the
// tiles, and map_passes tests i against the capacity); with the loop k_map_extract's call took 6 % longer on 827,644 cells.
template <bool ONE_ROUND = false, typename Keep, typename Write>
__device__ __forceinline__ void map_compact(uint32_t cap_log2, const uint32_t* __restrict__ blk_off, Keep keep, Write write)
{
    const size_t cap = (size_t)1 << cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; ONE_ROUND || base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool f = keep(i);
        uint32_t total;
        const uint32_t rank = pc_block_exclusive(f ? 1u : 0u, &total);
        if (f) write(i, (size_t)blk_off[base / kPcBlock] + rank);
        if (ONE_ROUND) break;
    }
}

// blk[b] = number of slots in [b * kPcBlock, (b + 1) * kPcBlock) that hold a cell passing the filter
__global__ void __launch_bounds__(kPcBlock) k_map_flag_count(MapTable t, uint32_t min_points, uint32_t min_windows, uint32_t* __restrict__ blk)
{
    const bool f = map_passes(t, (size_t)blockIdx.x * kPcBlock + threadIdx.x, min_points, min_windows);
    uint32_t total;
    (void)pc_block_exclusive(f ? 1u : 0u, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// cell blk_off[block] + rank of the output, in slot order: centroid (map_centroid) per axis
__global__ void __launch_bounds__(kPcBlock) k_map_extract(MapTable t, uint32_t min_points, uint32_t min_windows, double leaf,
                                                          const uint32_t* __restrict__ blk_off, float* __restrict__ xyz,
                                                          uint32_t* __restrict__ n_out, uint32_t* __restrict__ w_out,
                                                          unsigned long long* __restrict__ key_out)
{
    map_compact<true>(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, min_points, min_windows); },
        [&](size_t i, size_t o) {
            const unsigned long long k = t.keys[i];
            const uint32_t n = t.n[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) xyz[3 * o + a] = map_centroid(t, i, k, n, a, leaf);
            n_out[o] = n;
            w_out[o] = t.windows[i];
            key_out[o] = k;
        });
}

// The map as a pinhole camera at v.T (world -> view) sees it: a pass over the table's SLOTS, no compaction.  A cell that
// passes the filter is its extracted centroid (float, widened to double); X = ((r00 x + r01 y) + r02 z) + t0 and Y, Z
// alike; CLIPPED when X, Y or Z is not finite or not min_depth <= Z <= max_depth (NaN fails); u = (fx * (X / Z)) + cx,
// iu = floor(u + 0.5), v / iv alike; the footprint is the (2 splat + 1)^2 pixels around (iu, iv), each tested against the
// image on its own; OUTSIDE when none is inside.  Per footprint pixel: hits += 1 and
// zkey = min(zkey, bits((float) Z) << 32 | ~windows) -- Z > 0, so the bits order as the value; equal float depths go to
// the cell seen by more windows.  zkey starts at all ones, hits at 0 (the host's two memsets).  Integer atomics on
// initialised words only: the image depends neither on the thread order nor on the table's size nor on the probing.
// ctr: [0] cells that passed the filter, [1] clipped, [2] outside, [3] drawn.
// The image tests are made in double before anything becomes an integer: iu + dx with |dx| <= splat <= 4 is inside
// [0, width) for some dx iff -splat <= iu <= width - 1 + splat, which huge, infinite and NaN values fail; past that test
// iu is an integer in [-4, 2^26 + 3] and the per-pixel tests are exact in int.
// A counted slot walk (MapCounts).
__global__ void __launch_bounds__(kPcBlock) k_map_render(MapTable t, MapView v, double leaf, unsigned long long* __restrict__ zkey,
                                                         uint32_t* __restrict__ hits, unsigned long long* __restrict__ ctr)
{
    MapCounts<4> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool f = map_passes(t, i, v.min_points, v.min_windows);
        bool clipped = false, outside = false;
        if (f) {
            const unsigned long long k = t.keys[i];
            const uint32_t n = t.n[i];
            const double x = (double)map_centroid(t, i, k, n, 0, leaf), y = (double)map_centroid(t, i, k, n, 1, leaf),
                         z = (double)map_centroid(t, i, k, n, 2, leaf);
            const double X = ((v.T[0] * x + v.T[1] * y) + v.T[2] * z) + v.T[3];
            const double Y = ((v.T[4] * x + v.T[5] * y) + v.T[6] * z) + v.T[7];
            const double Z = ((v.T[8] * x + v.T[9] * y) + v.T[10] * z) + v.T[11];
            if (!(isfinite(X) && isfinite(Y) && Z >= v.min_depth && Z <= v.max_depth)) {  // (min/max_depth are finite)
                clipped = true;
            } else {
                const double du = floor(((v.fx * (X / Z)) + v.cx) + 0.5), dv = floor(((v.fy * (Y / Z)) + v.cy) + 0.5);
                const double s = (double)v.splat;
                if (!(du >= -s && du <= (double)(v.width - 1) + s && dv >= -s && dv <= (double)(v.height - 1) + s)) {
                    outside = true;
                } else {
                    const int iu = (int)du, iv = (int)dv;
                    const unsigned long long key =
                        ((unsigned long long)__float_as_uint((float)Z) << 32) | (unsigned long long)(0xffffffffu - t.windows[i]);
                    const int y0 = max(iv - v.splat, 0), y1 = min(iv + v.splat, v.height - 1);
                    const int x0 = max(iu - v.splat, 0), x1 = min(iu + v.splat, v.width - 1);
                    for (int py = y0; py <= y1; ++py)
                        for (int px = x0; px <= x1; ++px) {
                            const size_t p = (size_t)py * (size_t)v.width + (size_t)px;
                            atomicMin(&zkey[p], key);
                            atomicAdd(&hits[p], 1u);
                        }
                }
            }
        }
        cnt.count<0>(f);
        cnt.count<1>(clipped);
        cnt.count<2>(outside);
        cnt.count<3>(f && !clipped && !outside);
    }
    cnt.flush(ctr);
}

// the winner's key unpacked per pixel -- depth = (float) Z and windows where hits > 0, zeros elsewhere, mask = hits > 0;
// ctr[4] += covered pixels.  MapCounts' walk over pixels: i is tested against npix, every lane reaches the count.
__global__ void __launch_bounds__(kPcBlock) k_map_render_finish(const unsigned long long* __restrict__ zkey,
                                                                const uint32_t* __restrict__ hits, uint32_t npix,
                                                                float* __restrict__ depth, uint32_t* __restrict__ windows,
                                                                uint8_t* __restrict__ mask, unsigned long long* __restrict__ ctr)
{
    MapCounts<1> cnt;
    const uint32_t stride = gridDim.x * kPcBlock;  // (<= 2^18; npix <= 2^26: base cannot wrap)
    for (uint32_t base = blockIdx.x * kPcBlock; base < npix; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool covered = false;
        if (i < npix) {
            covered = hits[i] > 0u;
            const unsigned long long k = zkey[i];
            depth[i] = covered ? __uint_as_float((uint32_t)(k >> 32)) : 0.f;
            windows[i] = covered ? 0xffffffffu - (uint32_t)k : 0u;
            mask[i] = covered ? 1 : 0;
        }
        cnt.count<0>(covered);
    }
    cnt.flush(ctr + 4);
}

// ---- the map scored in 3-D (include/dsi_map_eval.h dsx_map_*; DESIGN.md 7j "Scoring the map in 3-D") ----
// A depth image as one integrate call: one thread per pixel.  A pixel (u, v) is integrated iff mask is NULL or mask > 0,
// and d is finite and min_depth <= d <= max_depth (in double; NaN fails); its float32 point is
// x = (float) ((((double) u - cx) / fx) * (double) d), y alike, z = d, which goes through map_integrate_point: the call
// is dsi_map_integrate of that point list, bit for bit.  ctr as k_map_integrate's, counted by MapCounts (one round: one
// global atomic per workgroup and counter).
__global__ void __launch_bounds__(kPcBlock) k_map_integrate_depth(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                  MapDepthImage g, MapPose T, double leaf, uint32_t serial, MapTable t,
                                                                  unsigned long long* __restrict__ ctr)
{
    MapCounts<4> cnt;
    const uint32_t i = blockIdx.x * kPcBlock + threadIdx.x;  // (npix <= 2^26)
    bool in = false, ok = false, fresh = false, full = false;
    if (i < g.npix && (mask == nullptr || mask[i] > 0)) {
        const float df = depth[i];
        const double d = (double)df;
        if (isfinite(d) && d >= g.min_depth && d <= g.max_depth) {
            in = true;
            const uint32_t v = i / g.width, u = i - v * g.width;
            const float x = (float)((((double)u - g.cx) / g.fx) * d);
            const float y = (float)((((double)v - g.cy) / g.fy) * d);
            map_integrate_point((double)x, (double)y, d, T, leaf, serial, t, &ok, &fresh, &full);
        }
    }
    cnt.count<0>(fresh);
    cnt.count<1>(ok);
    cnt.count<2>(in && !ok && !full);
    cnt.count<3>(full);
    cnt.flush(ctr);
}

// the slot of `keys` that holds k, ~0u when none does: read-only, from pc_hash(k) until the key or an empty slot, at
// most capacity probes (a table without an empty slot ends the loop, it cannot hang)
__device__ inline uint32_t map_find(const unsigned long long* __restrict__ keys, uint32_t mask, unsigned long long k)
{
    uint32_t h = pc_hash(k, mask);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long kk = keys[h];
        if (kk == k) return h;
        if (kk == 0ull) return ~0u;
        h = (h + 1u) & mask;
    }
    return ~0u;
}

// THE CANDIDATE SWEEP.  The point p against table t (mask = capacity - 1): per axis c = floor(p / leaf); the candidates
// are the cells that pass the filter at c + o, |o| <= reach per axis, an index with |c + o| > kPcCellMax skipped (tested
// in double, NaN included: a huge or non-finite c has no candidates) and the cell with key `self` (0: none) left out --
// BEFORE the probe: tested after it, the key stays live over map_find and costs the callers registers and a wave of
// occupancy; q = the candidate's extracted centroid; fn(slot, key, d2) with d2 = ((dx dx) + dy dy) + dz dz.  Every probe
// loop is map_find's: bounded by the capacity.
template <typename F>
__device__ __forceinline__ void map_near_cells(const MapTable& t, uint32_t mask, uint32_t min_points, uint32_t min_windows, double leaf,
                                               int reach, const double (&p)[3], unsigned long long self, F fn)
{
    double c[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) c[ax] = floor(p[ax] / leaf);
    for (int oz = -reach; oz <= reach; ++oz) {
        const double vz = c[2] + (double)oz;
        if (!(fabs(vz) <= (double)kPcCellMax)) continue;  // (NaN included)
        for (int oy = -reach; oy <= reach; ++oy) {
            const double vy = c[1] + (double)oy;
            if (!(fabs(vy) <= (double)kPcCellMax)) continue;
            for (int ox = -reach; ox <= reach; ++ox) {
                const double vx = c[0] + (double)ox;
                if (!(fabs(vx) <= (double)kPcCellMax)) continue;
                const unsigned long long kb = pc_key((int)vx, (int)vy, (int)vz);
                __builtin_assume(kb != 0ull);  // (every packed coordinate is >= 1: with self == 0 the test below costs nothing)
                if (kb == self) continue;
                const uint32_t j = map_find(t.keys, mask, kb);
                if (j == ~0u || !map_passes(t, j, min_points, min_windows)) continue;
                const uint32_t nb = t.n[j];
                const double dx = p[0] - (double)map_centroid(t, j, kb, nb, 0, leaf);
                const double dy = p[1] - (double)map_centroid(t, j, kb, nb, 1, leaf);
                const double dz = p[2] - (double)map_centroid(t, j, kb, nb, 2, leaf);
                fn(j, kb, ((dx * dx) + dy * dy) + dz * dz);
            }
        }
    }
}

// Every cell of `a` that passes a's filter against the cells of `b` that pass b's: p = a's extracted centroid (float,
// widened) swept over b by map_near_cells; the minimum d2 is kept (minima commute: the order of the offsets and of the
// probing does not matter); d = sqrt(min d2), IEEE; MATCHED iff d <= radius (no candidate: d = +inf).  Matched:
// hist[min((int) floor(d / w), n_bins - 1)] += 1, sum_q += (u64) floor((d / radius) * 2^32).  dist[slot] = (float) d or
// +inf.  ctr: [0] matched, [1] unmatched, [2] sum_q.  A counted slot walk (MapCounts) over a's table; the histogram and
// sum_q are accumulated in LDS beside the counts, and a workgroup issues one global atomic per counter and per non-empty
// bin.  Reads the tables, writes dist: a == b is legal.
__global__ void __launch_bounds__(kPcBlock) k_map_compare(MapTable a, MapTable b, MapCompare o, float* __restrict__ dist,
                                                          unsigned long long* __restrict__ hist, unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t s_hist[kMapCompareMaxBins];
    __shared__ unsigned long long s_sum;
    for (int j = threadIdx.x; j < o.n_bins; j += kPcBlock) s_hist[j] = 0u;
    if (threadIdx.x == 0) s_sum = 0ull;
    MapCounts<2> cnt;
    unsigned long long sum_q = 0ull;
    const uint32_t bmask = (1u << b.cap_log2) - 1u;
    const size_t cap = (size_t)1 << a.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool f = map_passes(a, i, o.min_points_a, o.min_windows_a);
        bool matched = false;
        if (f) {
            const unsigned long long k = a.keys[i];
            const uint32_t n = a.n[i];
            double p[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) p[ax] = (double)map_centroid(a, i, k, n, ax, o.leaf_a);
            double best = INFINITY;
            map_near_cells(b, bmask, o.min_points_b, o.min_windows_b, o.leaf_b, o.reach, p, 0ull,
                           [&](uint32_t, unsigned long long, double d2) {
                               if (d2 < best) best = d2;
                           });
            const double d = sqrt(best);
            matched = d <= o.radius;
            dist[i] = matched ? (float)d : INFINITY;
            if (matched) {
                const int bin = (int)fmin(floor(d / o.bin_width), (double)(o.n_bins - 1));  // (bin_width > 0, d >= 0: in range)
                atomicAdd(&s_hist[bin], 1u);
                sum_q += (unsigned long long)floor((d / o.radius) * 4294967296.0);
            }
        }
        cnt.count<0>(matched);
        cnt.count<1>(f && !matched);
    }
    if (sum_q) atomicAdd(&s_sum, sum_q);
    cnt.flush(ctr);
    if (threadIdx.x == 2 && s_sum) atomicAdd(&ctr[2], s_sum);
    for (int j = threadIdx.x; j < o.n_bins; j += kPcBlock)
        if (s_hist[j]) atomicAdd(&hist[j], (unsigned long long)s_hist[j]);
}

// the compare's distances compacted like k_map_extract's cells (same filter, same blk_off): key and dist in slot order
__global__ void __launch_bounds__(kPcBlock) k_map_compare_gather(MapTable t, uint32_t min_points, uint32_t min_windows,
                                                                 const float* __restrict__ dist, const uint32_t* __restrict__ blk_off,
                                                                 float* __restrict__ dist_out, unsigned long long* __restrict__ key_out)
{
    map_compact<true>(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, min_points, min_windows); },
        [&](size_t i, size_t o) {
            dist_out[o] = dist[i];
            key_out[o] = t.keys[i];
        });
}

// ---- pruning the map (include/dsi_map_prune.h dsx_map_prune*; DESIGN.md 7j "Pruning") ----
// Criteria 1-4 for every slot: first[slot] = the first criterion that fails, 0 when none does, kMapPruneEmpty for a slot
// without a cell.  1: n < min_points; 2: windows < min_windows (map_passes with the other bound at 0); 3: max_age >= 0 and
// calls - stamp > max_age (stamp <= calls: the difference is exact in 32 bits); 4: use_box and the extracted centroid
// (map_centroid, float, widened) outside [box_lo, box_hi] on some axis, compared in double (the centroid is finite; the
// bounds may be infinite, never NaN).  ctr[r] += the cells with reason r, r = 1..4.  A counted slot walk (MapCounts).
__global__ void __launch_bounds__(kPcBlock) k_map_prune_reason(MapTable t, MapPrune o, uint8_t* __restrict__ first,
                                                               unsigned long long* __restrict__ ctr)
{
    MapCounts<4> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = kMapPruneEmpty;
        if (map_passes(t, i, 0u, 0u)) {
            r = 0u;
            if (!map_passes(t, i, o.min_points, 0u)) {
                r = 1u;
            } else if (!map_passes(t, i, 0u, o.min_windows)) {
                r = 2u;
            } else if (o.max_age >= 0 && (long long)(o.calls - t.stamp[i]) > o.max_age) {
                r = 3u;
            } else if (o.use_box) {
                const unsigned long long k = t.keys[i];
                const uint32_t n = t.n[i];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double p = (double)map_centroid(t, i, k, n, a, o.leaf);
                    if (p < o.box_lo[a] || p > o.box_hi[a]) r = 4u;
                }
            }
        }
        first[i] = (uint8_t)r;  // (cap is a multiple of the workgroup: i < cap)
        cnt.count<0>(r == 1u);
        cnt.count<1>(r == 2u);
        cnt.count<2>(r == 3u);
        cnt.count<3>(r == 4u);
    }
    cnt.flush(ctr + 1);
}

// Criterion 5 for the cells that survived 1-4, judged on `first` alone (read-only here, so the outcome does not depend on
// the order of the threads: a neighbour that this criterion removes still counts).  The cell's index c comes from its key;
// the neighbours are the OTHER cells at c + o, |o| <= reach per axis, an index with |c + o| > kPcCellMax skipped (it has no
// key); a neighbour supports iff map_find finds it and first[its slot] == 0.  The sweep stops at min_neighbors supporters
// (the count is only compared with that bound).  reason[slot] = 5 with fewer, else 0; every other slot keeps first[slot].
// ctr[0] += kept, ctr[5] += removed here.  A counted slot walk (MapCounts).
__global__ void __launch_bounds__(kPcBlock) k_map_prune_support(MapTable t, MapPrune o, const uint8_t* __restrict__ first,
                                                                uint8_t* __restrict__ reason, unsigned long long* __restrict__ ctr)
{
    MapCounts<2> cnt;
    const uint32_t mask = (1u << t.cap_log2) - 1u;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = first[i];
        if (r == 0u && o.reach > 0) {
            const unsigned long long k = t.keys[i];
            int c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) c[a] = pc_cell_of(k, a);
            uint32_t found = 0;
            for (int oz = -o.reach; oz <= o.reach && found < o.min_neighbors; ++oz) {
                const int vz = c[2] + oz;
                if (abs(vz) > kPcCellMax) continue;
                for (int oy = -o.reach; oy <= o.reach && found < o.min_neighbors; ++oy) {
                    const int vy = c[1] + oy;
                    if (abs(vy) > kPcCellMax) continue;
                    for (int ox = -o.reach; ox <= o.reach && found < o.min_neighbors; ++ox) {
                        const int vx = c[0] + ox;
                        if (abs(vx) > kPcCellMax || (ox == 0 && oy == 0 && oz == 0)) continue;
                        const uint32_t j = map_find(t.keys, mask, pc_key(vx, vy, vz));
                        if (j != ~0u && first[j] == 0u) ++found;
                    }
                }
            }
            if (found < o.min_neighbors) r = 5u;
        }
        reason[i] = (uint8_t)r;
        cnt.count<0>(r == 0u);
        cnt.count<1>(r == 5u);
    }
    cnt.flush_to({&ctr[0], &ctr[5]});
}

// the kept cells (reason 0) of `from` with all their state into `to` (zeroed; keys are distinct, so a claimed slot has one
// writer): k_map_rehash restricted by `reason`, as a counted slot walk (MapCounts).  ctr[0] += the cells moved;
// ctr[3] += cells whose probe sequence ran through the whole of `to` (the host sizes it so that none does).
__global__ void __launch_bounds__(kPcBlock) k_map_prune_rehash(MapTable from, MapTable to, const uint8_t* __restrict__ reason,
                                                               unsigned long long* __restrict__ ctr)
{
    MapCounts<2> cnt;
    const uint32_t mask = (1u << to.cap_log2) - 1u;
    const size_t cap = (size_t)1 << from.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        bool moved = false, full = false;
        if (reason[i] == 0u) {
            bool fresh;
            const uint32_t slot = map_slot(to.keys, mask, from.keys[i], &fresh);
            if (slot == ~0u) {
                full = true;
            } else {
                moved = true;
                to.n[slot] = from.n[i];
                to.windows[slot] = from.windows[i];
                to.stamp[slot] = from.stamp[i];
#pragma unroll
                for (int a = 0; a < 3; ++a) to.sums[3 * (size_t)slot + a] = from.sums[3 * i + a];
            }
        }
        cnt.count<0>(moved);
        cnt.count<1>(full);
    }
    cnt.flush_to({&ctr[0], &ctr[3]});
}

// the classification compacted like k_map_extract's cells under the filter (1, 1) -- every cell --, with its blk_off: key
// and reason in slot order
__global__ void __launch_bounds__(kPcBlock) k_map_prune_gather(MapTable t, const uint8_t* __restrict__ reason,
                                                               const uint32_t* __restrict__ blk_off, uint8_t* __restrict__ reason_out,
                                                               unsigned long long* __restrict__ key_out)
{
    map_compact<true>(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, 1u, 1u); },
        [&](size_t i, size_t o) {
            reason_out[o] = reason[i];
            key_out[o] = t.keys[i];
        });
}

// ---- the map's connected components (include/dsi_map_components.h dsx_map_components*; DESIGN.md 7j "Components") ----
// A lock-free union-find over SLOT indices: parent[slot] = slot for a node (a cell that passes the filter), kMapCompNone
// elsewhere; a component's root is its smallest slot.  The launches are fixed -- init, union, flatten, reduce, two for the
// largest, count -- whatever the table holds.  Every kernel walks the slots in strides; those that count are counted
// slot walks (MapCounts).
//
// init: parent as above; label = all ones, cells = points = 0 (the reduce's atomics meet initialised words);
// ctr[0] += nodes, ctr[1] += occupied slots that are no node.
__global__ void __launch_bounds__(kPcBlock) k_map_comp_init(MapTable t, uint32_t min_points, uint32_t min_windows, MapComponents c,
                                                            unsigned long long* __restrict__ ctr)
{
    MapCounts<2> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool occupied = map_passes(t, i, 0u, 0u), node = occupied && map_passes(t, i, min_points, min_windows);
        c.parent[i] = node ? (uint32_t)i : kMapCompNone;  // (cap is a multiple of the workgroup: i < cap)
        c.label[i] = ~0ull;
        c.cells[i] = 0u;
        c.points[i] = 0ull;
        cnt.count<0>(node);
        cnt.count<1>(occupied && !node);
    }
    cnt.flush(ctr);
}

__device__ inline uint32_t comp_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this thread can see it; halves the path on the way (a parent becomes its own parent)
__device__ inline uint32_t comp_find(uint32_t* parent, uint32_t x)
{
    uint32_t p = comp_load(&parent[x]);
    while (p != x) {
        const uint32_t g = comp_load(&parent[p]);
        if (g != p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// One thread per node and, per node, the POSITIVE half of the connectivity's offsets (the first non-zero of oz, oy, ox is
// positive: 3 / 9 / 13 / 62 lookups at 6 / 18 / 26 / 124), so that every edge is met once; an index with
// |c + o| > kPcCellMax is skipped (it has no key).  A neighbour that map_find finds and that is a node is united with the
// cell: both roots are found, and the root with the larger slot is hooked under the smaller by
// atomicCAS(&parent[hi], hi, lo); when the CAS fails the find goes on from the value it returned.  The walks start from
// ancestors already in hand -- the cell's side from where the last neighbour's unite ended, the neighbour's from the parent
// that the node test loaded -- and a neighbour whose parent IS that ancestor costs no further load: inside a large
// component most do, and every walk saved is a load of the one line that holds the root.
// parent[i] <= i holds under every interleaving (a root is hooked under a smaller slot, a halving store writes an
// ancestor, and ancestors are smaller), so no cycle can form and every walk ends; every failed CAS is another thread's
// successful one, and there are fewer of those than nodes.
// A STALE read of parent is harmless, which is why there is no fence, no flag and no waiting here (a CU's L1 is not
// refreshed by other CUs' stores and the XCDs' L2s are not coherent; the loads are relaxed agent-scope atomics only so
// that retries stay few): only roots are ever hooked, and halving only replaces a parent by an ancestor, so "a is an
// ancestor of b" never stops being true -- whatever value of parent[x] a thread sees, old or new, is an ancestor of x.
// Two finds that meet at one slot therefore prove one component, and nothing is decided on a value that may be stale:
// a new edge enters only through the CAS, which executes at the coherence point, succeeds only on a slot that is a
// root at that moment and reports the current parent when it fails.
__global__ void __launch_bounds__(kPcBlock) k_map_comp_union(MapTable t, int connectivity, uint32_t* parent)
{
    const int reach = connectivity == 124 ? 2 : 1;
    const int most = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 6;  // the largest |o|_1
    const uint32_t mask = (1u << t.cap_log2) - 1u;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const uint32_t i = (uint32_t)(base + threadIdx.x);
        if (comp_load(&parent[i]) == kMapCompNone) continue;  // (nodes keep a slot, the others kMapCompNone, for good)
        const unsigned long long k = t.keys[i];
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = pc_cell_of(k, a);
        uint32_t up = i;  // the nearest ancestor of i this thread knows: the next neighbour's walk starts there
        for (int oz = 0; oz <= reach; ++oz) {
            const int vz = c[2] + oz;
            if (vz > kPcCellMax) continue;
            for (int oy = -reach; oy <= reach; ++oy) {
                const int vy = c[1] + oy;
                if (abs(vy) > kPcCellMax) continue;
                for (int ox = -reach; ox <= reach; ++ox) {
                    const int vx = c[0] + ox;
                    if (!(oz > 0 || oy > 0 || (oy == 0 && ox > 0)) || abs(ox) + abs(oy) + oz > most || abs(vx) > kPcCellMax) continue;
                    const uint32_t j = map_find(t.keys, mask, pc_key(vx, vy, vz));
                    if (j == ~0u) continue;
                    uint32_t a = up, b = comp_load(&parent[j]);  // ancestors of i and of j
                    if (b == kMapCompNone) continue;
                    while (a != b) {
                        a = comp_find(parent, a);
                        b = comp_find(parent, b);
                        if (a == b) break;
                        const uint32_t hi = max(a, b), lo = min(a, b);
                        const uint32_t seen = atomicCAS(&parent[hi], hi, lo);
                        a = lo;
                        if (seen == hi) break;
                        b = seen;  // (hi was hooked by another thread meanwhile: on from its current parent)
                    }
                    up = a;  // (a == b, or lo with hi hooked under it: an ancestor of i either way)
                }
            }
        }
    }
}

// every node's parent becomes its root.  Reads what k_map_comp_union left; a slot another thread of this launch has
// flattened already holds its root instead of a nearer ancestor, and either leads to the same root (a root is never written).
__global__ void __launch_bounds__(kPcBlock) k_map_comp_flatten(uint32_t cap_log2, uint32_t* parent)
{
    const size_t cap = (size_t)1 << cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = parent[i];
        if (r == kMapCompNone || r == (uint32_t)i) continue;
        for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;
        parent[i] = r;
    }
}

__device__ inline unsigned long long comp_wave_min(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline unsigned long long comp_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// per node, at its root's slot: label = min(label, key), cells += 1, points += n -- integer atomics on words that
// k_map_comp_init wrote, so the order of the threads does not matter.  The nodes among a wave's 64 slots are taken root by
// root (a uniform loop: the first node left names the root, every lane with that root joins): a root that one lane holds
// gets that lane's three atomics; a root that several hold -- the rule inside a large component, whose cells the hash
// scatters over the table -- is reduced in registers and gets the three atomics once.  Per-lane atomics alone were bound by
// the largest component: each of its cells an atomic on the same three words, at the 83 per microsecond one line takes.
__global__ void __launch_bounds__(kPcBlock) k_map_comp_reduce(MapTable t, MapComponents c)
{
    const int lane = threadIdx.x & 63;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const uint32_t r = c.parent[i];
        const bool node = r != kMapCompNone;
        const unsigned long long key = node ? t.keys[i] : ~0ull, n = node ? (unsigned long long)t.n[i] : 0ull;
        unsigned long long left = __ballot(node);  // (the same in every lane of the wave, as is the loop below)
        while (left != 0ull) {
            const int lead = __ffsll((long long)left) - 1;
            const uint32_t r0 = __shfl(r, lead, 64);
            const bool mine = node && r == r0;
            const unsigned long long same = __ballot(mine);  // (lanes taken earlier hold other roots)
            if (__popcll(same) == 1) {
                if (mine) {
                    atomicMin(&c.label[r0], key);
                    atomicAdd(&c.cells[r0], 1u);
                    atomicAdd(&c.points[r0], n);
                }
            } else {
                const unsigned long long k_min = comp_wave_min(mine ? key : ~0ull), n_sum = comp_wave_sum(mine ? n : 0ull);
                if (lane == lead) {
                    atomicMin(&c.label[r0], k_min);
                    atomicAdd(&c.cells[r0], (uint32_t)__popcll(same));
                    atomicAdd(&c.points[r0], n_sum);
                }
            }
            left &= ~same;
        }
    }
}

// whether the root at slot i passes the selection's criteria 2 and 3
__device__ inline bool comp_eligible(const MapComponents& c, size_t i, const MapCompSelect& o)
{
    return c.parent[i] == (uint32_t)i && (unsigned long long)c.cells[i] >= o.min_cells && c.points[i] >= o.min_points;
}

// whether (cells, label) comes strictly after rank k - 1 of `top` in the order cells descending, label ascending
__device__ inline bool comp_after(const unsigned long long* __restrict__ top, int k, unsigned long long cells, unsigned long long label)
{
    if (k == 0) return true;
    const unsigned long long tc = top[2 * (k - 1)], tl = top[2 * (k - 1) + 1];
    return cells < tc || (cells == tc && label > tl);
}

// Rank k of the selection's order, in two launches: top[2 k] = the most cells among the eligible roots after rank k - 1
// (0 when none is left: top was cleared), then top[2 k + 1] = the smallest label among those with that many cells (all
// ones when none is left).  Ranks 0 .. k - 1 are read as earlier launches left them.
__global__ void __launch_bounds__(kPcBlock) k_map_comp_rank_cells(uint32_t cap_log2, MapComponents c, MapCompSelect o, int k,
                                                                  unsigned long long* __restrict__ top)
{
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) top[2 * k + 1] = ~0ull;  // (k_map_comp_rank_label's start)
    __syncthreads();
    uint32_t best = 0;
    const size_t cap = (size_t)1 << cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        if (comp_eligible(c, i, o) && comp_after(top, k, c.cells[i], c.label[i])) best = max(best, c.cells[i]);
    }
    if (best) atomicMax(&s_max, best);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(&top[2 * k], (unsigned long long)s_max);
}

__global__ void __launch_bounds__(kPcBlock) k_map_comp_rank_label(uint32_t cap_log2, MapComponents c, MapCompSelect o, int k,
                                                                  unsigned long long* __restrict__ top)
{
    const unsigned long long want = top[2 * k];
    if (want == 0ull) return;  // (no component is left for this rank)
    const size_t cap = (size_t)1 << cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        if (comp_eligible(c, i, o) && (unsigned long long)c.cells[i] == want && comp_after(top, k, want, c.label[i]))
            atomicMin(&top[2 * k + 1], c.label[i]);  // (a handful of roots at most share the largest count)
    }
}

// ctr[2] += roots, ctr[3] += roots of one cell; ctr[4] = the points of the root that top[0], top[1] name (one writer)
__global__ void __launch_bounds__(kPcBlock) k_map_comp_count(uint32_t cap_log2, MapComponents c, const unsigned long long* __restrict__ top,
                                                             unsigned long long* __restrict__ ctr)
{
    MapCounts<2> cnt;
    const size_t cap = (size_t)1 << cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool root = c.parent[i] == (uint32_t)i;
        const uint32_t cells = root ? c.cells[i] : 0u;
        if (root && (unsigned long long)cells == top[0] && c.label[i] == top[1]) ctr[4] = c.points[i];
        cnt.count<0>(root);
        cnt.count<1>(cells == 1u);
    }
    cnt.flush(ctr + 2);
}

// The selection's reason of every slot (kMapPruneEmpty without a cell), the first that holds: 1 no node; 2 its
// component's cells < min_cells; 3 its points < min_points; 4 keep > 0 and the component comes after rank keep - 1 of
// `top` (a rank that found no component -- cells 0 -- means that fewer than keep exist: all of them stay).
// ctr[0] += kept, ctr[r] += removed by reason r, ctr[5] += roots kept.
__global__ void __launch_bounds__(kPcBlock) k_map_comp_select(MapTable t, MapComponents c, MapCompSelect o,
                                                              const unsigned long long* __restrict__ top, uint8_t* __restrict__ reason,
                                                              unsigned long long* __restrict__ ctr)
{
    MapCounts<kMapCompSelectCounters> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = kMapPruneEmpty;
        bool root = false;
        if (map_passes(t, i, 0u, 0u)) {
            const uint32_t p = c.parent[i];
            if (p == kMapCompNone) {
                r = 1u;
            } else {
                const unsigned long long cells = c.cells[p], label = c.label[p];
                if (cells < o.min_cells)
                    r = 2u;
                else if (c.points[p] < o.min_points)
                    r = 3u;
                else if (o.keep > 0 && top[2 * (o.keep - 1)] != 0ull && comp_after(top, o.keep, cells, label))
                    r = 4u;
                else
                    r = 0u;
                root = r == 0u && p == (uint32_t)i;
            }
        }
        reason[i] = (uint8_t)r;
        cnt.count<0>(r == 0u);
        cnt.count<1>(r == 1u);
        cnt.count<2>(r == 2u);
        cnt.count<3>(r == 3u);
        cnt.count<4>(r == 4u);
        cnt.count<5>(root);
    }
    cnt.flush(ctr);
}

// the labelling compacted like k_map_extract's cells under the labelling's filter, with its blk_off (one offset per tile of
// kPcBlock slots): key, label and, when asked for, the selection's reason, in slot order; walked in strides
__global__ void __launch_bounds__(kPcBlock) k_map_comp_gather(MapTable t, uint32_t min_points, uint32_t min_windows, MapComponents c,
                                                              const uint8_t* __restrict__ reason, const uint32_t* __restrict__ blk_off,
                                                              unsigned long long* __restrict__ key_out,
                                                              unsigned long long* __restrict__ label_out, uint8_t* __restrict__ reason_out)
{
    map_compact(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, min_points, min_windows); },
        [&](size_t i, size_t o) {
            key_out[o] = t.keys[i];
            label_out[o] = c.label[c.parent[i]];
            if (reason) reason_out[o] = reason[i];
        });
}

// blk[b] = number of roots in [b * kPcBlock, (b + 1) * kPcBlock): k_map_flag_count for components
__global__ void __launch_bounds__(kPcBlock) k_map_comp_root_count(const uint32_t* __restrict__ parent, uint32_t* __restrict__ blk)
{
    const size_t i = (size_t)blockIdx.x * kPcBlock + threadIdx.x;  // (< cap: a multiple of the workgroup)
    uint32_t total;
    (void)pc_block_exclusive(parent[i] == (uint32_t)i ? 1u : 0u, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one row per root, in slot order, with k_map_comp_root_count's scanned blk_off
__global__ void __launch_bounds__(kPcBlock) k_map_comp_list(uint32_t cap_log2, MapComponents c, const uint32_t* __restrict__ blk_off,
                                                            unsigned long long* __restrict__ label_out,
                                                            unsigned long long* __restrict__ cells_out,
                                                            unsigned long long* __restrict__ points_out)
{
    map_compact(
        cap_log2, blk_off, [&](size_t i) { return c.parent[i] == (uint32_t)i; },  // (a slot of the table: i < cap)
        [&](size_t i, size_t o) {
            label_out[o] = c.label[i];
            cells_out[o] = (unsigned long long)c.cells[i];
            points_out[o] = c.points[i];
        });
}

// ---- the map's k nearest cells (include/dsi_map_knn.h dsx_map_knn*; DESIGN.md 7j "Neighbours and statistical outliers") ----
// One thread per query.  The running top-k is a list of K (d2, key) pairs sorted ascending, K in {1, 2, 4, 8, 16} a
// template parameter and every index into the list a compile-time constant, so that the list lives in registers (an array
// indexed at run time would go to scratch); the runtime k is served by the next K and a truncation -- the first k of the K
// smallest are the k smallest.  An empty place holds (+inf, all ones), which no candidate ties with: an admitted d2 is finite.
//
// (nd, nk) into its place: one unrolled compare-and-swap pass carries the larger of the pair and the list's entry onward,
// and what falls off the end is dropped.  The order (d2, key) is total, so the list does not depend on the order of the calls.
template <int K>
__device__ inline void knn_insert(double (&d2)[K], unsigned long long (&key)[K], double nd, unsigned long long nk)
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool before = nd < d2[j] || (nd == d2[j] && nk < key[j]);
        const double td = d2[j];
        const unsigned long long tk = key[j];
        d2[j] = before ? nd : td;
        key[j] = before ? nk : tk;
        nd = before ? td : nd;
        nk = before ? tk : nk;
    }
}

// the query p against the table: map_near_cells' candidates, the cell with key `self` (0: none) left out; admitted iff
// sqrt(d2) <= radius.  Returns the number admitted; the list holds the first K of them by (d2, key).
template <int K>
__device__ inline uint32_t knn_scan(const MapTable& t, uint32_t mask, const MapKnn& o, const double (&p)[3], unsigned long long self,
                                    double (&d2)[K], unsigned long long (&key)[K])
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
        d2[j] = INFINITY;
        key[j] = ~0ull;
    }
    uint32_t admitted = 0;
    map_near_cells(t, mask, o.min_points, o.min_windows, o.leaf, o.reach, p, self, [&](uint32_t, unsigned long long kb, double dd) {
        if (!(sqrt(dd) <= o.radius)) return;
        ++admitted;
        knn_insert<K>(d2, key, dd, kb);
    });
    return admitted;
}

// the neighbours of n points, walked in strides: keys / dist [n][k] in rank order, padded with 0 / +inf; found [n]
template <int K>
__global__ void __launch_bounds__(kPcBlock) k_map_knn_points(MapTable t, MapKnn o, const float* __restrict__ pts, uint32_t stride, uint32_t n,
                                                             unsigned long long* __restrict__ keys, float* __restrict__ dist,
                                                             uint8_t* __restrict__ found)
{
    const uint32_t mask = (1u << t.cap_log2) - 1u;
    const size_t step = (size_t)gridDim.x * kPcBlock;
    for (size_t i = (size_t)blockIdx.x * kPcBlock + threadIdx.x; i < (size_t)n; i += step) {
        double p[3], d2[K];
        unsigned long long key[K];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) p[ax] = (double)pts[i * stride + ax];
        const uint32_t admitted = knn_scan<K>(t, mask, o, p, 0ull, d2, key);
        const int f = (int)min(admitted, (uint32_t)o.k);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < o.k) {
                const size_t at = i * (size_t)o.k + j;
                if (keys) keys[at] = j < f ? key[j] : 0ull;
                if (dist) dist[at] = j < f ? (float)sqrt(d2[j]) : INFINITY;
            }
        }
        if (found) found[i] = (uint8_t)f;
    }
}

// The self query: every cell that passes the filter against the others (itself left out by key), a counted slot walk
// (MapCounts).  Per query found = min(k, admitted), m = (((d_1 + d_2) + ...) + d_found) / found in rank
// order and q = (u64) floor((m / radius) * 2^30) (found == 0: m = +inf, q = 0), written per slot; scored iff
// found >= min_found.  ctr: [0] queries, [1] occupied slots the filter leaves out, [2] scored, [3] isolated, and over the
// scored [4] sum q, [5] sum of q^2's low 32 bits, [6] sum of q^2 >> 32 (q^2 <= 2^60 and at most 2^27 cells: neither word
// overflows; the host puts the 128-bit sum together).  The three sums are kept per thread and added in LDS beside the
// counts: one global atomic per workgroup for each of them too.
template <int K>
__global__ void __launch_bounds__(kPcBlock) k_map_knn_self(MapTable t, MapKnn o, MapKnnCells c, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0ull;
    MapCounts<4> cnt;
    unsigned long long sum_q = 0ull, sq_lo = 0ull, sq_hi = 0ull;
    const uint32_t mask = (1u << t.cap_log2) - 1u;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool occupied = map_passes(t, i, 0u, 0u), f = occupied && map_passes(t, i, o.min_points, o.min_windows);
        bool scored = false;
        if (f) {
            const unsigned long long k = t.keys[i];
            const uint32_t n = t.n[i];
            double p[3], d2[K];
            unsigned long long key[K];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) p[ax] = (double)map_centroid(t, i, k, n, ax, o.leaf);
            const uint32_t admitted = knn_scan<K>(t, mask, o, p, k, d2, key);
            const int fnd = (int)min(admitted, (uint32_t)o.k);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < fnd) s = s + sqrt(d2[j]);
            const double m = s / (double)fnd;
            const unsigned long long q = fnd ? (unsigned long long)floor((m / o.radius) * 1073741824.0) : 0ull;
            c.found[i] = (uint8_t)fnd;
            c.q[i] = (uint32_t)q;
            c.mean[i] = fnd ? (float)m : INFINITY;
            scored = fnd >= o.min_found;
            if (scored) {
                const unsigned long long q2 = q * q;
                sum_q += q;
                sq_lo += q2 & 0xffffffffull;
                sq_hi += q2 >> 32;
            }
        }
        cnt.count<0>(f);
        cnt.count<1>(occupied && !f);
        cnt.count<2>(scored);
        cnt.count<3>(f && !scored);
    }
    if (sum_q) atomicAdd(&s_sum[0], sum_q);
    if (sq_lo) atomicAdd(&s_sum[1], sq_lo);
    if (sq_hi) atomicAdd(&s_sum[2], sq_hi);
    cnt.flush(ctr);
    if (threadIdx.x >= 4 && threadIdx.x < 7 && s_sum[threadIdx.x - 4]) atomicAdd(&ctr[threadIdx.x], s_sum[threadIdx.x - 4]);
}

// The selection's reason of every slot (kMapPruneEmpty without a cell), the first that holds: 1 the cell fails the
// query's filter; 2 found < min_found; 3 use_threshold and q > T_q.  ctr[0] += kept, ctr[r] += removed by reason r.
__global__ void __launch_bounds__(kPcBlock) k_map_knn_select(MapTable t, MapKnn o, MapKnnCells c, int use_threshold, uint32_t T_q,
                                                             uint8_t* __restrict__ reason, unsigned long long* __restrict__ ctr)
{
    MapCounts<kMapKnnSelectCounters> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = kMapPruneEmpty;
        if (map_passes(t, i, 0u, 0u)) {
            if (!map_passes(t, i, o.min_points, o.min_windows))
                r = 1u;
            else if ((int)c.found[i] < o.min_found)
                r = 2u;
            else if (use_threshold && c.q[i] > T_q)
                r = 3u;
            else
                r = 0u;
        }
        reason[i] = (uint8_t)r;
        cnt.count<0>(r == 0u);
        cnt.count<1>(r == 1u);
        cnt.count<2>(r == 2u);
        cnt.count<3>(r == 3u);
    }
    cnt.flush(ctr);
}

// the self query compacted like k_map_extract's cells under the query's filter, with its blk_off (one offset per tile of
// kPcBlock slots): key, found, mean, q and, when asked for, the selection's reason, in slot order; walked in strides
__global__ void __launch_bounds__(kPcBlock) k_map_knn_gather(MapTable t, uint32_t min_points, uint32_t min_windows, MapKnnCells c,
                                                             const uint8_t* __restrict__ reason, const uint32_t* __restrict__ blk_off,
                                                             unsigned long long* __restrict__ key_out, uint8_t* __restrict__ found_out,
                                                             float* __restrict__ mean_out, uint32_t* __restrict__ q_out,
                                                             uint8_t* __restrict__ reason_out)
{
    map_compact(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, min_points, min_windows); },
        [&](size_t i, size_t at) {
            key_out[at] = t.keys[i];
            found_out[at] = c.found[i];
            mean_out[at] = c.mean[i];
            q_out[at] = c.q[i];
            if (reason) reason_out[at] = reason[i];
        });
}

// ---- the map's local shape (include/dsi_map_pca.h dsx_map_pca*; DESIGN.md 7j "Local shape") ----
// One thread per query cell.  The neighbourhood's nine integer moments are summed in registers -- straight in the scan for
// K == 0 (every admitted cell is a member), after knn_scan<K> for K > 0, whose found keys are looked up again for their
// offsets --, and the solve is dsi_pca_host.hpp's, the statements the host runs: its eighteen doubles sit behind
// compile-time indices.

// D = llrint((q - p) / quantum) per axis of the cell in slot j (key kb) against the query p, added to s and ss
__device__ inline void pca_accumulate(const MapTable& t, uint32_t j, unsigned long long kb, const MapPca& o, const double (&p)[3],
                                      long long (&s)[3], long long (&ss)[6])
{
    const uint32_t nb = t.n[j];
    const long long dx = llrint(((double)map_centroid(t, j, kb, nb, 0, o.q.leaf) - p[0]) / o.quantum);
    const long long dy = llrint(((double)map_centroid(t, j, kb, nb, 1, o.q.leaf) - p[1]) / o.quantum);
    const long long dz = llrint(((double)map_centroid(t, j, kb, nb, 2, o.q.leaf) - p[2]) / o.quantum);
    s[0] += dx, s[1] += dy, s[2] += dz;
    ss[0] += dx * dx, ss[1] += dx * dy, ss[2] += dx * dz;
    ss[3] += dy * dy, ss[4] += dy * dz, ss[5] += dz * dz;
}

// knn_scan's walk with every admitted candidate a member: returns their number, the moments in s and ss
__device__ inline uint32_t pca_scan_all(const MapTable& t, uint32_t mask, const MapPca& o, const double (&p)[3], unsigned long long self,
                                        long long (&s)[3], long long (&ss)[6])
{
    uint32_t admitted = 0;
    map_near_cells(t, mask, o.q.min_points, o.q.min_windows, o.q.leaf, o.q.reach, p, self,
                   [&](uint32_t j, unsigned long long kb, double dd) {
                       if (!(sqrt(dd) <= o.q.radius)) return;
                       ++admitted;
                       pca_accumulate(t, j, kb, o, p, s, ss);
                   });
    return admitted;
}

// The pass: every cell that passes the filter, a counted slot walk (MapCounts).  Per query the row of
// dsi_map_pca.h step 8 into c (a sparse query: label 0, flags 0, vectors 0, eigenvalues +inf).  ctr: [0] queries, [1] occupied
// slots the filter leaves out, [2] sparse, [3..5] label 1..3, [6] normal determined, [7] tangent determined, [8] sum of m.
// The members are counter 8, a per-thread sum.
template <int K>
__global__ void __launch_bounds__(kPcBlock) k_map_pca(MapTable t, MapPca o, MapPcaCells c, unsigned long long* __restrict__ ctr)
{
    MapCounts<kMapPcaCounters> cnt;
    const uint32_t mask = (1u << t.cap_log2) - 1u;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool occupied = map_passes(t, i, 0u, 0u), f = occupied && map_passes(t, i, o.q.min_points, o.q.min_windows);
        uint32_t label = 0u, flags = 0u;
        if (f) {
            const unsigned long long k = t.keys[i];
            const uint32_t n = t.n[i];
            double p[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) p[ax] = (double)map_centroid(t, i, k, n, ax, o.q.leaf);
            long long s[3] = {0, 0, 0}, ss[6] = {0, 0, 0, 0, 0, 0};
            uint32_t found;
            if constexpr (K == 0) {
                found = pca_scan_all(t, mask, o, p, k, s, ss);
            } else {
                double d2[K];
                unsigned long long key[K];
                const uint32_t admitted = knn_scan<K>(t, mask, o.q, p, k, d2, key);
                found = min(admitted, (uint32_t)o.q.k);
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (j < (int)found) {
                        const uint32_t slot = map_find(t.keys, mask, key[j]);
                        if (slot != ~0u) pca_accumulate(t, slot, key[j], o, p, s, ss);  // (always found: the scan saw it)
                    }
            }
            const uint32_t m = found + 1u;
            cnt.sum<8>(m);  // (at most 343 per round: a workgroup's sum stays far below 2^32)
            PcaSolved r;
            if ((int)found >= o.q.min_found) {
                const int64_t s3[3] = {s[0], s[1], s[2]}, ss6[6] = {ss[0], ss[1], ss[2], ss[3], ss[4], ss[5]};
                pca_solve_core(m, s3, ss6, o.quantum, o.orient, o.viewpoint, p, r);
                label = r.label, flags = r.flags;
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) r.normal_f[a] = r.tangent_f[a] = 0.0f, r.eval[a] = INFINITY;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                c.normal[3 * i + a] = r.normal_f[a];
                c.tangent[3 * i + a] = r.tangent_f[a];
                c.eval[3 * i + a] = r.eval[a];
            }
            c.members[i] = (uint16_t)m;
            c.label[i] = (uint8_t)label;
            c.flags[i] = (uint8_t)flags;
            if (c.moments) {
#pragma unroll
                for (int a = 0; a < 3; ++a) c.moments[9 * i + a] = s[a];
#pragma unroll
                for (int a = 0; a < 6; ++a) c.moments[9 * i + 3 + a] = ss[a];
            }
        }
        cnt.count<0>(f);
        cnt.count<1>(occupied && !f);
        cnt.count<2>(f && label == 0u);
        cnt.count<3>(label == 1u);
        cnt.count<4>(label == 2u);
        cnt.count<5>(label == 3u);
        cnt.count<6>((flags & 1u) != 0u);
        cnt.count<7>((flags & 2u) != 0u);
    }
    cnt.flush(ctr);
}

// The selection's reason of every slot (kMapPruneEmpty without a cell), the first that holds: 1 the cell fails the pass's
// filter; 2 it is sparse (label 0) and remove_sparse; 3 its label's bit 1 << (label - 1) is not in keep_labels (a sparse cell
// that stays is kept).  ctr[0] += kept, ctr[r] += removed by reason r.
__global__ void __launch_bounds__(kPcBlock) k_map_pca_select(MapTable t, uint32_t min_points, uint32_t min_windows, const uint8_t* __restrict__ label,
                                                             uint32_t keep_labels, int remove_sparse, uint8_t* __restrict__ reason,
                                                             unsigned long long* __restrict__ ctr)
{
    MapCounts<kMapPcaSelectCounters> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = kMapPruneEmpty;
        if (map_passes(t, i, 0u, 0u)) {
            if (!map_passes(t, i, min_points, min_windows)) {
                r = 1u;
            } else {
                const uint32_t l = label[i];
                if (l == 0u)
                    r = remove_sparse ? 2u : 0u;
                else
                    r = (keep_labels >> (l - 1u)) & 1u ? 0u : 3u;
            }
        }
        reason[i] = (uint8_t)r;
        cnt.count<0>(r == 0u);
        cnt.count<1>(r == 1u);
        cnt.count<2>(r == 2u);
        cnt.count<3>(r == 3u);
    }
    cnt.flush(ctr);
}

// the pass compacted like k_map_extract's cells under the pass's filter, with its blk_off (one offset per tile of kPcBlock
// slots), in slot order and walked in strides; out.moments and reason_out are written when asked for (not NULL)
__global__ void __launch_bounds__(kPcBlock) k_map_pca_gather(MapTable t, uint32_t min_points, uint32_t min_windows, MapPcaCells c,
                                                             const uint8_t* __restrict__ reason, const uint32_t* __restrict__ blk_off,
                                                             unsigned long long* __restrict__ key_out, MapPcaCells out,
                                                             uint8_t* __restrict__ reason_out)
{
    map_compact(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, min_points, min_windows); },
        [&](size_t i, size_t at) {
            key_out[at] = t.keys[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                out.normal[3 * at + a] = c.normal[3 * i + a];
                out.tangent[3 * at + a] = c.tangent[3 * i + a];
                out.eval[3 * at + a] = c.eval[3 * i + a];
            }
            out.members[at] = c.members[i];
            out.label[at] = c.label[i];
            out.flags[at] = c.flags[i];
            if (out.moments) {
#pragma unroll
                for (int a = 0; a < 9; ++a) out.moments[9 * at + a] = c.moments[9 * i + a];
            }
            if (reason_out) reason_out[at] = reason[i];
        });
}

// ---- the map carved by free space (include/dsi_map_visibility.h dsx_map_observe / visibility_*; DESIGN.md 7j "Visibility") ----
// k_map_integrate_depth's test of a pixel: unmasked (m > 0; the caller passes 1 without a mask), d finite and in the range
__device__ __forceinline__ bool map_depth_valid(double d, uint32_t m, double min_depth, double max_depth)
{
    return m > 0u && isfinite(d) && d >= min_depth && d <= max_depth;
}

// One observation: every occupied cell against the depth image, by the rule of dsi_map_visibility.h.  The cell is
// k_map_render's point -- its extracted centroid through o.T, CLIPPED as there --; OUTSIDE unless its centre pixel is in
// the image (in double, before anything becomes an integer); its (2 W + 1)^2 pixels are loaded with their coordinates
// clamped into the image and counted only where the unclamped ones are inside: W is a template parameter, the loads are
// unrolled, none depends on another and none is out of bounds.  The verdict goes into the slot's own tally words, plain
// read-modify-writes by the slot's one thread (the host zeroed them before the tally's first view).
// ctr: [0] clipped, [1] outside, [2] unseen, [3] agree, [4] through, [5] behind, [6] the image's valid pixels -- counted
// by a second walk, over the pixels, whose rounds every lane of a workgroup enters together.  A counted slot walk (MapCounts).
template <int W>
__global__ void __launch_bounds__(kPcBlock) k_map_observe(MapTable t, MapObserve o, double leaf, const float* __restrict__ depth,
                                                          const uint8_t* __restrict__ mask, MapTally c, unsigned long long* __restrict__ ctr)
{
    enum : uint32_t { kNone, kClipped, kOutside, kUnseen, kAgree, kThrough, kBehind };
    MapCounts<kMapObserveCounters> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t verdict = kNone;
        if (map_passes(t, i, 0u, 0u)) {
            const unsigned long long k = t.keys[i];
            const uint32_t n = t.n[i];
            const double x = (double)map_centroid(t, i, k, n, 0, leaf), y = (double)map_centroid(t, i, k, n, 1, leaf),
                         z = (double)map_centroid(t, i, k, n, 2, leaf);
            const double X = ((o.T[0] * x + o.T[1] * y) + o.T[2] * z) + o.T[3];
            const double Y = ((o.T[4] * x + o.T[5] * y) + o.T[6] * z) + o.T[7];
            const double Z = ((o.T[8] * x + o.T[9] * y) + o.T[10] * z) + o.T[11];
            if (!(isfinite(X) && isfinite(Y) && Z >= o.min_depth && Z <= o.max_depth)) {  // (min/max_depth are finite)
                verdict = kClipped;
            } else {
                const double du = floor(((o.fx * (X / Z)) + o.cx) + 0.5), dv = floor(((o.fy * (Y / Z)) + o.cy) + 0.5);
                if (!(du >= 0.0 && du <= (double)(o.width - 1) && dv >= 0.0 && dv <= (double)(o.height - 1))) {
                    verdict = kOutside;
                } else {
                    const int iu = (int)du, iv = (int)dv;  // (in [0, 2^26): exact)
                    const double tol = (o.rel_tol * Z) + o.abs_tol, lo = Z - tol, hi = Z + tol;
                    uint32_t n_valid = 0u, n_agree = 0u, n_through = 0u;
#pragma unroll
                    for (int dy = -W; dy <= W; ++dy) {
#pragma unroll
                        for (int dx = -W; dx <= W; ++dx) {
                            const int px = iu + dx, py = iv + dy;
                            const bool in = px >= 0 && px < o.width && py >= 0 && py < o.height;
                            const size_t p = (size_t)min(max(py, 0), o.height - 1) * (size_t)o.width + (size_t)min(max(px, 0), o.width - 1);
                            const double d = (double)depth[p];
                            const uint32_t m = mask ? (uint32_t)mask[p] : 1u;
                            const bool valid = in && map_depth_valid(d, m, o.min_depth, o.max_depth);
                            n_valid += valid ? 1u : 0u;
                            n_agree += valid && d >= lo && d <= hi ? 1u : 0u;
                            n_through += valid && d > hi ? 1u : 0u;
                        }
                    }
                    verdict = n_valid == 0u ? kUnseen : n_agree > 0u ? kAgree : n_through == n_valid ? kThrough : kBehind;
                    if (verdict != kUnseen) {
                        c.seen[i] += 1u;
                        if (verdict == kAgree) c.agree[i] += 1u;
                        if (verdict == kThrough) c.through[i] += 1u;
                    }
                }
            }
        }
        cnt.count<0>(verdict == kClipped);
        cnt.count<1>(verdict == kOutside);
        cnt.count<2>(verdict == kUnseen);
        cnt.count<3>(verdict == kAgree);
        cnt.count<4>(verdict == kThrough);
        cnt.count<5>(verdict == kBehind);
    }
    const uint32_t npix = (uint32_t)o.width * (uint32_t)o.height, pstride = gridDim.x * kPcBlock;  // (<= 2^26, <= 2^18: base cannot wrap)
    for (uint32_t base = blockIdx.x * kPcBlock; base < npix; base += pstride) {
        const uint32_t p = base + threadIdx.x;
        bool valid = false;
        if (p < npix) valid = map_depth_valid((double)depth[p], mask ? (uint32_t)mask[p] : 1u, o.min_depth, o.max_depth);
        cnt.count<6>(valid);
    }
    cnt.flush(ctr);
}

// The selection's reason of every slot (kMapPruneEmpty without a cell): 1 (carved) iff through >= min_through and
// through > agree_weight * agree in 64 bits, else 0.  ctr[0] += kept, ctr[1] += carved.  A counted slot walk (MapCounts).
__global__ void __launch_bounds__(kPcBlock) k_map_visibility_select(MapTable t, MapTally c, uint32_t min_through, uint32_t agree_weight,
                                                                    uint8_t* __restrict__ reason, unsigned long long* __restrict__ ctr)
{
    MapCounts<kMapVisibilitySelectCounters> cnt;
    const size_t cap = (size_t)1 << t.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        uint32_t r = kMapPruneEmpty;
        if (map_passes(t, i, 0u, 0u)) {
            const uint32_t through = c.through[i];
            r = through >= min_through && (unsigned long long)through > (unsigned long long)agree_weight * (unsigned long long)c.agree[i] ? 1u : 0u;
        }
        reason[i] = (uint8_t)r;
        cnt.count<0>(r == 0u);
        cnt.count<1>(r == 1u);
    }
    cnt.flush(ctr);
}

// the tally compacted like k_map_extract's cells under the filter (1, 1), with its blk_off (one offset per tile of kPcBlock
// slots), in slot order: one workgroup per tile; reason_out is written when asked for (not NULL)
__global__ void __launch_bounds__(kPcBlock) k_map_visibility_gather(MapTable t, MapTally c, const uint8_t* __restrict__ reason,
                                                                    const uint32_t* __restrict__ blk_off, unsigned long long* __restrict__ key_out,
                                                                    MapTally out, uint8_t* __restrict__ reason_out)
{
    map_compact<true>(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, 1u, 1u); },
        [&](size_t i, size_t at) {
            key_out[at] = t.keys[i];
            out.seen[at] = c.seen[i];
            out.agree[at] = c.agree[i];
            out.through[at] = c.through[i];
            if (reason_out) reason_out[at] = reason[i];
        });
}

// ---- merging maps and moving their state (include/dsi_map_merge.h dsx_map_export / import / merge; DESIGN.md 7j "Merging") ----
// Every occupied slot's raw state compacted like k_map_extract's cells under the filter (0, 0), with its blk_off (one
// offset per tile of kPcBlock slots): key, n, S[3], windows and stamp in slot order.  Walked in strides; reads the table only.
__global__ void __launch_bounds__(kPcBlock) k_map_export(MapTable t, const uint32_t* __restrict__ blk_off,
                                                         unsigned long long* __restrict__ key_out, uint32_t* __restrict__ n_out,
                                                         unsigned long long* __restrict__ sums_out, uint32_t* __restrict__ w_out,
                                                         uint32_t* __restrict__ stamp_out)
{
    map_compact(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, 0u, 0u); },
        [&](size_t i, size_t o) {
            key_out[o] = t.keys[i];
            n_out[o] = t.n[i];
            w_out[o] = t.windows[i];
            stamp_out[o] = t.stamp[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) sums_out[3 * o + a] = t.sums[3 * i + a];
        });
}

// m incoming cells (host arrays, nothing trusted) checked and built into the zeroed table `to`.  Per cell, each counted on
// its own: [0] key 0 or a packed coordinate outside [1, 2 kPcCellMax + 1]; [1] a duplicate -- map_slot does not report the
// key as fresh (a bad key is not inserted); [2] n == 0; [3] windows == 0, > n or > stamp; [4] stamp == 0 or > calls;
// [5] some S[a] > n * 2^32 (n < 2^32: the product is exact in 64 bits); [6] `to` found full; [7] the sum of n.  A fresh
// slot has one writer: plain stores.  ctr [kMapImportCounters]: one global atomic per workgroup and counter.  MapCounts'
// contract with a stage of its own: the sum of n shares it, so its LDS words are 64 bits wide.
__global__ void __launch_bounds__(kPcBlock) k_map_import_build(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ n,
                                                               const unsigned long long* __restrict__ sums,
                                                               const uint32_t* __restrict__ windows, const uint32_t* __restrict__ stamp,
                                                               uint32_t m, uint32_t calls, MapTable to, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long s_cnt[kMapImportCounters];
    if (threadIdx.x < kMapImportCounters) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    uint32_t c[kMapImportCounters - 1] = {0, 0, 0, 0, 0, 0, 0};  // (the same in every lane of a wave)
    unsigned long long sum_n = 0ull;                            // (per lane)
    const uint32_t mask = (1u << to.cap_log2) - 1u;
    const size_t stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < m; base += stride) {
        const size_t i = base + threadIdx.x;
        bool bad[kMapImportCounters - 1] = {false, false, false, false, false, false, false};
        if (i < m) {
            const unsigned long long k = keys[i];
            const uint32_t cn = n[i], cw = windows[i], cs = stamp[i];
            const unsigned long long S0 = sums[3 * i], S1 = sums[3 * i + 1], S2 = sums[3 * i + 2];
            bad[0] = k == 0ull || (k >> 63) != 0ull;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint32_t p = pc_packed_of(k, a);
                bad[0] = bad[0] || p < 1u || p > 2u * (uint32_t)kPcCellMax + 1u;
            }
            bad[2] = cn == 0u;
            bad[3] = cw == 0u || cw > cn || cw > cs;
            bad[4] = cs == 0u || cs > calls;
            const unsigned long long most = (unsigned long long)cn << 32;
            bad[5] = S0 > most || S1 > most || S2 > most;
            sum_n += cn;
            if (!bad[0]) {
                bool fresh = false;
                const uint32_t slot = map_slot(to.keys, mask, k, &fresh);
                if (slot == ~0u) {
                    bad[6] = true;
                } else if (!fresh) {
                    bad[1] = true;
                } else {
                    to.n[slot] = cn;
                    to.windows[slot] = cw;
                    to.stamp[slot] = cs;
                    to.sums[3 * (size_t)slot + 0] = S0;
                    to.sums[3 * (size_t)slot + 1] = S1;
                    to.sums[3 * (size_t)slot + 2] = S2;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kMapImportCounters - 1; ++q) c[q] += (uint32_t)__popcll(__ballot(bad[q]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum_n += __shfl_down(sum_n, off, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kMapImportCounters - 1; ++q)
            if (c[q]) atomicAdd(&s_cnt[q], (unsigned long long)c[q]);
        if (sum_n) atomicAdd(&s_cnt[kMapImportCounters - 1], sum_n);
    }
    __syncthreads();
    if (threadIdx.x < kMapImportCounters && s_cnt[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], s_cnt[threadIdx.x]);
}

// src appended to dst (dsi_map_merge.h "the rule"): one thread per slot of src, in strides.  src's keys are distinct, so
// exactly one thread finds or claims a given slot of dst and nothing else writes dst meanwhile: after map_slot's
// compare-and-swap the cell's words are read, combined and stored plainly -- n, S[3] and windows added, stamp =
// max(stamp, stamp_src + off); a claimed slot holds zeros.  Sums and maxima of integers: the result depends neither on the
// thread order nor on either table's size nor on the probing.  The host has checked that no sum wraps.  mctr: [0] += cells
// new to dst, [1] += cells both hold; ctr (dst's four counters): [0] += new, [3] += cells that found dst full (map_slot is
// bounded by the capacity: an error, not a hang), and one thread adds src's accepted and rejected points to [1] and [2].
__global__ void __launch_bounds__(kPcBlock) k_map_merge(MapTable src, MapTable dst, uint32_t off, unsigned long long add_accepted,
                                                        unsigned long long add_rejected, unsigned long long* __restrict__ ctr,
                                                        unsigned long long* __restrict__ mctr)
{
    MapCounts<3> cnt;
    const uint32_t mask = (1u << dst.cap_log2) - 1u;
    const size_t cap = (size_t)1 << src.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const unsigned long long k = src.keys[i];  // (cap is a multiple of the workgroup: i < cap)
        bool is_new = false, is_common = false, full = false;
        if (k != 0ull) {
            bool fresh = false;
            const uint32_t slot = map_slot(dst.keys, mask, k, &fresh);
            if (slot == ~0u) {
                full = true;
            } else {
                is_new = fresh;
                is_common = !fresh;
                dst.n[slot] += src.n[i];
                dst.windows[slot] += src.windows[i];
                const uint32_t moved = src.stamp[i] + off, had = dst.stamp[slot];
                dst.stamp[slot] = moved > had ? moved : had;
#pragma unroll
                for (int a = 0; a < 3; ++a) dst.sums[3 * (size_t)slot + a] += src.sums[3 * i + a];
            }
        }
        cnt.count<0>(is_new);
        cnt.count<1>(is_common);
        cnt.count<2>(full);
    }
    cnt.flush_to({&ctr[0], &mctr[1], &ctr[3]});
    const uint32_t n_new = cnt.total(0);  // (the new cells count in both arrays)
    if (threadIdx.x == 0 && n_new) atomicAdd(&mctr[0], (unsigned long long)n_new);
    if (blockIdx.x == 0 && threadIdx.x == 3) {
        if (add_accepted) atomicAdd(&ctr[1], add_accepted);
        if (add_rejected) atomicAdd(&ctr[2], add_rejected);
    }
}

// ---- aligning maps (include/dsi_map_align.h dsx_map_align*; DESIGN.md 7j "Aligning") ----
// One correspondence pass.  Every cell of `a` that passes a's filter: p = its extracted centroid (float, widened);
// p' = T p by rule 1; c = floor(p' / leaf_b) per axis; the candidates are b's filtered cells at c + o, |o| <= reach per
// axis, an index with |c + o| > kPcCellMax skipped (a non-finite p' has no candidates); q = the candidate's extracted
// centroid; d2 = ((dx dx) + dy dy) + dz dz; the least (d2, key) wins -- a total order, so neither the
// order of the offsets nor the probing matters; MATCHED iff sqrt(d2) <= radius.  key_b[slot] = the winner's key or 0,
// dist[slot] = (float) sqrt(d2) or +inf.  A matched pair is quantised, U = llrint(p' / quantum), V = llrint(q / quantum)
// (|U|, |V| < 2^31: dsi_map_align.h), and adds to 25 64-bit sums: su[3], sv[3], the high and low words of the nine
// products U[r] V[c], and e2.  A thread keeps the 25 sums in registers over its strides (two's-complement adds: the signed
// sums are kept as unsigned words); at the end a wave adds them across its lanes by shuffles, its first lane adds the
// wave's totals to LDS, and the workgroup issues one global atomic per non-zero sum.  ctr: [0] matched, [1] unmatched,
// [2 + k] sum k.  Reads the tables, writes key_b, dist and ctr: a == b is legal.
__global__ void __launch_bounds__(kPcBlock, 4) k_map_align_step(MapTable a, MapTable b, MapAlign o, unsigned long long* __restrict__ key_b,
                                                             float* __restrict__ dist, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long s_acc[kMapAlignSums];
    __shared__ double s_T[12];  // (the pose is read once per cell: in LDS it holds no scalar registers over the lookups)
    if (threadIdx.x < kMapAlignSums) s_acc[threadIdx.x] = 0ull;
    if (threadIdx.x >= 64 && threadIdx.x < 64 + 12) s_T[threadIdx.x - 64] = o.T[threadIdx.x - 64];
    MapCounts<2> cnt;
    unsigned long long acc[kMapAlignSums];
#pragma unroll
    for (int k = 0; k < kMapAlignSums; ++k) acc[k] = 0ull;
    const uint32_t bmask = (1u << b.cap_log2) - 1u;
    const uint32_t cap = 1u << a.cap_log2, stride = gridDim.x * kPcBlock;  // (at most 2^27 slots: 32 bits hold base + stride)
    for (uint32_t base = blockIdx.x * kPcBlock; base < cap; base += stride) {
        const uint32_t i = base + threadIdx.x;
        const bool f = map_passes(a, i, o.min_points_a, o.min_windows_a);
        bool matched = false;
        if (f) {
            const unsigned long long k = a.keys[i];
            const uint32_t n = a.n[i];
            const double x = (double)map_centroid(a, i, k, n, 0, o.leaf_a), y = (double)map_centroid(a, i, k, n, 1, o.leaf_a),
                         z = (double)map_centroid(a, i, k, n, 2, o.leaf_a);
            // c as integers: a cell index beyond kPcCellMax + reach (a non-finite one included) has no candidate on its
            // axis, and within that range c + o is the same number in int as in double
            double p[3];
            int c[3];
            bool any = true;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                p[ax] = ((s_T[4 * ax] * x + s_T[4 * ax + 1] * y) + s_T[4 * ax + 2] * z) + s_T[4 * ax + 3];
                const double cf = floor(p[ax] / o.leaf_b);
                any = any && fabs(cf) <= (double)(kPcCellMax + kMapCompareMaxReach);  // (NaN and the infinities fail)
                c[ax] = any ? (int)cf : 0;
            }
            double best = INFINITY;
            unsigned long long best_key = 0ull;
            uint32_t best_j = 0u;
            const int reach = any ? o.reach : -1;  // (-1: the sweep is empty)
            for (int oz = -reach; oz <= reach; ++oz) {
                const int vz = c[2] + oz;
                if (abs(vz) > kPcCellMax) continue;
                for (int oy = -reach; oy <= reach; ++oy) {
                    const int vy = c[1] + oy;
                    if (abs(vy) > kPcCellMax) continue;
                    for (int ox = -reach; ox <= reach; ++ox) {
                        const int vx = c[0] + ox;
                        if (abs(vx) > kPcCellMax) continue;
                        const unsigned long long kb = pc_key(vx, vy, vz);
                        const uint32_t j = map_find(b.keys, bmask, kb);
                        if (j == ~0u || !map_passes(b, j, o.min_points_b, o.min_windows_b)) continue;
                        const uint32_t nb = b.n[j];
                        const double dx = p[0] - (double)map_centroid(b, j, kb, nb, 0, o.leaf_b);
                        const double dy = p[1] - (double)map_centroid(b, j, kb, nb, 1, o.leaf_b);
                        const double dz = p[2] - (double)map_centroid(b, j, kb, nb, 2, o.leaf_b);
                        const double d2 = ((dx * dx) + dy * dy) + dz * dz;
                        if (d2 < best || (d2 == best && kb < best_key)) best = d2, best_key = kb, best_j = j;
                    }
                }
            }
            const double d = sqrt(best);
            matched = best_key != 0ull && d <= o.radius;
            dist[i] = matched ? (float)d : INFINITY;
            key_b[i] = matched ? best_key : 0ull;
            if (matched) {
                const uint32_t nb = b.n[best_j];  // (the winner's centroid again: three loads per matched cell, no registers held)
                long long U[3], V[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    U[ax] = llrint(p[ax] / o.quantum);
                    V[ax] = llrint((double)map_centroid(b, best_j, best_key, nb, ax, o.leaf_b) / o.quantum);
                    acc[ax] += (unsigned long long)U[ax];
                    acc[3 + ax] += (unsigned long long)V[ax];
                    const long long e = U[ax] - V[ax];
                    acc[24] += (unsigned long long)(e * e);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        const long long P = U[r] * V[cc];
                        acc[6 + 3 * r + cc] += (unsigned long long)(P >> 32);
                        acc[15 + 3 * r + cc] += (unsigned long long)P & 0xffffffffull;
                    }
            }
        }
        cnt.count<0>(matched);
        cnt.count<1>(f && !matched);
    }
#pragma unroll
    for (int k = 0; k < kMapAlignSums; ++k) {
        unsigned long long v = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_acc[k], v);
    }
    cnt.flush(ctr);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + kMapAlignSums && s_acc[threadIdx.x - 64])
        atomicAdd(&ctr[2 + threadIdx.x - 64], s_acc[threadIdx.x - 64]);
}

// the step's correspondences compacted like k_map_extract's cells (same filter, same blk_off): a's key, the winner's key
// and the distance in slot order
__global__ void __launch_bounds__(kPcBlock) k_map_align_gather(MapTable t, uint32_t min_points, uint32_t min_windows,
                                                               const unsigned long long* __restrict__ key_b, const float* __restrict__ dist,
                                                               const uint32_t* __restrict__ blk_off, unsigned long long* __restrict__ key_a_out,
                                                               unsigned long long* __restrict__ key_b_out, float* __restrict__ dist_out)
{
    map_compact<true>(
        t.cap_log2, blk_off, [&](size_t i) { return map_passes(t, i, min_points, min_windows); },
        [&](size_t i, size_t o) {
            key_a_out[o] = t.keys[i];
            key_b_out[o] = key_b[i];
            dist_out[o] = dist[i];
        });
}

// One map into another as one integrate call: every cell of src that passes the filter is its extracted centroid (float,
// widened), which goes through map_integrate_point under T into dst -- dsi_map_integrate of dsi_map_extract's list, bit for
// bit.  src is only read and dst != src.  A counted slot walk (MapCounts) over src; ctr as k_map_integrate_depth's.
__global__ void __launch_bounds__(kPcBlock) k_map_integrate_map(MapTable src, uint32_t min_points, uint32_t min_windows, double leaf_src,
                                                                MapPose T, double leaf, uint32_t serial, MapTable dst,
                                                                unsigned long long* __restrict__ ctr)
{
    MapCounts<4> cnt;
    const size_t cap = (size_t)1 << src.cap_log2, stride = (size_t)gridDim.x * kPcBlock;
    for (size_t base = (size_t)blockIdx.x * kPcBlock; base < cap; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool in = map_passes(src, i, min_points, min_windows);
        bool ok = false, fresh = false, full = false;
        if (in) {
            const unsigned long long k = src.keys[i];
            const uint32_t n = src.n[i];
            map_integrate_point((double)map_centroid(src, i, k, n, 0, leaf_src), (double)map_centroid(src, i, k, n, 1, leaf_src),
                                (double)map_centroid(src, i, k, n, 2, leaf_src), T, leaf, serial, dst, &ok, &fresh, &full);
        }
        cnt.count<0>(fresh);
        cnt.count<1>(ok);
        cnt.count<2>(in && !ok && !full);
        cnt.count<3>(full);
    }
    cnt.flush(ctr);
}

}  // namespace

size_t map_table_bytes(uint32_t cap_log2) { return ((size_t)1 << cap_log2) * (4 * sizeof(unsigned long long) + 3 * sizeof(uint32_t)); }

MapTable map_table_at(void* block, uint32_t cap_log2)
{
    const size_t cap = (size_t)1 << cap_log2;
    MapTable t;
    t.keys = static_cast<unsigned long long*>(block);
    t.sums = t.keys + cap;
    t.n = reinterpret_cast<uint32_t*>(t.sums + 3 * cap);
    t.windows = t.n + cap;
    t.stamp = t.windows + cap;
    t.cap_log2 = cap_log2;
    return t;
}

hipError_t launch_map_integrate(hipStream_t s, const float* pts, uint32_t stride, uint32_t n, const double T_w_rv[12], double leaf,
                                uint32_t serial, const MapTable& t, unsigned long long* ctr)
{
    if (n == 0) return hipSuccess;
    MapPose T;
    for (int k = 0; k < 12; ++k) T.m[k] = T_w_rv[k];
    hipLaunchKernelGGL(k_map_integrate, dim3(pc_blocks(n)), dim3(kPcBlock), 0, s, pts, stride, n, T, leaf, serial, t, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_rehash(hipStream_t s, const MapTable& from, const MapTable& to, unsigned long long* ctr)
{
    hipLaunchKernelGGL(k_map_rehash, dim3(pc_blocks((size_t)1 << from.cap_log2)), dim3(kPcBlock), 0, s, from, to, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_count(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, uint32_t* blk, uint32_t* tiles)
{
    const uint32_t nb = pc_blocks((size_t)1 << t.cap_log2);
    hipLaunchKernelGGL(k_map_flag_count, dim3(nb), dim3(kPcBlock), 0, s, t, min_points, min_windows, blk);
    return pc_scan(s, blk, nb, tiles);
}

hipError_t launch_map_extract(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, double leaf,
                              const uint32_t* blk, float* xyz, uint32_t* n_out, uint32_t* w_out, unsigned long long* key_out)
{
    const uint32_t nb = pc_blocks((size_t)1 << t.cap_log2);
    hipLaunchKernelGGL(k_map_extract, dim3(nb), dim3(kPcBlock), 0, s, t, min_points, min_windows, leaf, blk, xyz, n_out, w_out, key_out);
    return hipExtGetLastError();
}

hipError_t launch_map_render(hipStream_t s, const MapTable& t, const MapView& v, double leaf, const MapImage& img, unsigned long long* ctr)
{
    const size_t npix = (size_t)v.width * (size_t)v.height;
    hipError_t e = hipMemsetAsync(img.zkey, 0xff, npix * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(img.hits, 0, npix * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(ctr, 0, kMapRenderCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_render, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t, v,
                       leaf, img.zkey, img.hits, ctr);
    hipLaunchKernelGGL(k_map_render_finish, dim3(std::min(pc_blocks(npix), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, img.zkey,
                       img.hits, (uint32_t)npix, img.depth, img.windows, img.mask, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_integrate_depth(hipStream_t s, const float* depth, const uint8_t* mask, const MapDepthImage& g,
                                      const double T_w_c[12], double leaf, uint32_t serial, const MapTable& t, unsigned long long* ctr)
{
    MapPose T;
    for (int k = 0; k < 12; ++k) T.m[k] = T_w_c[k];
    hipLaunchKernelGGL(k_map_integrate_depth, dim3(pc_blocks(g.npix)), dim3(kPcBlock), 0, s, depth, mask, g, T, leaf, serial, t, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_compare(hipStream_t s, const MapTable& a, const MapTable& b, const MapCompare& o, float* dist,
                              unsigned long long* hist, unsigned long long* ctr)
{
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)o.n_bins * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(ctr, 0, kMapCompareCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_compare, dim3(std::min(pc_blocks((size_t)1 << a.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, a, b,
                       o, dist, hist, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_compare_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const float* dist,
                                     const uint32_t* blk, float* dist_out, unsigned long long* key_out)
{
    const uint32_t nb = pc_blocks((size_t)1 << t.cap_log2);
    hipLaunchKernelGGL(k_map_compare_gather, dim3(nb), dim3(kPcBlock), 0, s, t, min_points, min_windows, dist, blk, dist_out, key_out);
    return hipExtGetLastError();
}

hipError_t launch_map_prune_classify(hipStream_t s, const MapTable& t, const MapPrune& o, uint8_t* first, uint8_t* reason,
                                     unsigned long long* ctr)
{
    hipError_t e = hipMemsetAsync(ctr, 0, kMapPruneCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 grid(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks));
    hipLaunchKernelGGL(k_map_prune_reason, grid, dim3(kPcBlock), 0, s, t, o, first, ctr);
    hipLaunchKernelGGL(k_map_prune_support, grid, dim3(kPcBlock), 0, s, t, o, first, reason, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_prune_rehash(hipStream_t s, const MapTable& from, const MapTable& to, const uint8_t* reason,
                                   unsigned long long* ctr)
{
    hipLaunchKernelGGL(k_map_prune_rehash, dim3(std::min(pc_blocks((size_t)1 << from.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0,
                       s, from, to, reason, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_prune_gather(hipStream_t s, const MapTable& t, const uint8_t* reason, const uint32_t* blk, uint8_t* reason_out,
                                   unsigned long long* key_out)
{
    const uint32_t nb = pc_blocks((size_t)1 << t.cap_log2);
    hipLaunchKernelGGL(k_map_prune_gather, dim3(nb), dim3(kPcBlock), 0, s, t, reason, blk, reason_out, key_out);
    return hipExtGetLastError();
}

hipError_t launch_map_components(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, int connectivity,
                                 const MapComponents& c, unsigned long long* top, unsigned long long* ctr)
{
    hipError_t e = hipMemsetAsync(ctr, 0, kMapCompCounters * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(top, 0, kMapCompTopWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 grid(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), block(kPcBlock);
    const MapCompSelect all{0ull, 0ull, 1};
    hipLaunchKernelGGL(k_map_comp_init, grid, block, 0, s, t, min_points, min_windows, c, ctr);
    hipLaunchKernelGGL(k_map_comp_union, grid, block, 0, s, t, connectivity, c.parent);
    hipLaunchKernelGGL(k_map_comp_flatten, grid, block, 0, s, t.cap_log2, c.parent);
    hipLaunchKernelGGL(k_map_comp_reduce, grid, block, 0, s, t, c);
    hipLaunchKernelGGL(k_map_comp_rank_cells, grid, block, 0, s, t.cap_log2, c, all, 0, top);
    hipLaunchKernelGGL(k_map_comp_rank_label, grid, block, 0, s, t.cap_log2, c, all, 0, top);
    hipLaunchKernelGGL(k_map_comp_count, grid, block, 0, s, t.cap_log2, c, top, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_components_select(hipStream_t s, const MapTable& t, const MapComponents& c, const MapCompSelect& o, uint8_t* reason,
                                        unsigned long long* top, unsigned long long* ctr)
{
    hipError_t e = hipMemsetAsync(ctr, 0, kMapCompSelectCounters * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(top, 0, kMapCompTopWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 grid(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), block(kPcBlock);
    for (int k = 0; k < o.keep; ++k) {
        hipLaunchKernelGGL(k_map_comp_rank_cells, grid, block, 0, s, t.cap_log2, c, o, k, top);
        hipLaunchKernelGGL(k_map_comp_rank_label, grid, block, 0, s, t.cap_log2, c, o, k, top);
    }
    hipLaunchKernelGGL(k_map_comp_select, grid, block, 0, s, t, c, o, top, reason, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_components_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const MapComponents& c,
                                        const uint8_t* reason, const uint32_t* blk, unsigned long long* key_out,
                                        unsigned long long* label_out, uint8_t* reason_out)
{
    hipLaunchKernelGGL(k_map_comp_gather, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t,
                       min_points, min_windows, c, reason, blk, key_out, label_out, reason_out);
    return hipExtGetLastError();
}

hipError_t launch_map_components_count_roots(hipStream_t s, const MapTable& t, const MapComponents& c, uint32_t* blk, uint32_t* tiles)
{
    const uint32_t nb = pc_blocks((size_t)1 << t.cap_log2);
    hipLaunchKernelGGL(k_map_comp_root_count, dim3(nb), dim3(kPcBlock), 0, s, c.parent, blk);
    return pc_scan(s, blk, nb, tiles);
}

hipError_t launch_map_components_list(hipStream_t s, const MapTable& t, const MapComponents& c, const uint32_t* blk,
                                      unsigned long long* label_out, unsigned long long* cells_out, unsigned long long* points_out)
{
    hipLaunchKernelGGL(k_map_comp_list, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s,
                       t.cap_log2, c, blk, label_out, cells_out, points_out);
    return hipExtGetLastError();
}

hipError_t launch_map_knn_points(hipStream_t s, const MapTable& t, const MapKnn& o, const float* pts, uint32_t stride, uint32_t n,
                                 unsigned long long* keys, float* dist, uint8_t* found)
{
    if (n == 0) return hipSuccess;
    const dim3 grid(std::min(pc_blocks(n), kMapRenderMaxBlocks)), block(kPcBlock);
    // (the instantiation is the smallest K >= k: its list's first k are the result)
    if (o.k <= 1)
        hipLaunchKernelGGL(k_map_knn_points<1>, grid, block, 0, s, t, o, pts, stride, n, keys, dist, found);
    else if (o.k <= 2)
        hipLaunchKernelGGL(k_map_knn_points<2>, grid, block, 0, s, t, o, pts, stride, n, keys, dist, found);
    else if (o.k <= 4)
        hipLaunchKernelGGL(k_map_knn_points<4>, grid, block, 0, s, t, o, pts, stride, n, keys, dist, found);
    else if (o.k <= 8)
        hipLaunchKernelGGL(k_map_knn_points<8>, grid, block, 0, s, t, o, pts, stride, n, keys, dist, found);
    else
        hipLaunchKernelGGL(k_map_knn_points<16>, grid, block, 0, s, t, o, pts, stride, n, keys, dist, found);
    return hipExtGetLastError();
}

hipError_t launch_map_knn_self(hipStream_t s, const MapTable& t, const MapKnn& o, const MapKnnCells& c, unsigned long long* ctr)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, kMapKnnCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 grid(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), block(kPcBlock);
    if (o.k <= 1)
        hipLaunchKernelGGL(k_map_knn_self<1>, grid, block, 0, s, t, o, c, ctr);
    else if (o.k <= 2)
        hipLaunchKernelGGL(k_map_knn_self<2>, grid, block, 0, s, t, o, c, ctr);
    else if (o.k <= 4)
        hipLaunchKernelGGL(k_map_knn_self<4>, grid, block, 0, s, t, o, c, ctr);
    else if (o.k <= 8)
        hipLaunchKernelGGL(k_map_knn_self<8>, grid, block, 0, s, t, o, c, ctr);
    else
        hipLaunchKernelGGL(k_map_knn_self<16>, grid, block, 0, s, t, o, c, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_knn_select(hipStream_t s, const MapTable& t, const MapKnn& o, const MapKnnCells& c, int use_threshold, uint32_t T_q,
                                 uint8_t* reason, unsigned long long* ctr)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, kMapKnnSelectCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_knn_select, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t, o,
                       c, use_threshold, T_q, reason, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_knn_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const MapKnnCells& c,
                                 const uint8_t* reason, const uint32_t* blk, unsigned long long* key_out, uint8_t* found_out,
                                 float* mean_out, uint32_t* q_out, uint8_t* reason_out)
{
    hipLaunchKernelGGL(k_map_knn_gather, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t,
                       min_points, min_windows, c, reason, blk, key_out, found_out, mean_out, q_out, reason_out);
    return hipExtGetLastError();
}

hipError_t launch_map_pca(hipStream_t s, const MapTable& t, const MapPca& o, const MapPcaCells& c, unsigned long long* ctr)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, kMapPcaCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 grid(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), block(kPcBlock);
    // (the instantiation is the smallest K >= k: its list's first k are the neighbourhood; 0 is the radius search)
    if (o.q.k <= 0)
        hipLaunchKernelGGL(k_map_pca<0>, grid, block, 0, s, t, o, c, ctr);
    else if (o.q.k <= 1)
        hipLaunchKernelGGL(k_map_pca<1>, grid, block, 0, s, t, o, c, ctr);
    else if (o.q.k <= 2)
        hipLaunchKernelGGL(k_map_pca<2>, grid, block, 0, s, t, o, c, ctr);
    else if (o.q.k <= 4)
        hipLaunchKernelGGL(k_map_pca<4>, grid, block, 0, s, t, o, c, ctr);
    else if (o.q.k <= 8)
        hipLaunchKernelGGL(k_map_pca<8>, grid, block, 0, s, t, o, c, ctr);
    else
        hipLaunchKernelGGL(k_map_pca<16>, grid, block, 0, s, t, o, c, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_pca_select(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const uint8_t* label,
                                 uint32_t keep_labels, int remove_sparse, uint8_t* reason, unsigned long long* ctr)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, kMapPcaSelectCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_pca_select, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t,
                       min_points, min_windows, label, keep_labels, remove_sparse, reason, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_pca_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows, const MapPcaCells& c,
                                 const uint8_t* reason, const uint32_t* blk, unsigned long long* key_out, const MapPcaCells& out,
                                 uint8_t* reason_out)
{
    hipLaunchKernelGGL(k_map_pca_gather, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t,
                       min_points, min_windows, c, reason, blk, key_out, out, reason_out);
    return hipExtGetLastError();
}

hipError_t launch_map_observe(hipStream_t s, const MapTable& t, const MapObserve& o, double leaf, const float* depth, const uint8_t* mask,
                              const MapTally& c, unsigned long long* ctr)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, kMapObserveCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 grid(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), block(kPcBlock);
    switch (o.window) {
    case 0: hipLaunchKernelGGL(k_map_observe<0>, grid, block, 0, s, t, o, leaf, depth, mask, c, ctr); break;
    case 1: hipLaunchKernelGGL(k_map_observe<1>, grid, block, 0, s, t, o, leaf, depth, mask, c, ctr); break;
    case 2: hipLaunchKernelGGL(k_map_observe<2>, grid, block, 0, s, t, o, leaf, depth, mask, c, ctr); break;
    case 3: hipLaunchKernelGGL(k_map_observe<3>, grid, block, 0, s, t, o, leaf, depth, mask, c, ctr); break;
    default: return hipErrorInvalidValue;
    }
    return hipExtGetLastError();
}

hipError_t launch_map_visibility_select(hipStream_t s, const MapTable& t, const MapTally& c, uint32_t min_through, uint32_t agree_weight,
                                        uint8_t* reason, unsigned long long* ctr)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, kMapVisibilitySelectCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_visibility_select, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s,
                       t, c, min_through, agree_weight, reason, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_visibility_gather(hipStream_t s, const MapTable& t, const MapTally& c, const uint8_t* reason, const uint32_t* blk,
                                        unsigned long long* key_out, const MapTally& out, uint8_t* reason_out)
{
    hipLaunchKernelGGL(k_map_visibility_gather, dim3(pc_blocks((size_t)1 << t.cap_log2)), dim3(kPcBlock), 0, s, t, c, reason, blk, key_out, out,
                       reason_out);
    return hipExtGetLastError();
}

hipError_t launch_map_export(hipStream_t s, const MapTable& t, const uint32_t* blk, unsigned long long* key_out, uint32_t* n_out,
                             unsigned long long* sums_out, uint32_t* w_out, uint32_t* stamp_out)
{
    hipLaunchKernelGGL(k_map_export, dim3(std::min(pc_blocks((size_t)1 << t.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, t, blk,
                       key_out, n_out, sums_out, w_out, stamp_out);
    return hipExtGetLastError();
}

hipError_t launch_map_import_build(hipStream_t s, const unsigned long long* keys, const uint32_t* n, const unsigned long long* sums,
                                   const uint32_t* windows, const uint32_t* stamp, uint32_t m, uint32_t calls, const MapTable& to,
                                   unsigned long long* ctr)
{
    hipError_t e = hipMemsetAsync(ctr, 0, kMapImportCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess || m == 0) return e;
    hipLaunchKernelGGL(k_map_import_build, dim3(std::min(pc_blocks(m), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, keys, n, sums, windows,
                       stamp, m, calls, to, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_merge(hipStream_t s, const MapTable& src, const MapTable& dst, uint32_t off, unsigned long long add_accepted,
                            unsigned long long add_rejected, unsigned long long* ctr, unsigned long long* mctr)
{
    hipError_t e = hipMemsetAsync(mctr, 0, kMapMergeCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_merge, dim3(std::min(pc_blocks((size_t)1 << src.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, src,
                       dst, off, add_accepted, add_rejected, ctr, mctr);
    return hipExtGetLastError();
}

hipError_t launch_map_align_step(hipStream_t s, const MapTable& a, const MapTable& b, const MapAlign& o, unsigned long long* key_b,
                                 float* dist, unsigned long long* ctr)
{
    hipError_t e = hipMemsetAsync(ctr, 0, kMapAlignCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_align_step, dim3(std::min(pc_blocks((size_t)1 << a.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0, s, a,
                       b, o, key_b, dist, ctr);
    return hipExtGetLastError();
}

hipError_t launch_map_align_gather(hipStream_t s, const MapTable& t, uint32_t min_points, uint32_t min_windows,
                                   const unsigned long long* key_b, const float* dist, const uint32_t* blk, unsigned long long* key_a_out,
                                   unsigned long long* key_b_out, float* dist_out)
{
    const uint32_t nb = pc_blocks((size_t)1 << t.cap_log2);
    hipLaunchKernelGGL(k_map_align_gather, dim3(nb), dim3(kPcBlock), 0, s, t, min_points, min_windows, key_b, dist, blk, key_a_out,
                       key_b_out, dist_out);
    return hipExtGetLastError();
}

hipError_t launch_map_integrate_map(hipStream_t s, const MapTable& src, uint32_t min_points, uint32_t min_windows, double leaf_src,
                                    const double T_in[12], double leaf, uint32_t serial, const MapTable& dst, unsigned long long* ctr)
{
    MapPose T;
    for (int k = 0; k < 12; ++k) T.m[k] = T_in[k];
    hipLaunchKernelGGL(k_map_integrate_map, dim3(std::min(pc_blocks((size_t)1 << src.cap_log2), kMapRenderMaxBlocks)), dim3(kPcBlock), 0,
                       s, src, min_points, min_windows, leaf_src, T, leaf, serial, dst, ctr);
    return hipExtGetLastError();
}

// ---- focus-based collapses of a DSI (cartesian3dgrid.cpp:139-483; DESIGN.md "Focus-based collapses") ----
//
// Every z-slice of the volume is filtered by a 2-D separable stencil (Sobel, Laplacian, Gaussian) and a focus value
// per pixel is formed; the collapses keep the first plane of strictly largest focus (conf starts at +0, so values
// <= 0 and NaN are never taken), the local-focus transform writes the focus volume itself.  Arithmetic (the project's
// definition, restated in tests/focus_reference.py): OpenCV's borderInterpolate per axis (REFLECT_101 for Sobel and
// Laplacian, REFLECT for GaussianBlur), rows filtered first into fp32, then columns; a symmetric tap set is
// s = S0*c0, then s = s + (S[-j] + S[j])*cj for j = 1..r; an antisymmetric one s = (S[1] - S[-1])*c1; zero taps are
// skipped; fp32 per operation, no contraction.
//
// A workgroup of 256 threads owns a 64 x 16 tile of output pixels and a range of planes.  Per plane: the tile and its
// halo (border-reflected source offsets computed once) go to LDS, a row pass writes the fp32 intermediates to LDS, a
// column pass forms the focus in registers, where the running (conf, idx) of the thread's four pixels stay.  The
// next plane's loads are issued before the current plane is filtered.  The plane range is split over workgroups when
// the tiles alone would not fill the chip; each range leaves one arg-max key per pixel
// ((conf bits << 32) | ~k: conf > 0 and not NaN, so larger bits = larger value, ties to the smaller k) and
// k_focus_finish takes the largest key over the ranges -- the same pick as one strict-'>' walk in ascending k.
namespace {

constexpr int kFocusTX = 64, kFocusTY = 16, kFocusThreads = 256;

// the five collapses of MapperEMVS::getDepthMapFromDSI's switch (mapper_emvs_stereo.cpp:348-364) and the two
// computeLocalFocusInPlace transforms (cartesian3dgrid.cpp:417-483)
enum FocusKind { FK_LOCAL_VAR = 0, FK_LOCAL_MS = 1, FK_GRAD_MAG = 2, FK_LAPLACIAN = 3, FK_DOG = 4, FK_LF_MS = 5, FK_LF_STD = 6 };

// getGaussianKernel(5 | 7, sigma 0.5 | 0.8, CV_32F): the correctly rounded normalised taps
constexpr float kG5_0 = __builtin_bit_cast(float, 0x3f495cb3u), kG5_1 = __builtin_bit_cast(float, 0x3dda02ddu),
                           kG5_2 = __builtin_bit_cast(float, 0x398a575fu);
constexpr float kG7_0 = __builtin_bit_cast(float, 0x3eff5285u), kG7_1 = __builtin_bit_cast(float, 0x3e69ca49u),
                           kG7_2 = __builtin_bit_cast(float, 0x3cb37d42u), kG7_3 = __builtin_bit_cast(float, 0x39e71393u);

// cv::borderInterpolate for BORDER_REFLECT (delta 0) and BORDER_REFLECT_101 (delta 1)
__device__ __forceinline__ int focus_border(int p, int len, int delta)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p - 1 + delta;
        else p = len - 1 - (p - len) - delta;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

template <int ST> __device__ __forceinline__ float gauss5(const float* p)
{
    float s = p[0] * kG5_0;
    s = s + (p[-ST] + p[ST]) * kG5_1;
    s = s + (p[-2 * ST] + p[2 * ST]) * kG5_2;
    return s;
}
template <int ST> __device__ __forceinline__ float gauss5_sq(const float* p)  // gauss5 of the squared samples
{
    const float a = p[-2 * ST], b = p[-ST], c = p[0], d = p[ST], e = p[2 * ST];
    float s = (c * c) * kG5_0;
    s = s + (b * b + d * d) * kG5_1;
    s = s + (a * a + e * e) * kG5_2;
    return s;
}
template <int ST> __device__ __forceinline__ float gauss7(const float* p)
{
    float s = p[0] * kG7_0;
    s = s + (p[-ST] + p[ST]) * kG7_1;
    s = s + (p[-2 * ST] + p[2 * ST]) * kG7_2;
    s = s + (p[-3 * ST] + p[3 * ST]) * kG7_3;
    return s;
}
template <int ST> __device__ __forceinline__ float taps_121(const float* p) { return p[0] * 2.f + (p[-ST] + p[ST]) * 1.f; }
template <int ST> __device__ __forceinline__ float taps_m101(const float* p) { return (p[ST] - p[-ST]) * 1.f; }
template <int ST> __device__ __forceinline__ float taps_14641(const float* p)
{
    float s = p[0] * 6.f;
    s = s + (p[-ST] + p[ST]) * 4.f;
    s = s + (p[-2 * ST] + p[2 * ST]) * 1.f;
    return s;
}
template <int ST> __device__ __forceinline__ float taps_10m201(const float* p) { return p[0] * -2.f + (p[-2 * ST] + p[2 * ST]) * 1.f; }

template <int K> struct FocusTraits;  // R: halo of the source tile; TWO: two intermediates per pixel; DELTA: border
template <> struct FocusTraits<FK_LOCAL_VAR> { static constexpr int R = 2, TWO = 1, DELTA = 0; };
template <> struct FocusTraits<FK_LOCAL_MS> { static constexpr int R = 2, TWO = 0, DELTA = 0; };
template <> struct FocusTraits<FK_GRAD_MAG> { static constexpr int R = 1, TWO = 1, DELTA = 1; };  // + half_patchsize
template <> struct FocusTraits<FK_LAPLACIAN> { static constexpr int R = 2, TWO = 1, DELTA = 1; };
template <> struct FocusTraits<FK_DOG> { static constexpr int R = 3, TWO = 1, DELTA = 0; };
template <> struct FocusTraits<FK_LF_MS> { static constexpr int R = 2, TWO = 0, DELTA = 0; };
template <> struct FocusTraits<FK_LF_STD> { static constexpr int R = 2, TWO = 1, DELTA = 0; };

template <int K>
__device__ __forceinline__ void focus_row(const float* p, float& r0, float& r1)
{
    if constexpr (K == FK_LOCAL_VAR || K == FK_LF_STD) { r0 = gauss5<1>(p); r1 = gauss5_sq<1>(p); }
    else if constexpr (K == FK_LOCAL_MS || K == FK_LF_MS) { r0 = gauss5_sq<1>(p); r1 = 0.f; }
    else if constexpr (K == FK_GRAD_MAG) { r0 = taps_m101<1>(p); r1 = taps_121<1>(p); }      // d/dx row, d/dy row
    else if constexpr (K == FK_LAPLACIAN) { r0 = taps_10m201<1>(p); r1 = taps_14641<1>(p); }  // Dxx row, Dyy row
    else { r0 = gauss5<1>(p); r1 = gauss7<1>(p); }                                          // DoG
}

// focus (for GradMag: the squared gradient magnitude g) from the column pass over the intermediates
template <int K, int ST>
__device__ __forceinline__ float focus_col(const float* q0, const float* q1)
{
    if constexpr (K == FK_LOCAL_VAR || K == FK_LF_STD) {
        const float m = gauss5<ST>(q0), q = gauss5<ST>(q1);
        float v = q - m * m;
        v = v > 0.f ? v : 0.f;  // cv::threshold(THRESH_TOZERO, 0): NaN -> 0
        if constexpr (K == FK_LF_STD) return sqrtf(v);
        return fabsf(v);
    } else if constexpr (K == FK_LOCAL_MS || K == FK_LF_MS) {
        return gauss5<ST>(q0);
    } else if constexpr (K == FK_GRAD_MAG) {
        const float gx = taps_121<ST>(q0), gy = taps_m101<ST>(q1);
        return gx * gx + gy * gy;
    } else if constexpr (K == FK_LAPLACIAN) {
        const float l = taps_14641<ST>(q0) + taps_10m201<ST>(q1);
        return l * l;
    } else {
        return fabsf(gauss5<ST>(q0) - gauss7<ST>(q1));
    }
}

// K: FocusKind; E: GradMag's half_patchsize (0 otherwise).  COLLAPSE: keys[chunk][npix] of the arg-max over the
// workgroup's planes; otherwise out[k][npix] = focus (the local-focus volume).
template <int K, int E, bool COLLAPSE>
__global__ __launch_bounds__(kFocusThreads) void k_focus_tile(const float* __restrict__ src, int nx, int ny, int nz,
                                                              float* __restrict__ out, unsigned long long* __restrict__ keys)
{
    constexpr int R = FocusTraits<K>::R + E, TWO = FocusTraits<K>::TWO, DELTA = FocusTraits<K>::DELTA;
    constexpr int HI = kFocusTY + 2 * R, WI = kFocusTX + 2 * R;  // source tile
    constexpr int WO = kFocusTX + 2 * E;                          // intermediates: HI x WO
    constexpr int HG = kFocusTY + 2 * E;                          // GradMag: g over HG x WO
    constexpr int NL = (HI * WI + kFocusThreads - 1) / kFocusThreads;
    constexpr int PER = kFocusTX * kFocusTY / kFocusThreads;     // output pixels per thread (4)
    static_assert(PER * kFocusThreads == kFocusTX * kFocusTY, "tile");
    __shared__ float s_in[HI * WI];
    __shared__ float s_r0[HI * WO];
    __shared__ float s_r1[TWO ? HI * WO : 1];
    __shared__ float s_g[E ? HG * WO : 1];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kFocusTX, y0 = blockIdx.y * kFocusTY;
    const size_t npix = (size_t)nx * ny;
    const int k0 = (int)((long long)blockIdx.z * nz / gridDim.z), k1 = (int)((long long)(blockIdx.z + 1) * nz / gridDim.z);

    int off[NL];  // border-reflected offsets of the source tile within a plane (-1: no element)
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int i = tid + j * kFocusThreads;
        off[j] = -1;
        if (i < HI * WI) {
            const int yy = i / WI, xx = i - yy * WI;
            off[j] = focus_border(y0 - R + yy, ny, DELTA) * nx + focus_border(x0 - R + xx, nx, DELTA);
        }
    }
    float nxt[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) nxt[j] = off[j] >= 0 ? src[(size_t)k0 * npix + off[j]] : 0.f;
#pragma unroll
    for (int j = 0; j < NL; ++j)
        if (off[j] >= 0) s_in[tid + j * kFocusThreads] = nxt[j];
    __syncthreads();

    float conf[PER];
    int idx[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        conf[t] = 0.f;
        idx[t] = 0;
    }
    const int lx = tid % kFocusTX, ly = tid / kFocusTX;  // pixel t of the thread: (x0 + lx, y0 + ly + 4 t)
    for (int k = k0; k < k1; ++k) {
        if (k + 1 < k1) {  // the next plane's loads in flight while this one is filtered
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (off[j] >= 0) nxt[j] = src[(size_t)(k + 1) * npix + off[j]];
        }
        // row pass: intermediates of rows y0 - R .. y0 + TY + R, columns x0 - E .. x0 + TX + E
        for (int i = tid; i < HI * WO; i += kFocusThreads) {
            const int yy = i / WO, xo = i - yy * WO;
            float r0, r1;
            focus_row<K>(&s_in[yy * WI + xo + (R - E)], r0, r1);
            s_r0[i] = r0;
            if constexpr (TWO != 0) s_r1[i] = r1;
        }
        __syncthreads();
        float f[PER];
        if constexpr (E == 0) {  // (GradMag with half_patchsize 0: the mean of one g is g)
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                const int c = (ly + 4 * t + R) * WO + lx;
                f[t] = focus_col<K, WO>(&s_r0[c], TWO ? &s_r1[c] : nullptr);
            }
        } else {
            // GradMag: g over the tile + E on each side, then the (2E+1)^2 patch mean in double, row-major
            for (int i = tid; i < HG * WO; i += kFocusThreads) {
                const int yo = i / WO, xo = i - yo * WO;
                const int c = (yo + (R - E)) * WO + xo;
                s_g[i] = focus_col<K, WO>(&s_r0[c], &s_r1[c]);
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                double sum = 0.0;
                const float* g = &s_g[(ly + 4 * t) * WO + lx];
#pragma unroll 1
                for (int dy = 0; dy <= 2 * E; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= 2 * E; ++dx) sum += (double)g[dy * WO + dx];
                f[t] = (float)(sum * (1.0 / (double)((2 * E + 1) * (2 * E + 1))));
            }
        }
        if constexpr (COLLAPSE) {
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                bool ok = true;
                if constexpr (K == FK_GRAD_MAG) {  // cartesian3dgrid.cpp:225-226: only [h, n - h) in x and y
                    const int x = x0 + lx, y = y0 + ly + 4 * t;
                    ok = x >= E && x < nx - E && y >= E && y < ny - E;
                }
                if (ok && f[t] > conf[t]) {
                    conf[t] = f[t];
                    idx[t] = k;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                const int x = x0 + lx, y = y0 + ly + 4 * t;
                if (x < nx && y < ny) out[(size_t)k * npix + (size_t)y * nx + x] = f[t];
            }
        }
        if (k + 1 < k1) {
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (off[j] >= 0) s_in[tid + j * kFocusThreads] = nxt[j];
        }
        __syncthreads();
    }
    if constexpr (COLLAPSE) {
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int x = x0 + lx, y = y0 + ly + 4 * t;
            if (x < nx && y < ny) {
                const unsigned long long key =
                    conf[t] > 0.f ? ((unsigned long long)__float_as_uint(conf[t]) << 32) | (0xffffffffu - (unsigned)idx[t]) : 0ull;
                keys[(size_t)blockIdx.z * npix + (size_t)y * nx + x] = key;
            }
        }
    }
}

// the largest key over the plane ranges; conf = +0, idx = 0 where no plane was taken; sqrtf for GradMag / LaplacianMag
__global__ __launch_bounds__(256) void k_focus_finish(const unsigned long long* __restrict__ keys, int npix, int chunks,
                                                      int take_sqrt, float* __restrict__ conf, uint8_t* __restrict__ idx,
                                                      const float* __restrict__ planes, float* __restrict__ depth)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    unsigned long long best = 0;
    for (int c = 0; c < chunks; ++c) {
        const unsigned long long v = keys[(size_t)c * npix + p];
        best = v > best ? v : best;
    }
    float v = __uint_as_float((unsigned)(best >> 32));
    const int k = best ? (int)(0xffffffffu - (unsigned)best) : 0;
    if (take_sqrt) v = sqrtf(v);
    conf[p] = v;
    idx[p] = (uint8_t)k;
    if (depth) depth[p] = planes[k];
}

// Grid3D::collapseMinZSlice (cartesian3dgrid.cpp:139-161): std::min_element, the first minimum wins -- the mirror of
// k_collapse_max_z
__global__ __launch_bounds__(256) void k_collapse_min_z(const float* __restrict__ dsi, int npix, int nz,
                                                        float* __restrict__ val, uint8_t* __restrict__ idx)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float* col = dsi + p;
    float best = col[0];
    int best_k = 0;
    int k = 1;
    for (; k + 8 <= nz; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(size_t)(k + u) * npix];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (v[u] < best) {
                best = v[u];
                best_k = k + u;
            }
    }
    for (; k < nz; ++k) {
        const float v = col[(size_t)k * npix];
        if (v < best) {
            best = v;
            best_k = k;
        }
    }
    val[p] = best;
    idx[p] = (uint8_t)best_k;
}

template <int K, int E, bool COLLAPSE>
hipError_t focus_launch(hipStream_t s, const float* src, int nx, int ny, int nz, int chunks, float* out,
                        unsigned long long* keys)
{
    const dim3 grid((nx + kFocusTX - 1) / kFocusTX, (ny + kFocusTY - 1) / kFocusTY, chunks);
    hipLaunchKernelGGL((k_focus_tile<K, E, COLLAPSE>), grid, dim3(kFocusThreads), 0, s, src, nx, ny, nz, out, keys);
    return hipExtGetLastError();
}

}  // namespace

int focus_chunks(int nx, int ny, int nz)
{
    // about four workgroups per CU of the 256, with at least 4 planes per range
    const long long tiles = (long long)((nx + kFocusTX - 1) / kFocusTX) * ((ny + kFocusTY - 1) / kFocusTY);
    long long c = (1024 + tiles - 1) / tiles;
    c = std::min<long long>(c, std::max(1, nz / 4));
    return (int)std::max<long long>(1, c);
}

hipError_t launch_focus_collapse(hipStream_t s, const float* dsi, int nx, int ny, int nz, int method, int half_patchsize,
                                 unsigned long long* keys, float* conf, uint8_t* idx, const float* planes, float* depth)
{
    const int chunks = focus_chunks(nx, ny, nz);
    hipError_t e = hipErrorInvalidValue;
    switch (method) {
    case FK_LOCAL_VAR: e = focus_launch<FK_LOCAL_VAR, 0, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
    case FK_LOCAL_MS: e = focus_launch<FK_LOCAL_MS, 0, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
    case FK_GRAD_MAG:
        switch (half_patchsize) {
        case 0: e = focus_launch<FK_GRAD_MAG, 0, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 1: e = focus_launch<FK_GRAD_MAG, 1, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 2: e = focus_launch<FK_GRAD_MAG, 2, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 3: e = focus_launch<FK_GRAD_MAG, 3, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 4: e = focus_launch<FK_GRAD_MAG, 4, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 5: e = focus_launch<FK_GRAD_MAG, 5, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 6: e = focus_launch<FK_GRAD_MAG, 6, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 7: e = focus_launch<FK_GRAD_MAG, 7, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        case 8: e = focus_launch<FK_GRAD_MAG, 8, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
        default: return hipErrorInvalidValue;
        }
        break;
    case FK_LAPLACIAN: e = focus_launch<FK_LAPLACIAN, 0, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
    case FK_DOG: e = focus_launch<FK_DOG, 0, true>(s, dsi, nx, ny, nz, chunks, nullptr, keys); break;
    default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    const int npix = nx * ny;
    const int take_sqrt = method == FK_GRAD_MAG || method == FK_LAPLACIAN;  // cartesian3dgrid.cpp:243, :283
    hipLaunchKernelGGL(k_focus_finish, dim3((npix + 255) / 256), dim3(256), 0, s, keys, npix, chunks, take_sqrt, conf, idx,
                       planes, depth);
    return hipExtGetLastError();
}

hipError_t launch_local_focus(hipStream_t s, const float* src, float* dst, int nx, int ny, int nz, int focus_method)
{
    const int chunks = focus_chunks(nx, ny, nz);
    if (focus_method == 1) return focus_launch<FK_LF_MS, 0, false>(s, src, nx, ny, nz, chunks, dst, nullptr);
    return focus_launch<FK_LF_STD, 0, false>(s, src, nx, ny, nz, chunks, dst, nullptr);  // any other value: :423-425
}

hipError_t launch_collapse_min_z(hipStream_t s, const float* dsi, int nx, int ny, int nz, float* val, uint8_t* idx)
{
    const int npix = nx * ny;
    hipLaunchKernelGGL(k_collapse_min_z, dim3((npix + 255) / 256), dim3(256), 0, s, dsi, npix, nz, val, idx);
    return hipExtGetLastError();
}

// ------------------------------------------------- Grid3D: the rest of the class ---
// subtractTwoGrids / ratioTwoGrids / quadraticMeanTwoGrids / cubicMeanTwoGrids (cartesian3dgrid.h:95-109,166-184), getMinMax
// (cartesian3dgrid.cpp:177-188), getSlice (:72-113), accumulateZSliceAt (.h:195-204) and the 8-bit slice images of
// imwriteSlices (cartesian3dgrid_IO.cpp:39-76).  Arithmetic: DESIGN.md 7d.
namespace {

// the float nearest to the real cube root of x.  The estimate y (good to an ulp or two of a double) rounds to the right
// float unless it lies next to the midpoint m of two floats; there m^3 is compared with |x| exactly: m has 25 significant
// bits, so m*m is exact, (m*m)*m = h + e with e from one FMA, and m^3 (75 significant bits) never equals a double.
__device__ __forceinline__ float cbrt_rn_f32(double x)
{
    if (!(x == x) || x == 0.0 || __builtin_isinf(x)) return (float)x;  // cbrt keeps +-0, +-inf and NaN
    const double ax = __builtin_fabs(x);
    const double y = cbrt(ax);
    float f = (float)y;  // a normal float: |x| >= 2^-150, so y >= 2^-50
    const double fd = (double)f;
    const float o = __uint_as_float(fd <= y ? __float_as_uint(f) + 1u : __float_as_uint(f) - 1u);
    const double mid = 0.5 * (fd + (double)o);
    if (__builtin_fabs(y - mid) <= y * 0x1p-48) {
        const double p = mid * mid;
        const double h = p * mid;
        const double e = __builtin_fma(p, mid, -h);
        const bool mid_below = h < ax || (h == ax && e < 0.0);
        f = mid_below ? (f < o ? o : f) : (f < o ? f : o);
    }
    return x < 0.0 ? -f : f;
}

enum { GRID_OP_SUBTRACT = 1, GRID_OP_RATIO = 2, GRID_OP_QUADRATIC_MEAN = 3, GRID_OP_CUBIC_MEAN = 4 };

template <int OP>
__device__ __forceinline__ float grid_op(float a, float g)
{
    if (OP == GRID_OP_SUBTRACT) return a - g;  // :99
    if (OP == GRID_OP_RATIO)                   // :107, fabs is double fabs(double) there: sum and quotient in double
        return (float)((double)a / (__builtin_fabs((double)g) + (double)0.1f));
    if (OP == GRID_OP_QUADRATIC_MEAN) {        // :170-172, float sum of squares, 0.5 and sqrt in double
        const float s = a * a + g * g;
        return (float)sqrt(0.5 * (double)s);
    }
    const float s = (a * a) * a + (g * g) * g;  // :180-182
    return cbrt_rn_f32(0.5 * (double)s);
}

template <int OP>
struct GridOp : VoxelValue<1, true> {
    __device__ float operator()(const float* x, const double2*) const { return grid_op<OP>(x[0], x[1]); }
};

// std::minmax_element: the FIRST smallest and the LAST largest element.  (value, position) pairs under a total order --
// equal values (+0 and -0 included) are told apart by position -- so any reduction tree gives the same answer.
struct MinMaxItem {
    float mn, mx;
    unsigned long long mn_pos, mx_pos;
};
__device__ __forceinline__ void minmax_merge(MinMaxItem& a, float mn, unsigned long long mn_pos, float mx, unsigned long long mx_pos)
{
    if (mn < a.mn || (mn == a.mn && mn_pos < a.mn_pos)) {
        a.mn = mn;
        a.mn_pos = mn_pos;
    }
    if (mx > a.mx || (mx == a.mx && mx_pos > a.mx_pos)) {
        a.mx = mx;
        a.mx_pos = mx_pos;
    }
}
// a thread visits its elements in ascending position: a strictly smaller value replaces the minimum, a larger OR EQUAL one
// the maximum.  The neutral items (+inf at the last possible position, -inf at position 0) lose every tie.
__device__ __forceinline__ void minmax_take(MinMaxItem& a, float v, unsigned long long pos)
{
    if (v < a.mn || (v == a.mn && pos < a.mn_pos)) {
        a.mn = v;
        a.mn_pos = pos;
    }
    if (v >= a.mx) {
        a.mx = v;
        a.mx_pos = pos;
    }
}
__device__ __forceinline__ MinMaxItem minmax_block_reduce(MinMaxItem it, MinMaxItem* part)
{
    for (int off = 32; off > 0; off >>= 1) {
        const float mn = __shfl_down(it.mn, off, 64), mx = __shfl_down(it.mx, off, 64);
        const unsigned long long mn_pos = __shfl_down(it.mn_pos, off, 64), mx_pos = __shfl_down(it.mx_pos, off, 64);
        minmax_merge(it, mn, mn_pos, mx, mx_pos);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = it;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) minmax_merge(it, part[w].mn, part[w].mn_pos, part[w].mx, part[w].mx_pos);
    return it;  // thread 0 holds the block's item
}

__global__ __launch_bounds__(256) void k_grid_min_max(const float* __restrict__ vol, size_t n, MinMaxItem* __restrict__ partials)
{
    __shared__ MinMaxItem part[4];
    MinMaxItem it{INFINITY, -INFINITY, ~0ull, 0ull};
    const size_t n4 = n / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(vol)[i];
        minmax_take(it, v.x, 4 * i);
        minmax_take(it, v.y, 4 * i + 1);
        minmax_take(it, v.z, 4 * i + 2);
        minmax_take(it, v.w, 4 * i + 3);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // the tail lies behind everything this thread has seen
        const size_t i = n4 * 4 + threadIdx.x;
        minmax_take(it, vol[i], i);
    }
    it = minmax_block_reduce(it, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = it;
}

// the finishing step: one workgroup folds the partials; positions of a volume without any comparable value (all NaN:
// unspecified result) are clamped into the volume
__global__ __launch_bounds__(256) void k_grid_min_max_finish(const MinMaxItem* __restrict__ partials, int n_part, size_t n,
                                                             MinMaxItem* __restrict__ result)
{
    __shared__ MinMaxItem part[4];
    MinMaxItem it{INFINITY, -INFINITY, ~0ull, 0ull};
    for (int i = threadIdx.x; i < n_part; i += 256)
        minmax_merge(it, partials[i].mn, partials[i].mn_pos, partials[i].mx, partials[i].mx_pos);
    it = minmax_block_reduce(it, part);
    if (threadIdx.x == 0) {
        if (it.mn_pos >= n) it.mn_pos = n - 1;
        if (it.mx_pos >= n) it.mx_pos = n - 1;
        *result = it;
    }
}

// getSlice: one thread per output element
__global__ __launch_bounds__(256) void k_grid_get_slice(const float* __restrict__ vol, int nx, int ny, int nz, int slice, int dim,
                                                        float* __restrict__ out)
{
    const int cols = dim == 2 ? nx : nz, rows = dim == 0 ? ny : (dim == 1 ? nx : ny);
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= rows * cols) return;
    const int v = o / cols, u = o - v * cols;
    size_t src;
    if (dim == 0) src = ((size_t)u * ny + v) * nx + slice;       // (x = slice, y = v, z = u)
    else if (dim == 1) src = ((size_t)u * ny + slice) * nx + v;  // (x = v, y = slice, z = u)
    else src = ((size_t)slice * ny + v) * nx + u;                // (x = u, y = v, z = slice)
    out[o] = vol[src];
}

// accumulateZSliceAt: vol(ix, iy, iz) += img(iy, ix), one thread per image element
__global__ __launch_bounds__(256) void k_grid_accumulate_z_slice(float* __restrict__ vol, int nx, int ny, int iz,
                                                                 const float* __restrict__ img, int rows, int cols)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= rows * cols) return;
    const int iy = o / cols, ix = o - iy * cols;
    const size_t p = ((size_t)iz * ny + iy) * nx + ix;
    vol[p] = vol[p] + img[o];
}

// ---- slice images.  cvRound + saturate_cast<uchar>: nearest, ties to even, clamped, NaN -> 0
__device__ __forceinline__ uint32_t round_u8(float w)
{
    if (!(w == w)) return 0u;
    const float r = __builtin_rintf(w);
    return (uint32_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}
// normalize_by_minmax: (v - min) / range * 255, three roundings.  Per slice: v * a + b, two roundings (a, b of cv::normalize)
template <bool MINMAX>
__device__ __forceinline__ uint32_t slice_u8(float v, float p0, float p1)
{
    if (MINMAX) {
        float t = v - p0;
        t = t / p1;
        return round_u8(t * 255.f);
    }
    const float t = v * p0;
    return round_u8(t + p1);
}

// per-slice minima and maxima of one orientation in ONE pass over the volume, as monotone integer keys (integer atomics:
// min and max are exact in any order).  keys[2 s], keys[2 s + 1]: min and max of slice s, preset to 0xffffffff / 0.
// DIM 0: thread = x column of a chunk of (y, z) rows; DIM 1 / 2: blockIdx.y = the slice, the loop runs over the other axis.
template <int DIM>
__global__ __launch_bounds__(256) void k_grid_slice_minmax(const float* __restrict__ vol, int nx, int ny, int nz, int rows_per_block,
                                                           uint32_t* __restrict__ keys)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    if (DIM == 0) {
        if (x >= nx) return;
        const size_t rows = (size_t)ny * nz;
        const size_t r0 = (size_t)blockIdx.y * rows_per_block;
        const size_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
        for (size_t r = r0; r < r1; ++r) {
            const float v = vol[r * nx + x];
            if (v == v) {
                const uint32_t k = float_key(v);
                kmin = k < kmin ? k : kmin;
                kmax = k > kmax ? k : kmax;
            }
        }
        if (kmin <= kmax) {
            atomicMin(&keys[2 * x], kmin);
            atomicMax(&keys[2 * x + 1], kmax);
        }
        return;
    }
    const int s = blockIdx.y;
    const int n_other = DIM == 1 ? nz : ny;
    if (x < nx)
        for (int j = 0; j < n_other; ++j) {
            const size_t row = DIM == 1 ? (size_t)j * ny + s : (size_t)s * ny + j;
            const float v = vol[row * nx + x];
            if (v == v) {
                const uint32_t k = float_key(v);
                kmin = k < kmin ? k : kmin;
                kmax = k > kmax ? k : kmax;
            }
        }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t a = __shfl_down(kmin, off, 64), b = __shfl_down(kmax, off, 64);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63) == 0 && kmin <= kmax) {
        atomicMin(&keys[2 * s], kmin);
        atomicMax(&keys[2 * s + 1], kmax);
    }
}

__global__ __launch_bounds__(256) void k_grid_slice_keys_init(uint32_t* __restrict__ keys, int n_slices)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slices) return;
    keys[2 * s] = 0xffffffffu;
    keys[2 * s + 1] = 0u;
}

// cv::normalize(NORM_MINMAX, 0, 255): scale = 255 * (1 / (smax - smin)) if smax - smin > DBL_EPSILON else 0, shift =
// -smin * scale, in double, both cast to float (the arithmetic of the confidence image, k_conf8's)
__global__ __launch_bounds__(256) void k_grid_slice_scale(const uint32_t* __restrict__ keys, int n_slices, float2* __restrict__ ab)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slices) return;
    const double smin = (double)key_float(keys[2 * s]), smax = (double)key_float(keys[2 * s + 1]);
    const double rng = smax - smin;
    const double scale = 255.0 * (rng > 2.220446049250313e-16 ? 1.0 / rng : 0.0);
    const double shift = 0.0 - smin * scale;
    ab[s] = make_float2((float)scale, (float)shift);
}

// dim_idx 2: the images are the volume's own planes -- a streaming conversion, four voxels to one packed word
template <bool MINMAX, typename IDX>
__global__ __launch_bounds__(256) void k_grid_slices_u8_z(const float* __restrict__ vol, size_t n, IDX npix,
                                                          const MinMaxItem* __restrict__ mm, const float2* __restrict__ ab,
                                                          uint8_t* __restrict__ out)
{
    float p0 = 0.f, p1 = 0.f;
    if (MINMAX) {
        p0 = mm->mn;
        p1 = mm->mx - mm->mn;
    }
    const size_t n4 = n / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(vol)[i];
        const float e[4] = {v.x, v.y, v.z, v.w};
        IDX z = 0, r = 0;
        if (!MINMAX) {
            z = (IDX)(4 * i) / npix;
            r = (IDX)(4 * i) - z * npix;
        }
        uint32_t pk = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!MINMAX) {
                while (r >= npix) {
                    r -= npix;
                    ++z;
                }
                const float2 c = ab[z];
                p0 = c.x;
                p1 = c.y;
                ++r;
            }
            pk |= slice_u8<MINMAX>(e[k], p0, p1) << (8 * k);
        }
        reinterpret_cast<uint32_t*>(out)[i] = pk;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = n4 * 4 + threadIdx.x;
        if (!MINMAX) {
            const float2 c = ab[i / npix];
            p0 = c.x;
            p1 = c.y;
        }
        out[i] = (uint8_t)slice_u8<MINMAX>(vol[i], p0, p1);
    }
}

// dim_idx 0 (out[x][y][z]) and 1 (out[y][x][z]): z becomes the fastest axis, so for a fixed y a 64 x 64 tile of (x, z)
// goes through LDS, ALREADY AS BYTES: a thread converts four consecutive z of its x and stores them as one word.
//   global reads   a wave reads 64 consecutive x of one (y, z) row: 256 contiguous bytes
//   LDS            word (x, d) of the tile -- d = z / 4 -- lies at x * 16 + ((d + x / 2) & 15).  The store (32 lanes = 32
//                  consecutive x, one d) hits banks 16 (x & 1) + ((d + x / 2) & 15): all different.  The transposed load (32
//                  lanes = 2 consecutive x, 16 d) hits 16 (x & 1) + a rotation of 0..15: all different.  (A rotation where
//                  one would pad: a row pitch of 17 words keeps the store conflict-free but makes rows x and x + 1 collide
//                  in one bank of the load; 64 banks of 4 bytes, ds_read/write_b32 served in two groups of 32 lanes.)
//   global writes  16 lanes write the 64 contiguous bytes of one (x, y) row, a wave four such rows; words when dimZ is a
//                  multiple of 4 (every row then starts on a word), bytes otherwise
// out[x * stride_x + y * stride_y + z]; slice_is_x selects the per-slice (a, b) by x (dim_idx 0) or by y (dim_idx 1).
template <bool MINMAX>
__global__ __launch_bounds__(256) void k_grid_slices_u8(const float* __restrict__ vol, int nx, int ny, int nz, size_t stride_x,
                                                        size_t stride_y, int slice_is_x, int words,
                                                        const MinMaxItem* __restrict__ mm, const float2* __restrict__ ab,
                                                        uint8_t* __restrict__ out)
{
    __shared__ uint32_t tile[64 * 16];
    const int y = blockIdx.x, z0 = blockIdx.y * 64, x0 = blockIdx.z * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int x = x0 + lane;
    float p0 = 0.f, p1 = 0.f;
    if (MINMAX) {
        p0 = mm->mn;
        p1 = mm->mx - mm->mn;
    } else if (x < nx) {
        const float2 c = ab[slice_is_x ? x : y];
        p0 = c.x;
        p1 = c.y;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = w + 4 * j;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int z = z0 + 4 * d + k;
            v[k] = (x < nx && z < nz) ? vol[((size_t)z * ny + y) * nx + x] : 0.f;
        }
        uint32_t pk = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) pk |= slice_u8<MINMAX>(v[k], p0, p1) << (8 * k);
        tile[lane * 16 + ((d + (lane >> 1)) & 15)] = pk;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xl = (threadIdx.x >> 4) + 16 * j, d = threadIdx.x & 15;
        const uint32_t pk = tile[xl * 16 + ((d + (xl >> 1)) & 15)];
        const int xo = x0 + xl, z = z0 + 4 * d;
        if (xo < nx && z < nz) {
            uint8_t* o = out + (size_t)xo * stride_x + (size_t)y * stride_y + z;
            if (words) {
                *reinterpret_cast<uint32_t*>(o) = pk;
            } else {
                for (int k = 0; k < 4 && z + k < nz; ++k) o[k] = (uint8_t)(pk >> (8 * k));
            }
        }
    }
}

}  // namespace

size_t grid_min_max_words() { return (sizeof(MinMaxItem) / 8) * (size_t)(kGridMinMaxBlocks + 1); }

hipError_t launch_grid_binary(hipStream_t s, float* a, const float* g, size_t n, int op)
{
    return dispatch_int<1, 4>(op, [&](auto OP) { return launch_voxelwise(s, a, FuseSources{{g}}, n, GridOp<OP>()); });
}

hipError_t launch_grid_min_max(hipStream_t s, const float* vol, size_t n, unsigned long long* words, int max_blocks)
{
    static_assert(sizeof(MinMaxItem) == 24, "three words per item");
    MinMaxItem* items = reinterpret_cast<MinMaxItem*>(words);  // [0]: the result, [1..]: one partial per workgroup
    if (max_blocks < 1 || max_blocks > kGridMinMaxBlocks) max_blocks = kGridMinMaxBlocks;
    const int blocks = grid_for(n / 4 + 1, 256, max_blocks);
    hipLaunchKernelGGL(k_grid_min_max, dim3(blocks), dim3(256), 0, s, vol, n, items + 1);
    hipError_t e = hipExtGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_grid_min_max_finish, dim3(1), dim3(256), 0, s, items + 1, blocks, n, items);
    return hipExtGetLastError();
}

hipError_t launch_grid_get_slice(hipStream_t s, const float* vol, int nx, int ny, int nz, int slice, int dim, float* out)
{
    const size_t count = dim == 0 ? (size_t)ny * nz : (dim == 1 ? (size_t)nx * nz : (size_t)nx * ny);
    if (count > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_grid_get_slice, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, vol, nx, ny, nz, slice, dim, out);
    return hipExtGetLastError();
}

hipError_t launch_grid_accumulate_z_slice(hipStream_t s, float* vol, int nx, int ny, int iz, const float* img, int rows, int cols)
{
    const size_t count = (size_t)rows * cols;
    if (count == 0) return hipSuccess;
    if (count > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_grid_accumulate_z_slice, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, vol, nx, ny, iz, img, rows,
                       cols);
    return hipExtGetLastError();
}

// words: grid_min_max_words() for the volume's extremes, then one word of keys and one word of (a, b) per slice
hipError_t launch_grid_slices_u8(hipStream_t s, const float* vol, int nx, int ny, int nz, int dim, int normalize_by_minmax,
                                 unsigned long long* words, uint8_t* out)
{
    const size_t n = (size_t)nx * ny * nz;
    const int n_slices = dim == 0 ? nx : (dim == 1 ? ny : nz);
    const MinMaxItem* mm = reinterpret_cast<const MinMaxItem*>(words);
    uint32_t* keys = reinterpret_cast<uint32_t*>(words + grid_min_max_words());
    float2* ab = reinterpret_cast<float2*>(words + grid_min_max_words() + n_slices);
    hipError_t e;
    if (normalize_by_minmax) {
        if ((e = launch_grid_min_max(s, vol, n, words, 0)) != hipSuccess) return e;
    } else {
        hipLaunchKernelGGL(k_grid_slice_keys_init, dim3((n_slices + 255) / 256), dim3(256), 0, s, keys, n_slices);
        if ((e = hipExtGetLastError()) != hipSuccess) return e;
        const unsigned xb = (unsigned)((nx + 255) / 256);
        if (dim == 0) {
            const size_t rows = (size_t)ny * nz;
            const int rows_per_block = (int)((rows + 1023) / 1024 < 16 ? 16 : (rows + 1023) / 1024);
            const unsigned yb = (unsigned)((rows + rows_per_block - 1) / rows_per_block);
            hipLaunchKernelGGL(k_grid_slice_minmax<0>, dim3(xb, yb), dim3(256), 0, s, vol, nx, ny, nz, rows_per_block, keys);
        } else if (dim == 1) {
            hipLaunchKernelGGL(k_grid_slice_minmax<1>, dim3(xb, (unsigned)ny), dim3(256), 0, s, vol, nx, ny, nz, 0, keys);
        } else {
            hipLaunchKernelGGL(k_grid_slice_minmax<2>, dim3(xb, (unsigned)nz), dim3(256), 0, s, vol, nx, ny, nz, 0, keys);
        }
        if ((e = hipExtGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_grid_slice_scale, dim3((n_slices + 255) / 256), dim3(256), 0, s, keys, n_slices, ab);
        if ((e = hipExtGetLastError()) != hipSuccess) return e;
    }
    if (dim == 2) {
        const dim3 grid(grid_for(n / 4 + 1, 256)), block(256);
        const size_t npix = (size_t)nx * ny;
        if (normalize_by_minmax)
            hipLaunchKernelGGL((k_grid_slices_u8_z<true, uint32_t>), grid, block, 0, s, vol, n, 1u, mm, ab, out);
        else if (n <= 0xffffffffull)
            hipLaunchKernelGGL((k_grid_slices_u8_z<false, uint32_t>), grid, block, 0, s, vol, n, (uint32_t)npix, mm, ab, out);
        else
            hipLaunchKernelGGL((k_grid_slices_u8_z<false, size_t>), grid, block, 0, s, vol, n, npix, mm, ab, out);
        return hipExtGetLastError();
    }
    // out[x][y][z] (dim 0) or out[y][x][z] (dim 1)
    const size_t stride_x = dim == 0 ? (size_t)ny * nz : (size_t)nz;
    const size_t stride_y = dim == 0 ? (size_t)nz : (size_t)nx * nz;
    const dim3 grid((unsigned)ny, (unsigned)((nz + 63) / 64), (unsigned)((nx + 63) / 64));
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    const int words_ok = (nz % 4) == 0;
    if (normalize_by_minmax)
        hipLaunchKernelGGL(k_grid_slices_u8<true>, grid, dim3(256), 0, s, vol, nx, ny, nz, stride_x, stride_y, dim == 0, words_ok, mm,
                           ab, out);
    else
        hipLaunchKernelGGL(k_grid_slices_u8<false>, grid, dim3(256), 0, s, vol, nx, ny, nz, stride_x, stride_y, dim == 0, words_ok, mm,
                           ab, out);
    return hipExtGetLastError();
}


// ------------------------------------------------ the run's pictures ---
// accumulateEvents (utils.cpp:184-216) and the two images of saveDepthMaps (utils.cpp:55-58, 82-93).
namespace {

// monotone int -> uint, so that a zeroed word is the identity of atomicMax for the maximum (key) and the minimum (~key)
__device__ __forceinline__ uint32_t int_key(int c) { return (uint32_t)c ^ 0x80000000u; }
__device__ __forceinline__ int key_int(uint32_t k) { return (int)(k ^ 0x80000000u); }

__device__ __forceinline__ void event_vote(int* __restrict__ count, uint32_t ex, uint32_t ey, int d, int width, int height,
                                           uint32_t& dropped)
{
    if (ex < (uint32_t)width && ey < (uint32_t)height)
        (void)__hip_atomic_fetch_add(count + (size_t)ey * width + ex, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        ++dropped;
}

// Per-pixel event counts: a thread takes 8 consecutive events per step -- one 16-byte load of x, one of y, one 8-byte load
// of the polarity bytes -- and adds +-1 (POL) or +1 to count[y][x] with atomics whose result nobody reads.  x, y 16-byte
// aligned, pol 8-byte aligned.  scratch[2] += events outside the sensor.
template <bool POL>
__global__ __launch_bounds__(256) void k_event_image_count(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y,
                                                           const uint8_t* __restrict__ pol, size_t n, int width, int height,
                                                           int* __restrict__ count, uint32_t* __restrict__ scratch)
{
    uint32_t dropped = 0;
    const size_t n8 = n / 8;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const uint4 vx = reinterpret_cast<const uint4*>(x)[i];
        const uint4 vy = reinterpret_cast<const uint4*>(y)[i];
        uint2 vp = make_uint2(0u, 0u);
        if (POL) vp = reinterpret_cast<const uint2*>(pol)[i];
        const uint32_t wx[4] = {vx.x, vx.y, vx.z, vx.w}, wy[4] = {vy.x, vy.y, vy.z, vy.w}, wp[2] = {vp.x, vp.y};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t ex = (wx[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            const uint32_t ey = (wy[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            const int d = POL ? (((wp[k >> 2] >> (8 * (k & 3))) & 0xffu) ? 1 : -1) : 1;
            event_vote(count, ex, ey, d, width, height, dropped);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        const size_t i = n8 * 8 + threadIdx.x;
        event_vote(count, x[i], y[i], POL ? (pol[i] ? 1 : -1) : 1, width, height, dropped);
    }
    for (int off = 32; off > 0; off >>= 1) dropped += __shfl_down(dropped, off, 64);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&scratch[2], dropped);
}

// what the image is made of: the signed count (POL), or the count modulo 256 (the reference's uchar += 1 wraps)
template <bool POL>
__device__ __forceinline__ int event_value(int c) { return POL ? c : (c & 255); }

// scratch[0] = max of ~key (the minimum), scratch[1] = max of key (the maximum); both zero before
template <bool POL>
__global__ __launch_bounds__(256) void k_event_image_minmax(const int* __restrict__ count, int npix, uint32_t* __restrict__ scratch)
{
    uint32_t lo = 0u, hi = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t k = int_key(event_value<POL>(count[i]));
        lo = max(lo, ~k);
        hi = max(hi, k);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = max(lo, (uint32_t)__shfl_down((int)lo, off, 64));
        hi = max(hi, (uint32_t)__shfl_down((int)hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&scratch[0], lo);
        atomicMax(&scratch[1], hi);
    }
}

// POL: c * (float)(128 / half) + 128, half = max(|min|, |max|) in double, 128 everywhere when half == 0 (utils.cpp:196-206).
// Otherwise cv::normalize(NORM_MINMAX, 0, 255) of the wrapped counts with k_conf8's scale / shift.  Four pixels per thread,
// one word per store (out is 4-byte aligned); the last npix % 4 pixels as bytes.
template <bool POL>
__global__ __launch_bounds__(256) void k_event_image_u8(const int* __restrict__ count, int npix, const uint32_t* __restrict__ scratch,
                                                        uint8_t* __restrict__ out)
{
    const int i4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= npix) return;
    const double smin = (double)key_int(~scratch[0]), smax = (double)key_int(scratch[1]);
    float a, b;
    bool flat = false;
    if (POL) {
        const double half = fmax(fabs(smin), fabs(smax));
        flat = !(half > 0.0);
        a = flat ? 0.f : (float)(128.0 / half);
        b = 128.f;
    } else {
        const double range = smax - smin;
        const double scale = 255.0 * (range > 2.220446049250313e-16 ? 1. / range : 0.);
        a = (float)scale;
        b = (float)(0.0 - smin * scale);
    }
    uint32_t pk = 0;
    const int m = npix - i4 < 4 ? npix - i4 : 4;
    for (int k = 0; k < m; ++k) {
        const float v = (float)event_value<POL>(count[i4 + k]) * a + b;
        pk |= (uint32_t)(flat ? (uint8_t)128 : saturate_u8(v)) << (8 * k);
    }
    if (m == 4) {
        reinterpret_cast<uint32_t*>(out)[i4 >> 2] = pk;
    } else {
        for (int k = 0; k < m; ++k) out[i4 + k] = (uint8_t)(pk >> (8 * k));
    }
}

// extremes of the confidence map as float keys: mm[0] = max of ~key (the minimum), mm[1] = max of key; both zero before
__global__ __launch_bounds__(256) void k_image_conf_minmax(const float* __restrict__ conf, int n, uint32_t* __restrict__ mm)
{
    uint32_t lo = 0u, hi = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t k = float_key(conf[i]);
        lo = max(lo, ~k);
        hi = max(hi, k);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = max(lo, (uint32_t)__shfl_down((int)lo, off, 64));
        hi = max(hi, (uint32_t)__shfl_down((int)hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

// utils.cpp:55-58: 255 - normalize(conf, 0, 255, NORM_MINMAX) written as 8 bit (k_conf8's scale / shift, no reset of (0,0))
__global__ __launch_bounds__(256) void k_conf_negated_u8(const float* __restrict__ conf, int n, const uint32_t* __restrict__ mm,
                                                         uint8_t* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double smin = (double)key_float(~mm[0]), smax = (double)key_float(mm[1]);
    const double range = smax - smin;
    const double scale = 255.0 * (range > 2.220446049250313e-16 ? 1. / range : 0.);
    const double shift = 0.0 - smin * scale;
    const float a = (float)scale, b = (float)shift;
    const float nrm = conf[i] * a + b;
    out[i] = saturate_u8(255.f - nrm);
}

// colour of one pixel before the dilation (utils.cpp:83-89): lut[saturate_u8((1 / depth) * a + b)] where mask > 0, else black
__device__ __forceinline__ uint32_t inv_depth_bgr(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                  const uint8_t* __restrict__ lut, int p, float a, float b)
{
    if (!mask[p]) return 0u;
    const float inv = 1.0f / depth[p];
    const float v = inv * a + b;
    const int i = (v == v) ? (int)saturate_u8(v) : 0;
    return (uint32_t)lut[3 * i] | ((uint32_t)lut[3 * i + 1] << 8) | ((uint32_t)lut[3 * i + 2] << 16);
}

__device__ __forceinline__ uint32_t max_bgr(uint32_t p, uint32_t q)
{
    return max(p & 0xffu, q & 0xffu) | max(p & 0xff00u, q & 0xff00u) | max(p & 0xff0000u, q & 0xff0000u);
}

// utils.cpp:82-93: the coloured inverse-depth image dilated by the 3 x 3 cross, per channel; neighbours outside the image do
// not contribute.  One thread per pixel; it recomputes its four neighbours' colours.
__global__ __launch_bounds__(256) void k_inv_depth_colored_dilated(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                   const uint8_t* __restrict__ lut, int rows, int cols, float a,
                                                                   float b, uint8_t* __restrict__ out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= rows * cols) return;
    const int r = p / cols, c = p - r * cols;
    uint32_t v = inv_depth_bgr(depth, mask, lut, p, a, b);
    if (r > 0) v = max_bgr(v, inv_depth_bgr(depth, mask, lut, p - cols, a, b));
    if (r + 1 < rows) v = max_bgr(v, inv_depth_bgr(depth, mask, lut, p + cols, a, b));
    if (c > 0) v = max_bgr(v, inv_depth_bgr(depth, mask, lut, p - 1, a, b));
    if (c + 1 < cols) v = max_bgr(v, inv_depth_bgr(depth, mask, lut, p + 1, a, b));
    out[3 * (size_t)p] = (uint8_t)v;
    out[3 * (size_t)p + 1] = (uint8_t)(v >> 8);
    out[3 * (size_t)p + 2] = (uint8_t)(v >> 16);
}

}  // namespace

size_t event_image_scratch_words(int width, int height) { return kEventImageHeadWords + (size_t)width * height; }

hipError_t launch_event_image(hipStream_t s, const uint16_t* x, const uint16_t* y, const uint8_t* pol, size_t n, int width,
                              int height, int use_polarity, uint32_t* scratch, uint8_t* out)
{
    const size_t npix_z = (size_t)width * height;
    if (width < 1 || height < 1 || npix_z > 0x7fffffffull || (use_polarity && n && !pol)) return hipErrorInvalidValue;
    const int npix = (int)npix_z;
    int* count = reinterpret_cast<int*>(scratch + kEventImageHeadWords);
    hipError_t e = hipMemsetAsync(scratch, 0, event_image_scratch_words(width, height) * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (n) {
        const dim3 grid(grid_for(n / 8 + 1, 256, 4096)), block(256);
        if (use_polarity)
            hipLaunchKernelGGL(k_event_image_count<true>, grid, block, 0, s, x, y, pol, n, width, height, count, scratch);
        else
            hipLaunchKernelGGL(k_event_image_count<false>, grid, block, 0, s, x, y, pol, n, width, height, count, scratch);
        if ((e = hipExtGetLastError()) != hipSuccess) return e;
    }
    const dim3 rgrid(grid_for(npix_z, 256, 256)), ugrid((unsigned)((npix_z + 1023) / 1024)), block(256);
    if (use_polarity) {
        hipLaunchKernelGGL(k_event_image_minmax<true>, rgrid, block, 0, s, count, npix, scratch);
        hipLaunchKernelGGL(k_event_image_u8<true>, ugrid, block, 0, s, count, npix, scratch, out);
    } else {
        hipLaunchKernelGGL(k_event_image_minmax<false>, rgrid, block, 0, s, count, npix, scratch);
        hipLaunchKernelGGL(k_event_image_u8<false>, ugrid, block, 0, s, count, npix, scratch, out);
    }
    return hipExtGetLastError();
}

void default_jet_lut(uint8_t* lut_bgr)
{
    for (int i = 0; i < 256; ++i) {
        const double t = (double)i / 255.0;
        const double ch[3] = {1.5 - std::fabs(4.0 * t - 1.0), 1.5 - std::fabs(4.0 * t - 2.0), 1.5 - std::fabs(4.0 * t - 3.0)};  // b, g, r
        for (int k = 0; k < 3; ++k) {
            const double c = ch[k] < 0.0 ? 0.0 : (ch[k] > 1.0 ? 1.0 : ch[k]);
            lut_bgr[3 * i + k] = (uint8_t)std::nearbyint(c * 255.0);  // half to even (the default rounding mode)
        }
    }
}

hipError_t launch_depth_images(hipStream_t s, const float* depth, const float* conf, const uint8_t* mask, int rows, int cols,
                               float min_depth, float max_depth, const uint8_t* lut_dev, uint32_t* mm, uint8_t* conf_negated,
                               uint8_t* inv_depth_bgr)
{
    const size_t npix_z = (size_t)rows * cols;
    if (rows < 1 || cols < 1 || npix_z > 0x7fffffffull / 3) return hipErrorInvalidValue;
    const int npix = (int)npix_z;
    const dim3 pgrid((unsigned)((npix_z + 255) / 256)), block(256);
    hipError_t e;
    if (conf_negated) {
        if ((e = hipMemsetAsync(mm, 0, 2 * sizeof(uint32_t), s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_image_conf_minmax, dim3(grid_for(npix_z, 256, 256)), block, 0, s, conf, npix, mm);
        hipLaunchKernelGGL(k_conf_negated_u8, pgrid, block, 0, s, conf, npix, mm, conf_negated);
        if ((e = hipExtGetLastError()) != hipSuccess) return e;
    }
    if (inv_depth_bgr) {
        // utils.cpp:85: (invmap - 1./max_depth) / (1./min_depth - 1./max_depth) * 255. -- the scalars of the matrix expression
        // fold into one scale and one shift in double, applied to the float image in float
        const double s1 = 1.0 / (double)max_depth;
        const double s2 = 1.0 / (double)min_depth - s1;
        const double k = 1.0 / s2;
        const double alpha = k * 255.0, beta = ((-s1) * k) * 255.0;
        hipLaunchKernelGGL(k_inv_depth_colored_dilated, pgrid, block, 0, s, depth, mask, lut_dev, rows, cols, (float)alpha,
                           (float)beta, inv_depth_bgr);
        if ((e = hipExtGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}


// ------------------------------------------------ depth-map scores against ground truth ---
// The metrics of depth_metrics.py:4-37 and the error histogram of precision_completeness.py:43-92 over every window added.
namespace {

constexpr int kScoreBlock = 256;  // four waves of 64

__device__ __forceinline__ double score_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum, always of the same tree
}

__device__ __forceinline__ unsigned long long score_wave_max(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One pass over a map of n pixels.  Every count is a wave-uniform population count of a ballot, summed per block in LDS and
// added to st with one integer atomic per counter and block.  The four float64 sums go lane -> wave (shuffles) -> block (LDS,
// waves in order) into partials[blockIdx.x * 4 + k]: no floating-point atomic, so the same map gives the same bits.  A joint
// pixel's err = |g - d| is appended at st->cursor, which each wave advances once per step by its number of joint pixels;
// positions >= capacity are not written and raise st->overflow.  The loop is uniform per wave (all 64 lanes take every step).
__global__ __launch_bounds__(kScoreBlock) void k_score_accumulate(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                  const float* __restrict__ gt, size_t n, double gt_min, double b,
                                                                  double f, ScoreState* __restrict__ st, double* __restrict__ buf,
                                                                  unsigned long long capacity, double* __restrict__ partials)
{
    __shared__ double sh_sum[kScoreBlock / 64][4];
    __shared__ unsigned long long sh_cnt[kScoreBlock / 64][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s_di = 0.0, s_di2 = 0.0, s_are = 0.0, s_abs = 0.0;
    unsigned long long c_est = 0, c_gt = 0, c_joint = 0, c_d1 = 0, c_d2 = 0, c_d3 = 0, c_bad = 0, maxkey = 0;
    bool over = false;
    const size_t stride = (size_t)gridDim.x * kScoreBlock;
    for (size_t base = (size_t)blockIdx.x * kScoreBlock; base < n; base += stride) {
        const size_t i = base + threadIdx.x;
        bool est = false, gtv = false;
        double d = 1.0, g = 1.0;
        if (i < n) {
            const float df = depth[i], gf = gt[i];
            d = (double)df;
            g = (double)gf;
            est = mask[i] != 0 && isfinite(df) && df > 0.f;
            gtv = isfinite(gf) && g >= gt_min;
        }
        const bool joint = est && gtv;
        if (gtv) {
            const unsigned long long k = (unsigned long long)__double_as_longlong(g);  // g > 0: the bits order as the values
            maxkey = k > maxkey ? k : maxkey;
        }
        bool d1 = false, d2 = false, d3 = false, bad = false;
        double err = 0.0;
        if (joint) {
            const double ratio = fmax(d / g, g / d);                 // depth_metrics.py:9
            d1 = ratio < 1.25;
            d2 = ratio < 1.5625;
            d3 = ratio < 1.953125;
            const double di = log(g) - log(d);                       // :15
            s_di += di;
            s_di2 += di * di;
            s_are += fabs(d - g) / d;                                // :20
            err = fabs(g - d);
            s_abs += err;
            const double e = fabs(1.0 / d - 1.0 / g) * b * f;        // :26
            const double r = e * g / b / f;                          // :27
            bad = e > 5.0 && r > 0.05;                               // :28
        }
        const unsigned long long jb = __ballot(joint);
        c_est += __popcll(__ballot(est));
        c_gt += __popcll(__ballot(gtv));
        c_joint += __popcll(jb);
        c_d1 += __popcll(__ballot(d1));
        c_d2 += __popcll(__ballot(d2));
        c_d3 += __popcll(__ballot(d3));
        c_bad += __popcll(__ballot(bad));
        if (jb) {
            const unsigned long long cnt = (unsigned long long)__popcll(jb);
            unsigned long long start = 0;
            if (lane == 0) start = atomicAdd(&st->cursor, cnt);
            start = __shfl(start, 0, 64);
            if (start + cnt > capacity) over = true;
            const unsigned long long pos = start + (unsigned long long)__popcll(jb & ((1ull << lane) - 1ull));
            if (joint && pos < capacity) buf[pos] = err;
        }
    }
    s_di = score_wave_sum(s_di);
    s_di2 = score_wave_sum(s_di2);
    s_are = score_wave_sum(s_are);
    s_abs = score_wave_sum(s_abs);
    maxkey = score_wave_max(maxkey);
    if (lane == 0) {
        sh_sum[wave][0] = s_di;
        sh_sum[wave][1] = s_di2;
        sh_sum[wave][2] = s_are;
        sh_sum[wave][3] = s_abs;
        sh_cnt[wave][0] = c_est;
        sh_cnt[wave][1] = c_gt;
        sh_cnt[wave][2] = c_joint;
        sh_cnt[wave][3] = c_d1;
        sh_cnt[wave][4] = c_d2;
        sh_cnt[wave][5] = c_d3;
        sh_cnt[wave][6] = c_bad;
        sh_cnt[wave][7] = maxkey;
        if (over) atomicOr(&st->overflow, 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double p = sh_sum[0][threadIdx.x];
        for (int w = 1; w < kScoreBlock / 64; ++w) p += sh_sum[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 4 + threadIdx.x] = p;
    } else if (threadIdx.x >= 64 && threadIdx.x < 72) {
        const int k = threadIdx.x - 64;
        unsigned long long* dst = k < 7 ? &st->count[k] : &st->max_gt_key;
        if (k < 7) {
            unsigned long long c = 0;
            for (int w = 0; w < kScoreBlock / 64; ++w) c += sh_cnt[w][k];
            if (c) atomicAdd(dst, c);
        } else {
            unsigned long long c = 0;
            for (int w = 0; w < kScoreBlock / 64; ++w) c = sh_cnt[w][7] > c ? sh_cnt[w][7] : c;
            if (c) atomicMax(dst, c);
        }
    }
}

// st->sum[k] += the block partials of one k_score_accumulate, folded in an order that depends on nblocks alone: wave k takes
// sum k, lane l adds partials l, l + 64, ... in turn, then the shuffle tree.  One block of four waves.
__global__ __launch_bounds__(kScoreBlock) void k_score_finish(const double* __restrict__ partials, int nblocks, ScoreState* __restrict__ st)
{
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    double acc = 0.0;
    for (int j = lane; j < nblocks; j += 64) acc += partials[(size_t)j * 4 + k];
    acc = score_wave_sum(acc);
    if (lane == 0) st->sum[k] = st->sum[k] + acc;
}

// extremes of the n stored errors as bit patterns (non-negative doubles order as integers): mm[0] = min (all ones before),
// mm[1] = max (zero before)
__global__ __launch_bounds__(kScoreBlock) void k_score_minmax(const double* __restrict__ buf, size_t n, unsigned long long* __restrict__ mm)
{
    unsigned long long lo = ~0ull, hi = 0ull;
    const size_t stride = (size_t)gridDim.x * kScoreBlock;
    for (size_t i = (size_t)blockIdx.x * kScoreBlock + threadIdx.x; i < n; i += stride) {
        const unsigned long long k = (unsigned long long)__double_as_longlong(buf[i]);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    hi = score_wave_max(hi);
    lo = ~score_wave_max(~lo);
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

// numpy's linspace(first, last, nb + 1)[i]: arange * step + first, the last edge set to `last`; a step that underflows to
// zero takes the (i / nb) * delta form
__device__ __forceinline__ double score_edge(const ScoreBins& B, long long i)
{
    if (i == B.nb) return B.last;
    return B.step_zero ? ((double)i / (double)B.nb) * B.delta + B.first : (double)i * B.step + B.first;
}

// np.histogram's uniform-bin index of x in [first, last] (numpy/lib/_histograms_impl.py, the fast path): truncate
// ((x - first) / delta) * nb, fold nb into nb - 1, then correct by one against the edges; the last bin is closed on the right
__device__ __forceinline__ long long score_bin(const ScoreBins& B, double x)
{
    long long idx = (long long)(((x - B.first) / B.delta) * (double)B.nb);
    if (idx == B.nb) --idx;
    idx = idx < 0 ? 0 : (idx > B.nb - 1 ? B.nb - 1 : idx);  // (no effect on values inside the range; keeps every access in bounds)
    if (x < score_edge(B, idx) && idx > 0) --idx;
    if (x >= score_edge(B, idx + 1) && idx != B.nb - 1) ++idx;
    return idx;
}

constexpr int kScoreLdsBins = 8192;  // 32 KiB of 32-bit LDS counters

// counts[bin] += the number of stored errors per bin.  LDSBINS (nb <= kScoreLdsBins): 32-bit LDS atomics, then one 64-bit
// global atomic per non-empty bin and block; otherwise 64-bit global atomics.
template <bool LDSBINS>
__global__ __launch_bounds__(kScoreBlock) void k_score_histogram(const double* __restrict__ buf, size_t n, ScoreBins B,
                                                                 unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t bins[LDSBINS ? kScoreLdsBins : 1];
    const int nb = (int)B.nb;
    if (LDSBINS) {
        for (int k = threadIdx.x; k < nb; k += kScoreBlock) bins[k] = 0u;
        __syncthreads();
    }
    const size_t stride = (size_t)gridDim.x * kScoreBlock;
    for (size_t i = (size_t)blockIdx.x * kScoreBlock + threadIdx.x; i < n; i += stride) {
        const long long idx = score_bin(B, buf[i]);
        if (LDSBINS)
            atomicAdd(&bins[idx], 1u);
        else
            atomicAdd(&counts[idx], 1ull);
    }
    if (LDSBINS) {
        __syncthreads();
        for (int k = threadIdx.x; k < nb; k += kScoreBlock)
            if (bins[k]) atomicAdd(&counts[k], (unsigned long long)bins[k]);
    }
}

// Radix select on the bit patterns, most significant byte first (pass 0 .. 7), of two ranks at once.  sel[0..1]: the bytes
// chosen so far for each rank (zero before pass 0), hist: [8][2][256] counters, zero before pass 0.  This pass counts, per
// rank, the next byte of the errors whose higher bytes equal that rank's.
__global__ __launch_bounds__(kScoreBlock) void k_score_select(const double* __restrict__ buf, size_t n, const unsigned long long* __restrict__ sel,
                                                              int pass, unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t h[2][256];
    h[0][threadIdx.x] = 0u;
    h[1][threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    // the bytes above `shift`: (key >> shift) >> 8 keeps the shift count below 64 in pass 0
    const unsigned long long p0 = (sel[0] >> shift) >> 8, p1 = (sel[1] >> shift) >> 8;
    const size_t stride = (size_t)gridDim.x * kScoreBlock;
    for (size_t i = (size_t)blockIdx.x * kScoreBlock + threadIdx.x; i < n; i += stride) {
        const unsigned long long k = (unsigned long long)__double_as_longlong(buf[i]) >> shift;
        const unsigned long long hi = k >> 8;
        const uint32_t dg = (uint32_t)(k & 255ull);
        if (hi == p0) atomicAdd(&h[0][dg], 1u);
        if (hi == p1) atomicAdd(&h[1][dg], 1u);
    }
    __syncthreads();
    unsigned long long* out = hist + (size_t)pass * 512;
    if (h[0][threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)h[0][threadIdx.x]);
    if (h[1][threadIdx.x]) atomicAdd(&out[256 + threadIdx.x], (unsigned long long)h[1][threadIdx.x]);
}

// After pass `pass`: for each rank, the byte whose bucket holds it (exclusive prefix <= rank < inclusive prefix) joins
// sel[j], and sel[2 + j] becomes the rank inside that bucket.  Pass 0 takes the ranks from rank0 / rank1.  One block.
__global__ __launch_bounds__(kScoreBlock) void k_score_select_pick(unsigned long long* __restrict__ sel, int pass,
                                                                   const unsigned long long* __restrict__ hist, unsigned long long rank0,
                                                                   unsigned long long rank1)
{
    __shared__ unsigned long long scan[2][256];
    const int t = threadIdx.x, shift = 56 - 8 * pass;
    for (int j = 0; j < 2; ++j) {
        const unsigned long long c = hist[(size_t)pass * 512 + j * 256 + t];
        const unsigned long long r = pass == 0 ? (j ? rank1 : rank0) : sel[2 + j];
        int cur = 0;
        scan[0][t] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {  // Hillis-Steele inclusive scan, ping-pong
            const unsigned long long v = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0ull);
            scan[cur ^ 1][t] = v;
            cur ^= 1;
            __syncthreads();
        }
        const unsigned long long incl = scan[cur][t], excl = incl - c;
        __syncthreads();  // everyone has read sel[2 + j] and the scan before the one owner writes
        if (excl <= r && r < incl) {
            sel[j] |= (unsigned long long)t << shift;
            sel[2 + j] = r - excl;
        }
        __syncthreads();
    }
}

}  // namespace

static int score_blocks(size_t n)
{
    const size_t b = (n + kScoreBlock - 1) / kScoreBlock;
    return (int)(b < 1 ? 1 : (b > (size_t)kScoreMaxBlocks ? (size_t)kScoreMaxBlocks : b));
}

hipError_t launch_score_accumulate(hipStream_t s, const float* depth, const uint8_t* mask, const float* gt, size_t n, double gt_min,
                                   double baseline, double focal, ScoreState* st, double* buf, size_t capacity, double* partials)
{
    if (!depth || !mask || !gt || !st || !buf || !partials || n == 0) return hipErrorInvalidValue;
    const int blocks = score_blocks(n);  // a function of n alone: the order of every sum is
    hipLaunchKernelGGL(k_score_accumulate, dim3(blocks), dim3(kScoreBlock), 0, s, depth, mask, gt, n, gt_min, baseline, focal, st, buf,
                       (unsigned long long)capacity, partials);
    hipLaunchKernelGGL(k_score_finish, dim3(1), dim3(kScoreBlock), 0, s, partials, blocks, st);
    return hipExtGetLastError();
}

hipError_t launch_score_minmax(hipStream_t s, const double* buf, size_t n, unsigned long long* mm)
{
    hipError_t e = hipMemsetAsync(mm, 0xff, sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(mm + 1, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(k_score_minmax, dim3(score_blocks(n)), dim3(kScoreBlock), 0, s, buf, n, mm);
    return hipExtGetLastError();
}

hipError_t launch_score_histogram(hipStream_t s, const double* buf, size_t n, const ScoreBins& bins, unsigned long long* counts)
{
    if (bins.nb < 1 || bins.nb > kScoreMaxBins || !(bins.delta > 0.0)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)bins.nb * sizeof(unsigned long long), s);
    if (e != hipSuccess || n == 0) return e;
    if (bins.nb <= kScoreLdsBins)
        hipLaunchKernelGGL(k_score_histogram<true>, dim3(score_blocks(n)), dim3(kScoreBlock), 0, s, buf, n, bins, counts);
    else
        hipLaunchKernelGGL(k_score_histogram<false>, dim3(score_blocks(n)), dim3(kScoreBlock), 0, s, buf, n, bins, counts);
    return hipExtGetLastError();
}

hipError_t launch_score_select(hipStream_t s, const double* buf, size_t n, size_t rank0, size_t rank1, unsigned long long* work)
{
    if (n == 0 || rank0 >= n || rank1 >= n) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(work, 0, kScoreSelectWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(k_score_select, dim3(score_blocks(n)), dim3(kScoreBlock), 0, s, buf, n, work, pass, work + 4);
        hipLaunchKernelGGL(k_score_select_pick, dim3(1), dim3(kScoreBlock), 0, s, work, pass, work + 4, (unsigned long long)rank0,
                           (unsigned long long)rank1);
    }
    return hipExtGetLastError();
}


// ------------------------------- ground-truth depth from disparity images ---
// scripts/evaluate_mcemvs_dsec.py:108-122: reproject with Q, transform with T, project with K, forward-splat with numpy's
// scatter rules (the largest row-major source index wins a target pixel).
namespace {

constexpr int kGtBlock = 256;  // four waves of 64

struct GtPoint {
    bool kept;      // Z < +inf as float32
    bool write;     // has a target pixel in this mode
    bool outside;   // kept and not indexable (numpy's IndexError)
    uint32_t target;
    float value;    // float32(P_2)
};

__device__ __forceinline__ float gt_disparity(float d) { return d; }
// matplotlib's 16-bit rule, then the script's * 256: two fp32 operations, the divide correctly rounded
__device__ __forceinline__ float gt_disparity(uint16_t raw) { return __fdiv_rn((float)raw, 65535.0f) * 256.0f; }

// steps 1-4 of DESIGN.md 7g for source pixel (x, y): float64 throughout, sums left to right, no contraction
__device__ __forceinline__ GtPoint gt_point(const GtCalib& c, int x, int y, float disp, int W, int H, int mode)
{
    GtPoint r{false, false, false, 0u, 0.0f};
    const double xd = (double)x, yd = (double)y, d = (double)disp;
    double h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = ((c.Q[4 * i] * xd + c.Q[4 * i + 1] * yd) + c.Q[4 * i + 2] * d) + c.Q[4 * i + 3];
    const float Xf = (float)(h[0] / h[3]), Yf = (float)(h[1] / h[3]), Zf = (float)(h[2] / h[3]);
    r.kept = Zf < __builtin_inff();  // NaN and +inf are dropped; -inf and negative values stay
    if (!r.kept) return r;
    const double X = (double)Xf, Y = (double)Yf, Z = (double)Zf;
    double P[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) P[i] = ((c.T[4 * i] * X + c.T[4 * i + 1] * Y) + c.T[4 * i + 2] * Z) + c.T[4 * i + 3];
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = ((c.K[4 * i] * P[0] + c.K[4 * i + 1] * P[1]) + c.K[4 * i + 2] * P[2]) + c.K[4 * i + 3] * P[3];
    const double tu = trunc(p[0] / p[2]), tv = trunc(p[1] / p[2]);  // NaN / inf stay NaN / inf and fail the range test
    r.value = (float)P[2];
    const double Wd = (double)W, Hd = (double)H;
    if (!(tu >= -Wd && tu < Wd && tv >= -Hd && tv < Hd)) {
        r.outside = true;
        return r;
    }
    long long iu = (long long)tu, iv = (long long)tv;
    if (iu < 0 || iv < 0) {
        if (mode == GT_DROP_OUTSIDE) return r;  // no wrap: dropped on its own
        iu += iu < 0 ? W : 0;                  // numpy's negative indices
        iv += iv < 0 ? H : 0;
    }
    r.write = true;
    r.target = (uint32_t)((unsigned long long)iv * (unsigned long long)W + (unsigned long long)iu);
    return r;
}

// One thread per source pixel: winner[target] = max(source index + 1), counters[0] += kept points, counters[1] += outside
// points (a ballot's population count, one integer atomic per wave and counter; every lane of a wave reaches the ballots).
template <typename In>
__global__ __launch_bounds__(kGtBlock) void k_gt_project(const In* __restrict__ disp, GtCalib c, int W, int H, int mode,
                                                         uint32_t* __restrict__ winner, unsigned int* __restrict__ counters)
{
    const unsigned long long n = (unsigned long long)W * (unsigned long long)H;
    const unsigned long long i = (unsigned long long)blockIdx.x * kGtBlock + threadIdx.x;
    GtPoint r{false, false, false, 0u, 0.0f};
    if (i < n) {
        const int y = (int)(i / (unsigned long long)W), x = (int)(i - (unsigned long long)y * (unsigned long long)W);
        r = gt_point(c, x, y, gt_disparity(disp[i]), W, H, mode);
        if (r.write) atomicMax(&winner[r.target], (uint32_t)i + 1u);
    }
    const unsigned int c_kept = (unsigned int)__popcll(__ballot(r.kept));
    const unsigned int c_out = (unsigned int)__popcll(__ballot(r.outside));
    if ((threadIdx.x & 63) == 0) {
        if (c_kept) atomicAdd(&counters[0], c_kept);
        if (c_out) atomicAdd(&counters[1], c_out);
    }
}

// One thread per source pixel: it computes its point again, and the winner of a target pixel writes float32(P_2) there.
// In script mode one outside point leaves the whole (cleared) output as it is.
template <typename In>
__global__ __launch_bounds__(kGtBlock) void k_gt_write(const In* __restrict__ disp, GtCalib c, int W, int H, int mode,
                                                       const uint32_t* __restrict__ winner, const unsigned int* __restrict__ counters,
                                                       float* __restrict__ out)
{
    if (mode == GT_AS_SCRIPT && counters[1] != 0u) return;
    const unsigned long long n = (unsigned long long)W * (unsigned long long)H;
    const unsigned long long i = (unsigned long long)blockIdx.x * kGtBlock + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / (unsigned long long)W), x = (int)(i - (unsigned long long)y * (unsigned long long)W);
    const GtPoint r = gt_point(c, x, y, gt_disparity(disp[i]), W, H, mode);
    if (r.write && winner[r.target] == (uint32_t)i + 1u) out[r.target] = r.value;
}

// evaluate_mcemvs_dsec.py:75-79 (thicken_edges): erosion of the map with the 3 x 3 cross, pixels without an estimate
// standing at no_estimate; neighbours outside the image do not contribute
__global__ __launch_bounds__(kGtBlock) void k_depth_erode_cross(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                int rows, int cols, float no_estimate, float* __restrict__ out_depth,
                                                                uint8_t* __restrict__ out_mask)
{
    const size_t p = (size_t)blockIdx.x * kGtBlock + threadIdx.x;
    if (p >= (size_t)rows * cols) return;
    const int r = (int)(p / (size_t)cols), c = (int)(p - (size_t)r * cols);
    auto at = [&](size_t q) { return mask[q] ? depth[q] : no_estimate; };
    float e = at(p);
    if (r > 0) e = fminf(e, at(p - cols));
    if (r + 1 < rows) e = fminf(e, at(p + cols));
    if (c > 0) e = fminf(e, at(p - 1));
    if (c + 1 < cols) e = fminf(e, at(p + 1));
    out_depth[p] = e;
    out_mask[p] = e != no_estimate ? 1 : 0;
}

template <typename In>
hipError_t gt_project_any(hipStream_t s, const In* disp, const GtCalib& calib, int W, int H, int mode, const GtWork& w)
{
    const size_t n = (size_t)W * H;
    if (!disp || !w.winner || !w.counters || !w.out || W < 1 || H < 1 || n >= 0xffffffffull) return hipErrorInvalidValue;
    if (mode != GT_AS_SCRIPT && mode != GT_DROP_OUTSIDE) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(w.winner, 0, n * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.counters, 0, 2 * sizeof(unsigned int), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.out, 0, n * sizeof(float), s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((n + kGtBlock - 1) / kGtBlock)), block(kGtBlock);  // n < 2^32: at most 2^24 blocks
    hipLaunchKernelGGL(k_gt_project<In>, grid, block, 0, s, disp, calib, W, H, mode, w.winner, w.counters);
    hipLaunchKernelGGL(k_gt_write<In>, grid, block, 0, s, disp, calib, W, H, mode, w.winner, w.counters, w.out);
    return hipExtGetLastError();
}

}  // namespace

hipError_t launch_gt_project(hipStream_t s, const float* disp, const GtCalib& calib, int width, int height, int mode, const GtWork& w)
{
    return gt_project_any(s, disp, calib, width, height, mode, w);
}

hipError_t launch_gt_project_u16(hipStream_t s, const uint16_t* raw, const GtCalib& calib, int width, int height, int mode,
                                 const GtWork& w)
{
    return gt_project_any(s, raw, calib, width, height, mode, w);
}

hipError_t launch_depth_erode_cross(hipStream_t s, const float* depth, const uint8_t* mask, int rows, int cols, float no_estimate,
                                    float* out_depth, uint8_t* out_mask)
{
    const size_t npix = (size_t)rows * cols;
    if (!depth || !mask || !out_depth || !out_mask || rows < 1 || cols < 1 || npix > ((size_t)1 << 29)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_erode_cross, dim3((unsigned)((npix + kGtBlock - 1) / kGtBlock)), dim3(kGtBlock), 0, s, depth, mask, rows,
                       cols, no_estimate, out_depth, out_mask);
    return hipExtGetLastError();
}

}  // namespace dsi

// ---- lens rectification table: MapperEMVS::precomputeRectifiedPoints (mapper_emvs_stereo.cpp:256-299) ----
namespace dsi {
namespace {

constexpr int kLensBlock = 256;

// the plumb_bob inverse as cv::undistortPoints iterates it (5 rounds, no epsilon exit), then RR = P[:, :3] R applied.
// float64 throughout, every product and sum left to right, no contraction.
__device__ __forceinline__ void lens_plumb_bob(const LensCoef& c, double x, double y, double* u, double* v)
{
    const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5], k5 = c.k[6], k6 = c.k[7];
    const double ifx = 1.0 / c.fx, ify = 1.0 / c.fy;
    const double x0 = (x - c.cx) * ifx, y0 = (y - c.cy) * ify;
    double X = x0, Y = y0;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        const double r2 = X * X + Y * Y;
        const double icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0.0) {
            X = x0;
            Y = y0;
            break;
        }
        const double dX = 2.0 * p1 * X * Y + p2 * (r2 + 2.0 * X * X);
        const double dY = p1 * (r2 + 2.0 * Y * Y) + 2.0 * p2 * X * Y;
        X = (x0 - dX) * icdist;
        Y = (y0 - dY) * icdist;
    }
    const double xx = c.RR[0] * X + c.RR[1] * Y + c.RR[2], yy = c.RR[3] * X + c.RR[4] * Y + c.RR[5];
    const double ww = 1.0 / (c.RR[6] * X + c.RR[7] * Y + c.RR[8]);
    *u = xx * ww;
    *v = yy * ww;
}

// the Kannala-Brandt inverse as cv::fisheye::undistortPoints iterates it (Newton, at most 10 rounds, |fix| < 1e-8); a pixel
// that does not converge, or whose angle changes sign, gets OpenCV's -1000000.  sqrt is the correctly rounded one
// (k_pc_backproject's); tan is the device library's, the only operation here that is not correctly rounded.
__device__ __forceinline__ void lens_fisheye(const LensCoef& c, double x, double y, double* u, double* v)
{
    const double k1 = c.k[0], k2 = c.k[1], k3 = c.k[2], k4 = c.k[3];
    const double px = (x - c.cx) / c.fx, py = (y - c.cy) / c.fy;
    const double half_pi = 1.57079632679489661923;
    double theta_d = sqrt(px * px + py * py);
    theta_d = fmin(fmax(-half_pi, theta_d), half_pi);
    double theta = theta_d, scale = 0.0;
    bool converged = false;
    if (fabs(theta_d) > 1e-8) {
#pragma unroll 1
        for (int j = 0; j < 10; ++j) {
            const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double a = k1 * t2, b = k2 * t4, cc = k3 * t6, d = k4 * t8;
            const double fix = (theta * (1.0 + a + b + cc + d) - theta_d) / (1.0 + 3.0 * a + 5.0 * b + 7.0 * cc + 9.0 * d);
            theta = theta - fix;
            if (fabs(fix) < 1e-8) {
                converged = true;
                break;
            }
        }
        scale = tan(theta) / theta_d;
    } else {
        converged = true;
    }
    const bool flipped = (theta_d < 0.0 && theta > 0.0) || (theta_d > 0.0 && theta < 0.0);
    if (converged && !flipped) {
        const double X = px * scale, Y = py * scale;
        const double w = c.RR[6] * X + c.RR[7] * Y + c.RR[8];
        *u = (c.RR[0] * X + c.RR[1] * Y + c.RR[2]) / w;
        *v = (c.RR[3] * X + c.RR[4] * Y + c.RR[5]) / w;
    } else {
        *u = -1000000.0;
        *v = -1000000.0;
    }
}

// One thread per raw pixel (x, y): lut[y W + x] = float32 of its rectified position.  Registers only: no LDS, no atomics;
// the coefficients and RR arrive in the kernel-argument segment.
template <int MODEL>
__global__ __launch_bounds__(kLensBlock) void k_rectify_lut(LensCoef c, int W, unsigned long long npix, float2* __restrict__ lut)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kLensBlock + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long yi = i / (unsigned long long)W;
    const double x = (double)(i - yi * (unsigned long long)W), y = (double)yi;
    double u, v;
    if (MODEL == LENS_FISHEYE)
        lens_fisheye(c, x, y, &u, &v);
    else
        lens_plumb_bob(c, x, y, &u, &v);
    lut[i] = make_float2((float)u, (float)v);
}

}  // namespace

hipError_t launch_rectify_lut(hipStream_t s, int model, const LensCoef& c, int width, int height, float2* lut)
{
    const unsigned long long n = (unsigned long long)width * (unsigned long long)height;
    if (!lut || width < 1 || height < 1 || n >= 0xffffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kLensBlock - 1) / kLensBlock)), block(kLensBlock);  // n < 2^32: at most 2^24 workgroups
    if (model == LENS_PLUMB_BOB)
        hipLaunchKernelGGL(k_rectify_lut<LENS_PLUMB_BOB>, grid, block, 0, s, c, width, n, lut);
    else if (model == LENS_FISHEYE)
        hipLaunchKernelGGL(k_rectify_lut<LENS_FISHEYE>, grid, block, 0, s, c, width, n, lut);
    else
        return hipErrorInvalidValue;
    return hipExtGetLastError();
}

// ------------------------------------------------------------------------------------------------ volume filters ---
// Grid3D::laplacianInPlace / smoothInPlace (the free functions laplacian3D and diffuse, cartesian3dgrid_filter.cpp:72-104,
// 19-62), smoothInPlaceIIR3D (the 3-sigma gaussianiir3d, gaussianiir3d.cpp:143-251) and the reductions of
// computeMoranIndexGaussianWeights (cartesian3dgrid_filter.cpp:113-199).  DESIGN.md 7i.  Every product is an fp32 multiply
// rounded on its own (-ffp-contract=off), then an fp32 add; nothing flushes subnormals.
namespace {

// One workgroup owns a 64 x 16 tile of the x-y plane and marches over a chunk of z.  Three LDS slots hold the planes z - 1,
// z, z + 1 of the tile WITH its one-voxel rim, every cell read from the index-clamped position (homogeneous Neumann:
// the neighbour of a border voxel is the voxel itself), so a voxel costs one global read per step.  Each thread keeps its
// four voxels of the planes z - 1, z, z + 1 in registers; x and y neighbours come from the LDS slot of plane z.  The rim
// loads of plane z + 2 are in flight while plane z is computed.  One barrier per plane: plane z + 2 overwrites the slot of
// plane z - 1, which no thread reads after the barrier of plane z + 1.
constexpr int kStTX = 64, kStTY = 16, kStRows = 4;
constexpr int kStW = kStTX + 2, kStCells = kStW * (kStTY + 2);
constexpr int kStFill = (kStCells + 255) / 256;

template <bool DIFFUSE>
__global__ __launch_bounds__(256) void k_stencil3d(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz,
                                                   int zchunk, float dt)
{
    __shared__ float tile[3][kStCells];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x0 = blockIdx.x * kStTX, y0 = blockIdx.y * kStTY;
    const int z_begin = blockIdx.z * zchunk, z_end = min(nz, z_begin + zchunk);
    const size_t plane = (size_t)nx * (size_t)ny;

    size_t off[kStFill];  // this thread's cells of a slot, as clamped positions in a plane
#pragma unroll
    for (int i = 0; i < kStFill; ++i) {
        const int c = (int)threadIdx.x + 256 * i;
        const int row = c / kStW, col = c - row * kStW;
        const int gx = min(max(x0 - 1 + col, 0), nx - 1), gy = min(max(y0 - 1 + row, 0), ny - 1);
        off[i] = (size_t)gy * (size_t)nx + (size_t)gx;
    }
    float t[kStFill];
    auto load = [&](int z) {
        const float* base = src + (size_t)min(max(z, 0), nz - 1) * plane;
#pragma unroll
        for (int i = 0; i < kStFill; ++i)
            if ((int)threadIdx.x + 256 * i < kStCells) t[i] = base[off[i]];
    };
    auto put = [&](int z) {
        float* slot = tile[(z + 1) % 3];  // z >= -1
#pragma unroll
        for (int i = 0; i < kStFill; ++i)
            if ((int)threadIdx.x + 256 * i < kStCells) slot[threadIdx.x + 256 * i] = t[i];
    };
    int cell[kStRows];
#pragma unroll
    for (int r = 0; r < kStRows; ++r) cell[r] = (1 + ty + 4 * r) * kStW + 1 + tx;

    load(z_begin - 1);
    put(z_begin - 1);
    load(z_begin);
    put(z_begin);
    load(z_begin + 1);
    __syncthreads();
    float prev[kStRows], cur[kStRows];
#pragma unroll
    for (int r = 0; r < kStRows; ++r) {
        prev[r] = tile[z_begin % 3][cell[r]];
        cur[r] = tile[(z_begin + 1) % 3][cell[r]];
    }
    const int x = x0 + tx;
    for (int z = z_begin; z < z_end; ++z) {
        put(z + 1);
        load(z + 2);
        __syncthreads();
        const float* here = tile[(z + 1) % 3];
        const float* above = tile[(z + 2) % 3];
        float* out = dst + (size_t)z * plane;
#pragma unroll
        for (int r = 0; r < kStRows; ++r) {
            const int c = cell[r];
            const float v = cur[r], nxt = above[c];
            const float two_v = 2.f * v;
            const float dxx = (here[c + 1] - two_v) + here[c - 1];
            const float dyy = (here[c + kStW] - two_v) + here[c - kStW];
            const float dzz = (nxt - two_v) + prev[r];
            const float lap = (dxx + dyy) + dzz;
            const int y = y0 + ty + 4 * r;
            if (x < nx && y < ny) out[(size_t)y * (size_t)nx + (size_t)x] = DIFFUSE ? v + dt * lap : lap;
            prev[r] = v;
            cur[r] = nxt;
        }
    }
}

// The line recurrence of gaussianiir3d (gaussianiir3d.cpp:169-184), sequential by definition: p is one lane's line.  Eight
// voxels are read ahead of the chain that consumes them (the reads do not depend on it; the chain's order and roundings are
// those of the plain loop), so a chain link waits for the previous link, not for memory.
constexpr int kIirAhead = 8;
template <class Line>
__device__ __forceinline__ void iir_sweeps(Line p, int n, float nu, float bs, int numsteps)
{
    for (int step = 0; step < numsteps; ++step) {
        float prev = p.get(0) * bs;
        p.set(0, prev);
        int i = 1;
        for (; i + kIirAhead <= n; i += kIirAhead) {
            float a[kIirAhead];
#pragma unroll
            for (int k = 0; k < kIirAhead; ++k) a[k] = p.get(i + k);
#pragma unroll
            for (int k = 0; k < kIirAhead; ++k) {
                prev = a[k] + nu * prev;
                p.set(i + k, prev);
            }
        }
        for (; i < n; ++i) {
            prev = p.get(i) + nu * prev;
            p.set(i, prev);
        }
        prev = prev * bs;  // a line of one voxel is scaled twice per step, as the reference does
        p.set(n - 1, prev);
        i = n - 1;  // prev is voxel i
        for (; i - kIirAhead >= 0; i -= kIirAhead) {
            float a[kIirAhead];
#pragma unroll
            for (int k = 0; k < kIirAhead; ++k) a[k] = p.get(i - 1 - k);
#pragma unroll
            for (int k = 0; k < kIirAhead; ++k) {
                prev = a[k] + nu * prev;
                p.set(i - 1 - k, prev);
            }
        }
        for (; i > 0; --i) {
            prev = p.get(i - 1) + nu * prev;
            p.set(i - 1, prev);
        }
    }
}

struct LdsLine {  // element i of the line at base[i * stride]
    float* base;
    int stride;
    __device__ __forceinline__ float get(int i) const { return base[i * stride]; }
    __device__ __forceinline__ void set(int i, float v) const { base[i * stride] = v; }
};
struct GlobalLine {
    float* base;
    size_t stride;
    __device__ __forceinline__ float get(int i) const { return base[(size_t)i * stride]; }
    __device__ __forceinline__ void set(int i, float v) const { base[(size_t)i * stride] = v; }
};

// y and z lines: 64 lanes along x (every access coalesced), one wave per workgroup.  Line `outer * tiles + tile` starts at
// vol[outer * outer_stride + x], x < width, and steps by `stride`.  IN_LDS: the 64 lines live in LDS ([len][64], a lane
// touches its own column only: no bank conflict, no barrier), so all sweeps cost one global read and one global write;
// otherwise (a line set larger than the LDS) the sweeps run through global memory.  POST: * post on the way out.
template <bool IN_LDS, bool POST>
__global__ __launch_bounds__(64) void k_iir_strided(float* __restrict__ vol, size_t width, unsigned tiles, size_t stride,
                                                    size_t outer_stride, int len, float nu, float bs, int numsteps, float post)
{
    extern __shared__ float s_lines[];
    const unsigned outer = blockIdx.x / tiles, tile = blockIdx.x - outer * tiles;
    const size_t x = (size_t)tile * 64 + threadIdx.x;
    if (x >= width) return;
    float* p = vol + (size_t)outer * outer_stride + x;
    if (IN_LDS) {
        float* mine = s_lines + threadIdx.x;
#pragma unroll 16  // one wave per workgroup: the loads in flight are what hides HBM latency
        for (int i = 0; i < len; ++i) mine[i * 64] = p[(size_t)i * stride];
        iir_sweeps(LdsLine{mine, 64}, len, nu, bs, numsteps);
#pragma unroll 16
        for (int i = 0; i < len; ++i) p[(size_t)i * stride] = POST ? mine[i * 64] * post : mine[i * 64];
    } else {
        iir_sweeps(GlobalLine{p, stride}, len, nu, bs, numsteps);
        if (POST)
            for (int i = 0; i < len; ++i) p[(size_t)i * stride] = p[(size_t)i * stride] * post;
    }
}

// x lines: the recurrence runs along the contiguous axis.  A workgroup stages `rows` consecutive rows (one contiguous
// piece of the volume) into LDS with coalesced loads, row stride `pitch` odd so that the lanes of wave 0, one row each,
// walk distinct banks; wave 0 sweeps; all four waves store coalesced.
__global__ __launch_bounds__(256) void k_iir_x_lds(float* __restrict__ vol, int nx, size_t n_rows, int rows, int pitch, float nu,
                                                   float bs, int numsteps)
{
    extern __shared__ float s_lines[];
    const size_t row0 = (size_t)blockIdx.x * (size_t)rows;
    const int here = (int)min((size_t)rows, n_rows - row0);
    float* g = vol + row0 * (size_t)nx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < here; r += 4) {
#pragma unroll 8
        for (int c = lane; c < nx; c += 64) s_lines[r * pitch + c] = g[(size_t)r * (size_t)nx + c];
    }
    __syncthreads();
    if ((int)threadIdx.x < here) iir_sweeps(LdsLine{s_lines + threadIdx.x * pitch, 1}, nx, nu, bs, numsteps);
    __syncthreads();
    for (int r = wave; r < here; r += 4)
        for (int c = lane; c < nx; c += 64) g[(size_t)r * (size_t)nx + c] = s_lines[r * pitch + c];
}

// rows too long for the LDS: one lane per row, through global memory
__global__ __launch_bounds__(64) void k_iir_x_global(float* __restrict__ vol, int nx, size_t n_rows, float nu, float bs, int numsteps)
{
    const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= n_rows) return;
    iir_sweeps(GlobalLine{vol + row * (size_t)nx, 1}, nx, nu, bs, numsteps);
}

__global__ __launch_bounds__(256) void k_scale(float* __restrict__ vol, size_t n, float post)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) vol[i] = vol[i] * post;
}

// Sums in double with a FIXED tree: a thread's grid-stride partial, 64 lanes by shuffles, 4 waves in order, then the
// workgroups' partials folded by one workgroup the same way.  The number of workgroups depends on n alone, so two calls
// return the same bits.  words[0] = mean, words[1] = stddev, words[2] = the Moran numerator.
constexpr int VF_SUM = 0, VF_SQ_DEV = 1, VF_MORAN = 2;

__device__ __forceinline__ double vf_block_sum(double acc, double* part)
{
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);  // every thread holds the workgroup's sum
}

template <int WHAT>
__global__ __launch_bounds__(256) void k_vf_partials(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                     const double* __restrict__ words, float c, double* __restrict__ partials)
{
    __shared__ double part[4];
    const double mean = WHAT == VF_SQ_DEV ? words[0] : 0.0;
    double acc = 0.0;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        if (WHAT == VF_SUM) {
            acc += (double)a[i];
        } else if (WHAT == VF_SQ_DEV) {
            const double d = (double)a[i] - mean;
            acc += d * d;
        } else {  // cartesian3dgrid_filter.cpp:188-190: a = standardized, b = its smoothed copy, c = the centre weight
            const float z = a[i];
            const float cz = c * z;
            const float nb = b[i] - cz;
            acc += (double)(z * nb);
        }
    }
    const double sum = vf_block_sum(acc, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

template <int WHAT>
__global__ __launch_bounds__(256) void k_vf_finish(const double* __restrict__ partials, int n_part, double count,
                                                   double* __restrict__ words)
{
    __shared__ double part[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) acc += partials[i];
    const double sum = vf_block_sum(acc, part);
    if (threadIdx.x == 0) {
        if (WHAT == VF_SUM) words[0] = sum / count;
        else if (WHAT == VF_SQ_DEV) words[1] = sqrt(sum / count);
        else words[2] = sum;
    }
}

// cartesian3dgrid_filter.cpp:126-129: (v - mean) in double, times the fp32 reciprocal deviation, rounded to fp32
__global__ __launch_bounds__(256) void k_standardize(const float* __restrict__ vol, size_t n, double mean, float inv_stddev,
                                                     float* __restrict__ z, float* __restrict__ z_copy)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float v = (float)(((double)vol[i] - mean) * (double)inv_stddev);
        z[i] = v;
        z_copy[i] = v;
    }
}

}  // namespace

hipError_t launch_stencil3d(hipStream_t s, const float* src, float* dst, int nx, int ny, int nz, bool diffuse, float dt)
{
    if (!src || !dst || src == dst || nx < 1 || ny < 1 || nz < 1) return hipErrorInvalidValue;
    const unsigned bx = (unsigned)((nx + kStTX - 1) / kStTX), by = (unsigned)((ny + kStTY - 1) / kStTY);
    if (by > 65535u) return hipErrorInvalidValue;
    // chunks of z: long enough that the two extra planes a chunk reads stay cheap, short enough to fill the machine
    int zchunk = 32;
    while (zchunk > 8 && (size_t)bx * by * (size_t)((nz + zchunk - 1) / zchunk) < 2048) zchunk /= 2;
    unsigned bz = (unsigned)((nz + zchunk - 1) / zchunk);
    if (bz > 65535u) {
        zchunk = (nz + 65534) / 65535;
        bz = (unsigned)((nz + zchunk - 1) / zchunk);
    }
    const dim3 grid(bx, by, bz), block(256);
    if (diffuse)
        hipLaunchKernelGGL(k_stencil3d<true>, grid, block, 0, s, src, dst, nx, ny, nz, zchunk, dt);
    else
        hipLaunchKernelGGL(k_stencil3d<false>, grid, block, 0, s, src, dst, nx, ny, nz, zchunk, dt);
    return hipExtGetLastError();
}

// lines along `stride` (y: width = nx, n_outer = nz, outer_stride = nx ny; z: width = nx ny, n_outer = 1)
static hipError_t launch_iir_strided(hipStream_t s, float* vol, size_t width, size_t n_outer, size_t stride, size_t outer_stride,
                                     int len, float nu, float bs, int numsteps, bool with_post, float post)
{
    const size_t tiles = (width + 63) / 64, blocks = tiles * n_outer;
    if (tiles > 0x7fffffffull || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds = (size_t)len * 64 * sizeof(float);
    const bool in_lds = lds <= max_dynamic_lds();
    const dim3 grid((unsigned)blocks), block(64);
#define DSI_IIR_STRIDED(IN_LDS, POST)                                                                                          \
    do {                                                                                                                       \
        if (IN_LDS)                                                                                                            \
            if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_iir_strided<IN_LDS, POST>), lds)) return e;  \
        hipLaunchKernelGGL((k_iir_strided<IN_LDS, POST>), grid, block, IN_LDS ? lds : 0, s, vol, width, (unsigned)tiles, stride, \
                           outer_stride, len, nu, bs, numsteps, post);                                                         \
    } while (0)
    if (in_lds && with_post) DSI_IIR_STRIDED(true, true);
    else if (in_lds) DSI_IIR_STRIDED(true, false);
    else if (with_post) DSI_IIR_STRIDED(false, true);
    else DSI_IIR_STRIDED(false, false);
#undef DSI_IIR_STRIDED
    return hipExtGetLastError();
}

hipError_t launch_iir_axis(hipStream_t s, float* vol, int nx, int ny, int nz, int axis, float nu, float bs, int numsteps,
                           bool with_post, float post)
{
    if (!vol || nx < 1 || ny < 1 || nz < 1 || numsteps < 1 || axis < 0 || axis > 2) return hipErrorInvalidValue;
    const size_t plane = (size_t)nx * (size_t)ny, n = plane * (size_t)nz;
    if (axis == 1) return launch_iir_strided(s, vol, (size_t)nx, (size_t)nz, (size_t)nx, plane, ny, nu, bs, numsteps, with_post, post);
    if (axis == 2) return launch_iir_strided(s, vol, plane, 1, plane, 0, nz, nu, bs, numsteps, with_post, post);
    const size_t n_rows = (size_t)ny * (size_t)nz;
    const int pitch = nx | 1;
    const size_t fit = max_dynamic_lds() / ((size_t)pitch * sizeof(float));
    if (fit >= 8) {
        // as many rows as fit, 64 at the most (one per lane of the sweeping wave); no more than the volume needs to fill the machine
        size_t rows = std::min<size_t>(fit, 64);
        while (rows > 16 && (n_rows + rows - 1) / rows < 512) rows /= 2;
        const size_t blocks = (n_rows + rows - 1) / rows, lds = rows * (size_t)pitch * sizeof(float);
        if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_iir_x_lds), lds)) return e;
        hipLaunchKernelGGL(k_iir_x_lds, dim3((unsigned)blocks), dim3(256), lds, s, vol, nx, n_rows, (int)rows, pitch, nu, bs, numsteps);
    } else {
        const size_t blocks = (n_rows + 63) / 64;
        if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_iir_x_global, dim3((unsigned)blocks), dim3(64), 0, s, vol, nx, n_rows, nu, bs, numsteps);
    }
    if (hipError_t e = hipExtGetLastError()) return e;
    if (with_post) {
        hipLaunchKernelGGL(k_scale, dim3(grid_for(n, 256)), dim3(256), 0, s, vol, n, post);
        return hipExtGetLastError();
    }
    return hipSuccess;
}

size_t volume_sum_words() { return 4 + (size_t)kVolumeSumBlocks; }

static hipError_t launch_vf_sum(hipStream_t s, int what, const float* a, const float* b, size_t n, float c, double* words)
{
    if (!a || !words || n < 1) return hipErrorInvalidValue;
    const int blocks = grid_for(n, 256, kVolumeSumBlocks);
    double* partials = words + 4;
    const double count = (double)n;
    if (what == VF_SUM) {
        hipLaunchKernelGGL(k_vf_partials<VF_SUM>, dim3(blocks), dim3(256), 0, s, a, b, n, words, c, partials);
        hipLaunchKernelGGL(k_vf_finish<VF_SUM>, dim3(1), dim3(256), 0, s, partials, blocks, count, words);
    } else if (what == VF_SQ_DEV) {
        hipLaunchKernelGGL(k_vf_partials<VF_SQ_DEV>, dim3(blocks), dim3(256), 0, s, a, b, n, words, c, partials);
        hipLaunchKernelGGL(k_vf_finish<VF_SQ_DEV>, dim3(1), dim3(256), 0, s, partials, blocks, count, words);
    } else {
        hipLaunchKernelGGL(k_vf_partials<VF_MORAN>, dim3(blocks), dim3(256), 0, s, a, b, n, words, c, partials);
        hipLaunchKernelGGL(k_vf_finish<VF_MORAN>, dim3(1), dim3(256), 0, s, partials, blocks, count, words);
    }
    return hipExtGetLastError();
}

hipError_t launch_volume_mean_std(hipStream_t s, const float* vol, size_t n, double* words)
{
    if (hipError_t e = launch_vf_sum(s, VF_SUM, vol, nullptr, n, 0.f, words)) return e;
    return launch_vf_sum(s, VF_SQ_DEV, vol, nullptr, n, 0.f, words);
}

hipError_t launch_volume_standardize(hipStream_t s, const float* vol, size_t n, double mean, float inv_stddev, float* z, float* z_copy)
{
    if (!vol || !z || !z_copy || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_standardize, dim3(grid_for(n, 256)), dim3(256), 0, s, vol, n, mean, inv_stddev, z, z_copy);
    return hipExtGetLastError();
}

hipError_t launch_volume_moran_numerator(hipStream_t s, const float* z, const float* smooth, size_t n, float centre, double* words)
{
    if (!smooth) return hipErrorInvalidValue;
    return launch_vf_sum(s, VF_MORAN, z, smooth, n, centre, words);
}

}  // namespace dsi
