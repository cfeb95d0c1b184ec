// The host-only arithmetic of include/dsi_map_knn.h: the 128-bit sum of squares put together from the kernel's two words, and
// the outlier threshold.  Plain C++ with no HIP in it, so that a stand-alone program can run it under the host sanitizers
// (tests/cpp/knn_threshold_sanitize.cpp); dsi_engine.cpp wraps it in dsx_map_knn_threshold.
#pragma once
#include <cmath>
#include <cstdint>

namespace dsi {

constexpr uint64_t kKnnQOne = (uint64_t)1 << 30;  // q of a mean distance equal to the radius
constexpr uint64_t kKnnMaxCells = (uint64_t)1 << 27;

// sum q^2 = lo + hi * 2^32 from k_map_knn_self's two accumulators (neither above 2^59): out = low word, high word
inline void knn_sum_q2(uint64_t lo, uint64_t hi, uint64_t out[2])
{
    const unsigned __int128 s = (unsigned __int128)lo + ((unsigned __int128)hi << 32);
    out[0] = (uint64_t)s;
    out[1] = (uint64_t)(s >> 64);
}

enum KnnThresholdError { kKnnOk = 0, kKnnTooManyCells, kKnnMomentsTooLarge, kKnnNegativeVariance };

// V = N sum_q2 - sum_q^2 exactly; mu = sum_q / N; sigma = sqrt(V / (N (N - 1))) (N >= 2, else 0); T = mu + std_mult sigma;
// T_q = T >= 2^30 ? 2^30 : T < 0 ? 0 : floor(T); N == 0: mu = sigma = 0, T_q = 2^30.  Every operation rounded on its own (the
// file is built without FMA contraction); the integer-to-double conversions round to nearest even.  std_mult is finite.
inline KnnThresholdError knn_threshold_host(uint64_t N, uint64_t sum_q, const uint64_t sum_q2[2], double std_mult, double* mu,
                                            double* sigma, uint64_t* T_q)
{
    typedef unsigned __int128 u128;
    const u128 s2 = ((u128)sum_q2[1] << 64) | (u128)sum_q2[0];
    if (N > kKnnMaxCells) return kKnnTooManyCells;
    if (sum_q > N * kKnnQOne || s2 > (u128)N * kKnnQOne * kKnnQOne) return kKnnMomentsTooLarge;
    const u128 a = (u128)N * s2, b = (u128)sum_q * (u128)sum_q;  // (N <= 2^27, s2 <= 2^87, sum_q <= 2^57: both below 2^115)
    if (a < b) return kKnnNegativeVariance;
    const u128 V = a - b;
    *mu = *sigma = 0.0;
    *T_q = kKnnQOne;
    if (N == 0) return kKnnOk;
    *mu = (double)sum_q / (double)N;
    if (N >= 2) *sigma = std::sqrt((double)V / ((double)N * (double)(N - 1)));
    const double T = *mu + std_mult * *sigma;
    *T_q = T >= (double)kKnnQOne ? kKnnQOne : T < 0.0 ? 0 : (uint64_t)std::floor(T);
    return kKnnOk;
}

}  // namespace dsi
