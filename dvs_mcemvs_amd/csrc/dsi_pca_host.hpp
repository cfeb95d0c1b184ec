// The arithmetic of include/dsi_map_pca.h from one cell's integer moments on: the centred scatter matrix, the 3 x 3 Jacobi
// eigen-solve, the flags, the signs, the label and the row.  Plain C++ with no HIP in it, so that a stand-alone program can
// run it under the host sanitizers (tests/cpp/pca_solve_sanitize.cpp); dsi_engine.cpp wraps it in dsx_pca_solve, and
// dsi_kernels.hip includes it with DSI_PCA_FN naming the device too, so that k_map_pca runs these very statements.  Every
// index into A and V is a compile-time constant: in a kernel the eighteen doubles stay in registers.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef DSI_PCA_FN
#define DSI_PCA_FN inline
#endif

namespace dsi {

constexpr int kPcaSweeps = 8;
constexpr uint32_t kPcaMaxMembers = 343;  // (2 * 3 + 1)^3: the neighbours of reach 3 and the cell itself
constexpr int64_t kPcaMaxOffset = 3073;   // |D| <= 3 * 2^10 + 1
constexpr double kPcaQuantumPerLeaf = 0x1p-10;
constexpr double kPcaSeparation = 0x1p-26;

struct PcaSolved {
    double normal[3], tangent[3], lambda[3];
    float normal_f[3], tangent_f[3], eval[3];
    uint8_t label, flags;
};

// one Jacobi rotation of the pair (P, Q), dsx_map_align_solve's: columns from the old pair, then rows, then V
template <int P, int Q>
DSI_PCA_FN void pca_rotate(double (&A)[3][3], double (&V)[3][3])
{
    if (A[P][Q] == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * A[P][Q]);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
    {
        const double a0p = A[0][P], a0q = A[0][Q], a1p = A[1][P], a1q = A[1][Q], a2p = A[2][P], a2q = A[2][Q];
        A[0][P] = c * a0p - s * a0q, A[0][Q] = s * a0p + c * a0q;
        A[1][P] = c * a1p - s * a1q, A[1][Q] = s * a1p + c * a1q;
        A[2][P] = c * a2p - s * a2q, A[2][Q] = s * a2p + c * a2q;
    }
    {
        const double ap0 = A[P][0], aq0 = A[Q][0], ap1 = A[P][1], aq1 = A[Q][1], ap2 = A[P][2], aq2 = A[Q][2];
        A[P][0] = c * ap0 - s * aq0, A[Q][0] = s * ap0 + c * aq0;
        A[P][1] = c * ap1 - s * aq1, A[Q][1] = s * ap1 + c * aq1;
        A[P][2] = c * ap2 - s * aq2, A[Q][2] = s * ap2 + c * aq2;
    }
    {
        const double v0p = V[0][P], v0q = V[0][Q], v1p = V[1][P], v1q = V[1][Q], v2p = V[2][P], v2q = V[2][Q];
        V[0][P] = c * v0p - s * v0q, V[0][Q] = s * v0p + c * v0q;
        V[1][P] = c * v1p - s * v1q, V[1][Q] = s * v1p + c * v1q;
        V[2][P] = c * v2p - s * v2q, V[2][Q] = s * v2p + c * v2q;
    }
}

// a[i] without an index at run time
DSI_PCA_FN double pca_pick(double a0, double a1, double a2, int i) { return i == 0 ? a0 : i == 1 ? a1 : a2; }

// (x, y, z) / its norm, the component of largest magnitude made positive (the first among equals)
DSI_PCA_FN void pca_unit_canonical(double x, double y, double z, double (&out)[3])
{
    const double norm = std::sqrt(((x * x + y * y) + z * z));
    x = x / norm, y = y / norm, z = z / norm;
    const double ax = std::fabs(x), ay = std::fabs(y), az = std::fabs(z);
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    if (lead < 0.0) x = -x, y = -y, z = -z;
    out[0] = x, out[1] = y, out[2] = z;
}

// steps 3-7 of the rule and the row of step 8; m = found + 1 in 1..343 and moments within the bounds (the callers' business).
// viewpoint and p are read only when orient
DSI_PCA_FN void pca_solve_core(uint32_t m, const int64_t (&s)[3], const int64_t (&ss)[6], double quantum, int orient,
                               const double (&viewpoint)[3], const double (&p)[3], PcaSolved& out)
{
    const int64_t mi = (int64_t)m;
    const double cxx = (double)(mi * ss[0] - s[0] * s[0]), cxy = (double)(mi * ss[1] - s[0] * s[1]), cxz = (double)(mi * ss[2] - s[0] * s[2]);
    const double cyy = (double)(mi * ss[3] - s[1] * s[1]), cyz = (double)(mi * ss[4] - s[1] * s[2]), czz = (double)(mi * ss[5] - s[2] * s[2]);
    double A[3][3] = {{cxx, cxy, cxz}, {cxy, cyy, cyz}, {cxz, cyz, czz}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kPcaSweeps; ++sweep) {
        pca_rotate<0, 1>(A, V);
        pca_rotate<0, 2>(A, V);
        pca_rotate<1, 2>(A, V);
    }
    const double e0 = A[0][0] < 0.0 ? 0.0 : A[0][0], e1 = A[1][1] < 0.0 ? 0.0 : A[1][1], e2 = A[2][2] < 0.0 ? 0.0 : A[2][2];
    const int i0 = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);  // the first minimum
    // the first maximum among the other two
    const int ia = i0 == 0 ? 1 : 0, ib = i0 == 2 ? 1 : 2;
    const int i2 = pca_pick(e0, e1, e2, ia) >= pca_pick(e0, e1, e2, ib) ? ia : ib;
    const int i1 = 3 - i0 - i2;
    const double l0 = pca_pick(e0, e1, e2, i0), l1 = pca_pick(e0, e1, e2, i1), l2 = pca_pick(e0, e1, e2, i2);
    out.lambda[0] = l0, out.lambda[1] = l1, out.lambda[2] = l2;
    pca_unit_canonical(pca_pick(V[0][0], V[0][1], V[0][2], i0), pca_pick(V[1][0], V[1][1], V[1][2], i0),
                       pca_pick(V[2][0], V[2][1], V[2][2], i0), out.normal);
    pca_unit_canonical(pca_pick(V[0][0], V[0][1], V[0][2], i2), pca_pick(V[1][0], V[1][1], V[1][2], i2),
                       pca_pick(V[2][0], V[2][1], V[2][2], i2), out.tangent);
    if (orient) {
        const double w0 = viewpoint[0] - p[0], w1 = viewpoint[1] - p[1], w2 = viewpoint[2] - p[2];
        const double dot = ((out.normal[0] * w0 + out.normal[1] * w1) + out.normal[2] * w2);
        if (dot < 0.0) out.normal[0] = -out.normal[0], out.normal[1] = -out.normal[1], out.normal[2] = -out.normal[2];
    }
    const double size = (l0 + l1) + l2;
    out.flags = (uint8_t)((l1 - l0 > kPcaSeparation * size ? 1u : 0u) | (l2 - l1 > kPcaSeparation * size ? 2u : 0u));
    const double g0 = std::sqrt(l0), g1 = std::sqrt(l1), g2 = std::sqrt(l2);
    const double lin = g2 - g1, pla = g1 - g0;
    out.label = (uint8_t)((lin >= pla && lin >= g0) ? 1u : (pla >= g0 ? 2u : 3u));
    const double md = (double)m, mm = md * md, qq = quantum * quantum;
    out.eval[0] = (float)((l0 / mm) * qq), out.eval[1] = (float)((l1 / mm) * qq), out.eval[2] = (float)((l2 / mm) * qq);
    out.normal_f[0] = (float)out.normal[0], out.normal_f[1] = (float)out.normal[1], out.normal_f[2] = (float)out.normal[2];
    out.tangent_f[0] = (float)out.tangent[0], out.tangent_f[1] = (float)out.tangent[1], out.tangent_f[2] = (float)out.tangent[2];
}

enum PcaSolveError { kPcaOk = 0, kPcaBadMembers, kPcaMomentsTooLarge, kPcaNegativeVariance };

// the moments that no pass can return are refused, then pca_solve_core
inline PcaSolveError pca_solve_host(uint32_t m, const int64_t s[3], const int64_t ss[6], double quantum, int orient, const double viewpoint[3],
                                    const double p[3], PcaSolved* out)
{
    if (m < 1 || m > kPcaMaxMembers) return kPcaBadMembers;
    const int64_t bound_s = (int64_t)(m - 1) * kPcaMaxOffset, bound_ss = bound_s * kPcaMaxOffset;
    for (int a = 0; a < 3; ++a)
        if (s[a] > bound_s || s[a] < -bound_s) return kPcaMomentsTooLarge;
    for (int ab = 0; ab < 6; ++ab)
        if (ss[ab] > bound_ss || ss[ab] < -bound_ss) return kPcaMomentsTooLarge;
    if (ss[0] < 0 || ss[3] < 0 || ss[5] < 0) return kPcaMomentsTooLarge;
    const int64_t mi = (int64_t)m;
    if (mi * ss[0] - s[0] * s[0] < 0 || mi * ss[3] - s[1] * s[1] < 0 || mi * ss[5] - s[2] * s[2] < 0) return kPcaNegativeVariance;
    const int64_t s3[3] = {s[0], s[1], s[2]}, ss6[6] = {ss[0], ss[1], ss[2], ss[3], ss[4], ss[5]};
    const double vp[3] = {orient ? viewpoint[0] : 0.0, orient ? viewpoint[1] : 0.0, orient ? viewpoint[2] : 0.0};
    const double pp[3] = {orient ? p[0] : 0.0, orient ? p[1] : 0.0, orient ? p[2] : 0.0};
    pca_solve_core(m, s3, ss6, quantum, orient, vp, pp, *out);
    return kPcaOk;
}

}  // namespace dsi
