// The host-only arithmetic of include/dsi_map_pca.h (dvs_mcemvs_amd/csrc/dsi_pca_host.hpp: the refusals, the centred scatter
// matrix, the Jacobi eigen-solve, flags, signs, label and row) as a stand-alone program for the host sanitizers.
// tests/test_map_pca_cpu.py builds it with -fsanitize=address,undefined and compares what it prints with the restatement.
//   pca_solve_sanitize < cases
// reads  lines of "m s0 s1 s2 ss0 .. ss5 quantum orient vx vy vz px py pz" (the doubles as hexadecimal floats)
// prints per line "error label flags" and, as hexadecimal floats, normal_d[3] tangent_d[3] lambda[3] normal[3] tangent[3] eval[3]
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../dvs_mcemvs_amd/csrc/dsi_pca_host.hpp"

int main()
{
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        uint32_t m = 0;
        int64_t s[3], ss[6];
        double quantum = 0.0, vp[3], p[3];
        int orient = 0;
        if (std::sscanf(line,
                        "%" SCNu32 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64
                        " %la %d %la %la %la %la %la %la",
                        &m, &s[0], &s[1], &s[2], &ss[0], &ss[1], &ss[2], &ss[3], &ss[4], &ss[5], &quantum, &orient, &vp[0], &vp[1], &vp[2],
                        &p[0], &p[1], &p[2]) != 18)
            return 2;
        dsi::PcaSolved r;
        std::memset(&r, 0, sizeof r);
        const int e = (int)dsi::pca_solve_host(m, s, ss, quantum, orient, vp, p, &r);
        std::printf("%d %u %u", e, (unsigned)r.label, (unsigned)r.flags);
        for (int a = 0; a < 3; ++a) std::printf(" %a", r.normal[a]);
        for (int a = 0; a < 3; ++a) std::printf(" %a", r.tangent[a]);
        for (int a = 0; a < 3; ++a) std::printf(" %a", r.lambda[a]);
        for (int a = 0; a < 3; ++a) std::printf(" %a", (double)r.normal_f[a]);
        for (int a = 0; a < 3; ++a) std::printf(" %a", (double)r.tangent_f[a]);
        for (int a = 0; a < 3; ++a) std::printf(" %a", (double)r.eval[a]);
        std::printf("\n");
    }
    return 0;
}
