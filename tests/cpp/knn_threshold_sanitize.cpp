// The host-only arithmetic of include/dsi_map_knn.h (dvs_mcemvs_amd/csrc/dsi_knn_host.hpp: the outlier threshold and the
// 128-bit sum of squares) as a stand-alone program for the host sanitizers.  tests/test_map_knn_cpu.py builds it with
// -fsanitize=address,undefined and compares what it prints with exact Python arithmetic.
//   knn_threshold_sanitize < cases
// reads  lines of "N sum_q sum_q2_low sum_q2_high std_mult" (std_mult as a hexadecimal float) and lines of "S lo hi"
// prints per line "error mu sigma T_q" (mu and sigma as hexadecimal floats) or "low high"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../dvs_mcemvs_amd/csrc/dsi_knn_host.hpp"

int main()
{
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        uint64_t a = 0, b = 0, w[2] = {0, 0};
        double std_mult = 0.0;
        if (line[0] == 'S') {
            if (std::sscanf(line + 1, "%" SCNu64 " %" SCNu64, &a, &b) != 2) return 2;
            dsi::knn_sum_q2(a, b, w);
            std::printf("%" PRIu64 " %" PRIu64 "\n", w[0], w[1]);
            continue;
        }
        if (std::sscanf(line, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la", &a, &b, &w[0], &w[1], &std_mult) != 5) return 2;
        double mu = -1.0, sigma = -1.0;
        uint64_t T_q = 0;
        const int e = (int)dsi::knn_threshold_host(a, b, w, std_mult, &mu, &sigma, &T_q);
        std::printf("%d %a %a %" PRIu64 "\n", e, mu, sigma, T_q);
    }
    return 0;
}
