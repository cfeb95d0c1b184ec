// The volume filters called as the reference spells them, with its default arguments (gaussianiir3d.h:27-29,
// cartesian3dgrid_filter.cpp:9-13,66-69,107-110,113): smoothInPlace, smoothInPlaceIIR3D, laplacianInPlace,
// computeMoranIndexGaussianWeights, computeMeanStd.  Run by tests/test_gpu_volume_filters.py, which writes the arrays compared
// against here (tests/volume_filters_reference.py):
//   test_volume_filters DIR NX NY NZ   in.f32, want_laplacian.f32, want_diffuse_default.f32, want_diffuse_07.f32,
//                                      want_iir_default.f32, want_iir_mixed.f32 (0.7, 1.3, 2), stats.f64 (mean, stddev,
//                                      Moran's index at sigma 1, its tolerance)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dsi_engine.hpp"

namespace {

int failures = 0;
#define EXPECT(c)                                                              \
    do {                                                                       \
        if (!(c)) {                                                            \
            std::fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

template <typename T>
std::vector<T> read(const std::string& path, size_t count)
{
    std::vector<T> v(count);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot read " + path);
    const size_t got = std::fread(v.data(), sizeof(T), count, f);
    std::fclose(f);
    if (got != count) throw std::runtime_error("short file " + path);
    return v;
}

bool same(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

void run(const std::string& dir, unsigned nx, unsigned ny, unsigned nz)
{
    const size_t n = (size_t)nx * ny * nz;
    const std::vector<float> in = read<float>(dir + "/in.f32", n);
    const std::vector<double> stats = read<double>(dir + "/stats.f64", 4);
    Grid3D g(nx, ny, nz);

    g.upload(in);
    g.laplacianInPlace();
    EXPECT(same(g.download(), read<float>(dir + "/want_laplacian.f32", n)));

    g.upload(in);
    g.smoothInPlace();  // sigma = 1
    EXPECT(same(g.download(), read<float>(dir + "/want_diffuse_default.f32", n)));
    g.upload(in);
    g.smoothInPlace(0.7f);
    EXPECT(same(g.download(), read<float>(dir + "/want_diffuse_07.f32", n)));

    g.upload(in);
    g.smoothInPlaceIIR3D();  // sigmas 1, 1, 1; three steps
    EXPECT(same(g.download(), read<float>(dir + "/want_iir_default.f32", n)));
    g.upload(in);
    g.smoothInPlaceIIR3D(0.7f, 1.3f, 2.f);
    EXPECT(same(g.download(), read<float>(dir + "/want_iir_mixed.f32", n)));

    g.upload(in);
    const Grid3D& cg = g;  // the two statistics are const members
    double mean = 0, stddev = 0;
    cg.computeMeanStd(&mean, &stddev);
    EXPECT(std::fabs(mean - stats[0]) <= 1e-10 * std::fabs(stats[0]));
    EXPECT(std::fabs(stddev - stats[1]) <= 1e-10 * std::fabs(stats[1]));
    const double moran = cg.computeMoranIndexGaussianWeights(1.f);
    EXPECT(std::fabs(moran - stats[2]) <= stats[3]);
    EXPECT(same(g.download(), in));  // Moran's index leaves the grid alone

    bool refused = false;
    try {
        g.smoothInPlace(0.f);
    } catch (const dsi::Error& e) {
        refused = e.code == DSI_ERR_INVALID;
    }
    EXPECT(refused);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: test_volume_filters DIR NX NY NZ\n");
        return 2;
    }
    try {
        run(argv[1], (unsigned)std::atoi(argv[2]), (unsigned)std::atoi(argv[3]), (unsigned)std::atoi(argv[4]));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
