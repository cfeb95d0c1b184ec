// dsi::GroundTruthProjector through the C++ adapter: the fixture's cases, read from files, are projected in both modes from
// the float32 disparity image and from the PNG's 16-bit samples, and the depth maps and counts are written back for
// tests/test_gpu_ground_truth.py to compare with the fixture.  Without a device the context's constructor throws and the
// program says so.
//   test_ground_truth DIR   reads  DIR/cases.txt (one "name rows cols" per line), DIR/<name>.d.f32, <name>.raw.u16,
//                                  <name>.calib.f64 (Q[16] T[16] K[12])
//                           writes DIR/<name>.<mode>.<f32|u16>.depth.f32 and DIR/results.txt
//                                  ("name mode input n_points n_outside" per projection)
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dsi_engine.hpp"

// a call site that only has to compile: a mapper's resident maps against a projector
void compile_only(dsi::DepthScore& score, EMVS::MapperEMVS& mapper, dsi::GroundTruthProjector& projector)
{
    score.addMapper(mapper, projector);
}

namespace {

template <typename T>
std::vector<T> read_all(const std::string& path, size_t n)
{
    std::vector<T> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot read " + path);
    const size_t got = std::fread(v.data(), sizeof(T), n, f);
    std::fclose(f);
    if (got != n) throw std::runtime_error("short file " + path);
    return v;
}

void write_all(const std::string& path, const std::vector<float>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    std::fwrite(v.data(), sizeof(float), v.size(), f);
    std::fclose(f);
}

int run(const std::string& dir)
{
    dsi::Context ctx(0);  // throws without a device
    FILE* list = std::fopen((dir + "/cases.txt").c_str(), "r");
    if (!list) throw std::runtime_error("cannot read " + dir + "/cases.txt");
    FILE* res = std::fopen((dir + "/results.txt").c_str(), "w");
    if (!res) {
        std::fclose(list);
        throw std::runtime_error("cannot write " + dir + "/results.txt");
    }
    int failures = 0;
    char name[128];
    int rows = 0, cols = 0;
    while (std::fscanf(list, "%127s %d %d", name, &rows, &cols) == 3) {
        const std::string base = dir + "/" + name;
        const size_t npix = (size_t)rows * cols;
        const std::vector<double> calib = read_all<double>(base + ".calib.f64", 44);
        dsi::Image<float> disp(rows, cols);
        dsi::Image<uint16_t> raw(rows, cols);
        disp.data = read_all<float>(base + ".d.f32", npix);
        raw.data = read_all<uint16_t>(base + ".raw.u16", npix);
        const int modes[2] = {DSI_GT_AS_SCRIPT, DSI_GT_DROP_OUTSIDE};
        const char* mode_names[2] = {"script", "drop"};
        for (int k = 0; k < 2; ++k) {
            dsi::GroundTruthProjector gt(ctx, cols, rows, calib.data(), calib.data() + 16, calib.data() + 32, modes[k]);
            for (int u16 = 0; u16 < 2; ++u16) {
                if (u16)
                    gt.projectPng16(raw);
                else
                    gt.project(disp);
                dsi::Image<float> depth;
                uint64_t n_points = 0, n_outside = 0;
                gt.fetch(depth, &n_points, &n_outside);
                if (depth.rows != rows || depth.cols != cols || !gt.devicePtr()) {
                    std::fprintf(stderr, "FAILED %s: fetch gave another size or no device map\n", name);
                    ++failures;
                }
                write_all(base + "." + mode_names[k] + (u16 ? ".u16" : ".f32") + ".depth.f32", depth.data);
                std::fprintf(res, "%s %s %s %llu %llu\n", name, mode_names[k], u16 ? "u16" : "f32", (unsigned long long)n_points,
                             (unsigned long long)n_outside);
            }
            // a window scored against the projector's map equals the same window against the fetched map
            dsi::Image<float> fetched, est(rows, cols);
            dsi::Image<uint8_t> mask(rows, cols);
            gt.fetch(fetched);
            for (size_t i = 0; i < npix; ++i) {
                est.data[i] = fetched.data[i] * (1.0f + 0.01f * (float)(i % 7));
                mask.data[i] = (uint8_t)(i % 3 != 0);
            }
            dsi::DepthScore a(ctx, npix, 0.6, 557.25), b(ctx, npix, 0.6, 557.25);
            a.add(est, mask, gt);
            b.add(est, mask, fetched);
            const dsi_score_metrics_t ma = a.metrics(), mb = b.metrics();
            if (ma.n_joint != mb.n_joint || ma.n_gt != mb.n_gt || std::memcmp(&ma.sum_abs, &mb.sum_abs, sizeof(double)) ||
                std::memcmp(&ma.sum_di, &mb.sum_di, sizeof(double)) || std::memcmp(&ma.median_abs, &mb.median_abs, sizeof(double))) {
                std::fprintf(stderr, "FAILED %s %s: add(projector) differs from add(fetched map)\n", name, mode_names[k]);
                ++failures;
            }
            // sizes are checked by the adapter and by the engine
            try {
                dsi::Image<float> wrong(rows + 1, cols);
                gt.project(wrong);
                std::fprintf(stderr, "FAILED: an image of another size was accepted\n");
                ++failures;
            } catch (const dsi::Error& e) {
                if (e.code != DSI_ERR_INVALID) ++failures;
            }
            try {
                dsi::Image<float> e2(rows + 1, cols);
                dsi::Image<uint8_t> m2(rows + 1, cols);
                a.add(e2, m2, gt);
                std::fprintf(stderr, "FAILED: maps of another size than the projector's were accepted\n");
                ++failures;
            } catch (const dsi::Error& e) {
                if (e.code != DSI_ERR_INVALID) ++failures;
            }
        }
    }
    std::fclose(list);
    std::fclose(res);
    return failures;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: test_ground_truth DIR\n");
        return 2;
    }
    try {
        const int failures = run(argv[1]);
        if (failures)
            std::printf("%d check(s) FAILED\n", failures);
        else
            std::printf("all checks passed\n");
        return failures ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "test_ground_truth: %s\n", e.what());
        return 3;
    }
}
