// dsi::DepthScore through the C++ adapter: a stack of windows read from files is added window by window, from dsi::Image
// maps, and the metrics and curves are written back for tests/test_gpu_score.py to compare with the recorded output of the
// reference's programs.  Without a device the context's constructor throws and the program says so.
//   test_score DIR    reads  DIR/case.txt ("windows rows cols baseline focal"), est.f32, mask.u8, gt.f32
//                     writes DIR/metrics.txt (one "name value" per line; doubles as %a) and DIR/curves.f64
//                            (base | precision | recall | f1 | outliers, n_bins doubles each)
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dsi_engine.hpp"

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

int run(const std::string& dir)
{
    dsi::Context ctx(0);  // throws without a device
    int windows = 0, rows = 0, cols = 0;
    double b = 0, f = 0;
    {
        FILE* c = std::fopen((dir + "/case.txt").c_str(), "r");
        if (!c) throw std::runtime_error("cannot read " + dir + "/case.txt");
        const int got = std::fscanf(c, "%d %d %d %lf %lf", &windows, &rows, &cols, &b, &f);
        std::fclose(c);
        if (got != 5) throw std::runtime_error("case.txt: expected 'windows rows cols baseline focal'");
    }
    const size_t npix = (size_t)rows * cols, n = npix * windows;
    const std::vector<float> est = read_all<float>(dir + "/est.f32", n), gt = read_all<float>(dir + "/gt.f32", n);
    const std::vector<uint8_t> mask = read_all<uint8_t>(dir + "/mask.u8", n);

    dsi::DepthScore score(ctx, n, b, f);
    for (int w = 0; w < windows; ++w) {
        dsi::Image<float> d(rows, cols), g(rows, cols);
        dsi::Image<uint8_t> m(rows, cols);
        std::memcpy(d.data.data(), est.data() + w * npix, npix * sizeof(float));
        std::memcpy(g.data.data(), gt.data() + w * npix, npix * sizeof(float));
        std::memcpy(m.data.data(), mask.data() + w * npix, npix);
        score.add(d, m, g);
    }
    const dsi_score_metrics_t r = score.metrics();
    const dsi::ScoreCurves c = score.curves(0.01);
    int failures = 0;
    if (score.median() != r.median_abs && r.n_joint) {
        std::fprintf(stderr, "FAILED median() != metrics().median_abs\n");
        ++failures;
    }
    // a mismatched size is refused by the adapter before anything is queued
    try {
        dsi::Image<float> d(rows, cols), g(rows + 1, cols);
        dsi::Image<uint8_t> m(rows, cols);
        score.add(d, m, g);
        std::fprintf(stderr, "FAILED: maps of different sizes were accepted\n");
        ++failures;
    } catch (const dsi::Error& e) {
        if (e.code != DSI_ERR_INVALID) ++failures;
    }
    FILE* o = std::fopen((dir + "/metrics.txt").c_str(), "w");
    if (!o) throw std::runtime_error("cannot write " + dir + "/metrics.txt");
    std::fprintf(o, "n_est %llu\nn_gt %llu\nn_joint %llu\nn_delta0 %llu\nn_delta1 %llu\nn_delta2 %llu\nn_bad %llu\nn_stored %llu\n",
                 (unsigned long long)r.n_est, (unsigned long long)r.n_gt, (unsigned long long)r.n_joint,
                 (unsigned long long)r.n_delta[0], (unsigned long long)r.n_delta[1], (unsigned long long)r.n_delta[2],
                 (unsigned long long)r.n_bad, (unsigned long long)r.n_stored);
    std::fprintf(o, "overflow %d\nguard_intact %d\nn_bins %zu\n", (int)r.overflow, (int)r.guard_intact, c.base.size());
    const struct {
        const char* name;
        double v;
    } reals[] = {{"sum_di", r.sum_di}, {"sum_di2", r.sum_di2}, {"sum_are", r.sum_are}, {"sum_abs", r.sum_abs}, {"max_gt", r.max_gt},
                 {"delta0", r.delta[0]}, {"delta1", r.delta[1]}, {"delta2", r.delta[2]}, {"silog", r.silog}, {"are", r.are},
                 {"lrmse", r.lrmse}, {"badp", r.badp}, {"mean_abs", r.mean_abs}, {"median_abs", r.median_abs}};
    for (const auto& kv : reals) std::fprintf(o, "%s %a\n", kv.name, kv.v);
    std::fclose(o);
    o = std::fopen((dir + "/curves.f64").c_str(), "wb");
    if (!o) throw std::runtime_error("cannot write " + dir + "/curves.f64");
    for (const std::vector<double>* v : {&c.base, &c.precision, &c.recall, &c.f1, &c.outliers})
        if (!v->empty()) std::fwrite(v->data(), sizeof(double), v->size(), o);
    std::fclose(o);
    return failures;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: test_score DIR\n");
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
        std::fprintf(stderr, "test_score: %s\n", e.what());
        return 3;
    }
}
