// dsi::WorldMap::integrateDepth / integrateGroundTruth / compare / fetchDistances and dsi::map_f_score.  Run by
// tests/test_gpu_map_eval_cpp.py, which writes the calls and the depth image this program reads and compares the files
// it writes with the numpy restatement (tests/map_eval_reference.py).
//   test_map_eval DIR leaf_a n_calls_a leaf_b n_calls_b n_bins width height fx fy cx cy min_depth max_depth radius...
// reads  DIR/a_<k>.f32, DIR/b_<k>.f32 (N x 3 floats, integrated with the identity pose), DIR/depth.f32, DIR/mask.u8
//        (height x width), DIR/T_w_c.f64 (12 doubles)
// writes DIR/cmp_<ab|ba>_<r>.{hist.u64,info.u64,keys.u64,dist.f32} per radius index r; info = n_cells, n_matched,
//        n_unmatched, sum_q, reach;  DIR/f_<r>.f64 = thresholds, precision, recall, f1 (n_bins each);
//        DIR/depth_cells.{keys.u64,n.u32,windows.u32,xyz.f32} and DIR/depth_info.u64 = n_points, n_rejected
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
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
std::vector<T> read(const std::string& path)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot read " + path);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && std::fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) throw std::runtime_error("short read of " + path);
    std::fclose(f);
    return v;
}

void write(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    if (bytes) std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

bool refused(const std::function<void()>& f, int code)
{
    try {
        f();
    } catch (const dsi::Error& e) {
        return e.code == code;
    }
    return false;
}

void dump(const std::string& base, dsi::WorldMap& a, const dsi::MapCompareResult& r)
{
    const dsi::MapDistances dd = a.fetchDistances();
    EXPECT(dd.size() == r.info.n_cells && r.info.n_cells == r.info.n_matched + r.info.n_unmatched);
    uint64_t in_bins = 0, finite = 0;
    for (uint64_t h : r.hist) in_bins += h;
    for (float v : dd.dist) finite += std::isfinite(v) ? 1 : 0;
    EXPECT(in_bins == r.info.n_matched && finite == r.info.n_matched);
    const uint64_t iv[5] = {r.info.n_cells, r.info.n_matched, r.info.n_unmatched, r.info.sum_q, (uint64_t)r.info.reach};
    write(base + ".info.u64", iv, sizeof iv);
    write(base + ".hist.u64", r.hist.data(), r.hist.size() * sizeof(uint64_t));
    write(base + ".keys.u64", dd.keys.data(), dd.keys.size() * sizeof(uint64_t));
    write(base + ".dist.f32", dd.dist.data(), dd.dist.size() * sizeof(float));
}

int run(int argc, char** a)
{
    const std::string dir = a[1];
    const double leaf_a = std::atof(a[2]), leaf_b = std::atof(a[4]);
    const int calls_a = std::atoi(a[3]), calls_b = std::atoi(a[5]), n_bins = std::atoi(a[6]);
    const int width = std::atoi(a[7]), height = std::atoi(a[8]);
    const double fx = std::atof(a[9]), fy = std::atof(a[10]), cx = std::atof(a[11]), cy = std::atof(a[12]);
    const double min_depth = std::atof(a[13]), max_depth = std::atof(a[14]);

    dsi::Context ctx(0);
    dsi::WorldMap A(ctx, leaf_a, 8), B(ctx, leaf_b, 8);
    EXPECT(refused([&] { A.fetchDistances(); }, DSI_ERR_INVALID));  // nothing compared yet
    const std::array<double, 12> identity = dsi::pose_matrix(dsi::Transformation());
    for (int k = 0; k < calls_a; ++k) {
        const auto pts = read<float>(dir + "/a_" + std::to_string(k) + ".f32");
        EXPECT(A.integrate(pts.data(), 3, pts.size() / 3, identity) == 0);
    }
    for (int k = 0; k < calls_b; ++k) {
        const auto pts = read<float>(dir + "/b_" + std::to_string(k) + ".f32");
        EXPECT(B.integrate(pts.data(), 3, pts.size() / 3, identity) == 0);
    }
    for (int r = 0; r + 15 < argc; ++r) {
        dsi::MapCompareOptions o{};
        o.min_points_a = o.min_windows_a = o.min_points_b = o.min_windows_b = 1;
        o.radius = std::atof(a[15 + r]);
        o.n_bins = n_bins;
        const dsi::MapFScore f = dsi::map_f_score(A, B, o);
        EXPECT(f.est.info.n_cells == A.count() && f.gt.info.n_cells == B.count());
        EXPECT(f.est.mean() > 0.0 && f.est.mean() < o.radius && f.gt.mean() > 0.0 && f.gt.mean() < o.radius);
        // map_f_score compared A against B, then B against A: each map holds the distances of its own direction
        dump(dir + "/cmp_ab_" + std::to_string(r), A, f.est);
        dump(dir + "/cmp_ba_" + std::to_string(r), B, f.gt);
        std::vector<double> curves;
        for (const auto* v : {&f.thresholds, &f.precision, &f.recall, &f.f1}) curves.insert(curves.end(), v->begin(), v->end());
        EXPECT(curves.size() == 4 * (size_t)n_bins);
        write(dir + "/f_" + std::to_string(r) + ".f64", curves.data(), curves.size() * sizeof(double));
        std::printf("radius %g: precision %.2f %%, recall %.2f %%, f1 %.2f\n", o.radius, f.precision.back(), f.recall.back(), f.f1.back());
    }
    // a change to the second map leaves the first one's distances standing; a change to the first does not
    {
        dsi::MapCompareOptions o{};
        o.min_points_a = o.min_windows_a = o.min_points_b = o.min_windows_b = 1;
        o.radius = leaf_b;
        o.n_bins = n_bins;
        const dsi::MapCompareResult r = A.compare(B, o);
        const float p[3] = {0.f, 0.f, 1.f};
        dsi::WorldMap C(ctx, leaf_b, 8);
        C.integrate(p, 3, 1, identity);
        const dsi::MapDistances before = A.fetchDistances();
        EXPECT(before.size() == r.info.n_cells);
        A.integrate(p, 3, 1, identity);
        EXPECT(refused([&] { A.fetchDistances(); }, DSI_ERR_INVALID));
        o.radius = 4.0 * leaf_b;  // reach 4
        EXPECT(refused([&] { A.compare(B, o); }, DSI_ERR_INVALID));
        o.radius = leaf_b;
        o.n_bins = 0;
        EXPECT(refused([&] { A.compare(B, o); }, DSI_ERR_INVALID));
        dsi::Context other(0);
        dsi::WorldMap foreign(other, leaf_b, 8);
        o.n_bins = n_bins;
        EXPECT(refused([&] { A.compare(foreign, o); }, DSI_ERR_CONTEXT));
    }
    // a depth image into a map
    {
        const auto depth = read<float>(dir + "/depth.f32");
        const auto mask = read<uint8_t>(dir + "/mask.u8");
        const auto T = read<double>(dir + "/T_w_c.f64");
        EXPECT(depth.size() == (size_t)width * height && mask.size() == depth.size() && T.size() == 12);
        std::array<double, 12> T_w_c;
        std::memcpy(T_w_c.data(), T.data(), sizeof T_w_c);
        dsi::WorldMap D(ctx, leaf_a, 8);
        uint64_t rejected = 99;
        const uint64_t n = D.integrateDepth(depth.data(), mask.data(), width, height, fx, fy, cx, cy, min_depth, max_depth, T_w_c, &rejected);
        const dsi_map_info_t info = D.info();
        EXPECT(info.calls == 1 && info.accepted + info.rejected == n && info.rejected == rejected);
        const dsi::WorldMapCells cells = D.extract();
        write(dir + "/depth_cells.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
        write(dir + "/depth_cells.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
        write(dir + "/depth_cells.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
        write(dir + "/depth_cells.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
        const uint64_t iv[2] = {n, rejected};
        write(dir + "/depth_info.u64", iv, sizeof iv);
        EXPECT(refused([&] { D.integrateDepth(depth.data(), nullptr, width, height, 0.0, fy, cx, cy, min_depth, max_depth, T_w_c); },
                       DSI_ERR_INVALID));
        // through a projector that copies its input: the same map again
        const double Q[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, K[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1};
        dsi::GroundTruthProjector proj(ctx, width, height, Q, Q, K);
        dsi::Image<float> clean(height, width), held;
        for (size_t i = 0; i < depth.size(); ++i) clean.data[i] = std::isfinite(depth[i]) && depth[i] > 0.f ? depth[i] : 0.f;
        proj.project(clean);
        proj.fetch(held);
        dsi::WorldMap G(ctx, leaf_a, 8), H(ctx, leaf_a, 8);
        const uint64_t ng = G.integrateGroundTruth(proj, fx, fy, cx, cy, min_depth, max_depth, T_w_c);
        const uint64_t nh = H.integrateDepth(held.data.data(), nullptr, width, height, fx, fy, cx, cy, min_depth, max_depth, T_w_c);
        EXPECT(ng == nh && ng > 0);
        const dsi::WorldMapCells g = G.extract(), h = H.extract();
        EXPECT(g.keys == h.keys && g.n == h.n && g.windows == h.windows && g.size() > 0 &&
               std::memcmp(g.xyz.data(), h.xyz.data(), g.xyz.size() * sizeof(float)) == 0);
        std::printf("depth image: %llu pixels integrated, %zu cells\n", (unsigned long long)n, cells.size());
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 16) {
        std::fprintf(stderr,
                     "usage: %s DIR leaf_a n_calls_a leaf_b n_calls_b n_bins width height fx fy cx cy min_depth max_depth radius...\n",
                     argv[0]);
        return 2;
    }
    try {
        run(argc, argv);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
