// dsi::WorldMap::query / knn / pruneOutliers and dsi::knn_threshold on the sparse scene of tests/map_knn_reference.py.  Run by
// tests/test_gpu_map_knn_cpp.py, which writes the calls and the query points this program reads and compares the files it
// writes with the restatement.
//   test_map_knn DIR
// reads  DIR/opts.f64 = leaf, n_calls, min_points, min_windows, k, min_found, radius, std_mult (8 doubles),
//        DIR/call_<k>.f32 (N x 3 floats per call, integrated with the identity pose) and DIR/points.f32 (M x 4 floats)
// writes DIR/query.keys.u64, DIR/query.dist.f32 (M x k) and DIR/query.found.u8 (M); DIR/info.u64 = the self query's n_cells,
//        n_unqueried, n_scored, n_isolated, sum_q, sum_q2 low and high, reach, then T_q of dsi::knn_threshold, then n_cells,
//        n_kept, n_removed[3], T_q, capacity of the prune (shrink = 1); DIR/threshold.f64 = mu and sigma of dsi::knn_threshold,
//        then of the prune; DIR/cells.{keys.u64,n.u32,windows.u32,xyz.f32}: the pruned map
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

int run(char** a)
{
    const std::string dir = a[1];
    dsi::Context ctx(0);
    const std::array<double, 12> identity = dsi::pose_matrix(dsi::Transformation());
    const auto o = read<double>(dir + "/opts.f64");
    EXPECT(o.size() == 8);
    dsi::WorldMap map(ctx, o[0], 8);
    EXPECT(refused([&] { map.pruneOutliers(); }, DSI_ERR_INVALID));  // no self query yet
    for (int k = 0; k < (int)o[1]; ++k) {
        const auto pts = read<float>(dir + "/call_" + std::to_string(k) + ".f32");
        (void)map.integrate(pts.data(), 3, pts.size() / 3, identity);
    }
    dsi::MapKnnOptions opts(o[6], (int)o[4]);
    opts.min_points = (uint32_t)o[2];
    opts.min_windows = (uint32_t)o[3];
    opts.min_found = (int32_t)o[5];
    const dsi_map_info_t before = map.info();
    const auto points = read<float>(dir + "/points.f32");
    const dsi::MapNeighbours nb = map.query(points.data(), 4, points.size() / 4, opts);
    EXPECT(nb.k == opts.k && nb.size() == points.size() / 4 && nb.keys.size() == nb.size() * (size_t)nb.k && nb.dist.size() == nb.keys.size());
    write(dir + "/query.keys.u64", nb.keys.data(), nb.keys.size() * sizeof(uint64_t));
    write(dir + "/query.dist.f32", nb.dist.data(), nb.dist.size() * sizeof(float));
    write(dir + "/query.found.u8", nb.found.data(), nb.found.size());
    EXPECT(map.query(nullptr, 3, 0, opts).size() == 0);  // no points
    const dsi::MapKnnInfo q = map.knn(opts);
    EXPECT(q.n_cells + q.n_unqueried == before.occupied && q.n_scored + q.n_isolated == q.n_cells);
    const dsi::MapKnnThreshold thr = dsi::knn_threshold(q, o[7]);
    const dsi::MapKnnThreshold same = dsi::knn_threshold(q.n_scored, q.sum_q, q.sum_q2, o[7]);
    EXPECT(thr.mu == same.mu && thr.sigma == same.sigma && thr.T_q == same.T_q);
    std::vector<uint64_t> info = {q.n_cells, q.n_unqueried, q.n_scored, q.n_isolated, q.sum_q, q.sum_q2[0], q.sum_q2[1], (uint64_t)q.reach,
                                  thr.T_q};
    const dsi::MapKnnSelectInfo done = map.pruneOutliers(dsi::MapKnnSelection(o[7], true));
    EXPECT(done.T_q == thr.T_q && done.mu == thr.mu && done.sigma == thr.sigma);  // one routine behind both
    info.push_back(done.n_cells);
    info.push_back(done.n_kept);
    for (int r = 0; r < 3; ++r) info.push_back(done.n_removed[r]);
    info.push_back(done.T_q);
    info.push_back(done.capacity);
    write(dir + "/info.u64", info.data(), info.size() * sizeof(uint64_t));
    const double t[4] = {thr.mu, thr.sigma, done.mu, done.sigma};
    write(dir + "/threshold.f64", t, sizeof t);
    const dsi_map_info_t after = map.info();
    EXPECT(after.occupied == done.n_kept && after.capacity == done.capacity && after.calls == before.calls &&
           after.accepted == before.accepted && after.growths == before.growths);
    EXPECT(refused([&] { map.pruneOutliers(); }, DSI_ERR_INVALID));  // the prune invalidated the self query
    const dsi::WorldMapCells cells = map.extract();
    write(dir + "/cells.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
    write(dir + "/cells.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
    write(dir + "/cells.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
    write(dir + "/cells.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
    opts.k = 17;
    EXPECT(refused([&] { map.knn(opts); }, DSI_ERR_INVALID));
    EXPECT(refused([&] { map.query(points.data(), 4, 1, opts); }, DSI_ERR_INVALID));
    const uint64_t no_cells[2] = {1, 0};
    EXPECT(refused([&] { dsi::knn_threshold(2, 4, no_cells, 1.0); }, DSI_ERR_INVALID));  // V < 0
    std::printf("%llu queries, %llu scored, T_q %llu, %llu kept\n", (unsigned long long)q.n_cells, (unsigned long long)q.n_scored,
                (unsigned long long)thr.T_q, (unsigned long long)done.n_kept);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    try {
        run(argv);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
