// dsi::WorldMap::pca / fetchPca / pruneShapes and dsi::pca_solve on the scene of tests/map_pca_reference.py.  Run by
// tests/test_gpu_map_pca_cpp.py, which writes the calls this program reads and compares the files it writes with the Python
// rows and the restatement.
//   test_map_pca DIR
// reads  DIR/opts.f64 = leaf, n_calls, min_points, min_windows, k, min_found, radius, viewpoint[3], keep_labels (11 doubles)
//        and DIR/call_<k>.f32 (N x 3 floats per call, integrated with the identity pose)
// writes DIR/rows.{keys.u64,normal.f32,tangent.f32,eval.f32,members.u16,label.u8,flags.u8,moments.i64}: fetchPca's rows;
//        DIR/info.u64 = the pass's n_cells, n_unqueried, n_sparse, n_label[3], n_normal_determined, n_tangent_determined,
//        sum_members, reach, then n_cells, n_kept, n_removed[3], capacity of the prune (shrink = 1);
//        DIR/cells.{keys.u64,n.u32,windows.u32,xyz.f32}: the pruned map
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
    EXPECT(o.size() == 11);
    dsi::WorldMap map(ctx, o[0], 8);
    EXPECT(refused([&] { map.pruneShapes(); }, DSI_ERR_INVALID));  // no pass yet
    EXPECT(refused([&] { map.fetchPca(); }, DSI_ERR_INVALID));
    for (int k = 0; k < (int)o[1]; ++k) {
        const auto pts = read<float>(dir + "/call_" + std::to_string(k) + ".f32");
        (void)map.integrate(pts.data(), 3, pts.size() / 3, identity);
    }
    dsi::MapPcaOptions opts(o[6], (int)o[4]);
    opts.min_points = (uint32_t)o[2];
    opts.min_windows = (uint32_t)o[3];
    opts.min_found = (int32_t)o[5];
    opts.keep_moments = 1;
    opts.lookAt(o[7], o[8], o[9]);
    const dsi_map_info_t before = map.info();
    const dsi::MapPcaInfo q = map.pca(opts);
    EXPECT(q.n_cells + q.n_unqueried == before.occupied && q.n_sparse + q.n_label[0] + q.n_label[1] + q.n_label[2] == q.n_cells);
    const dsi::MapShapes rows = map.fetchPca();
    EXPECT(rows.size() == q.n_cells && rows.normal.size() == 3 * rows.size() && rows.moments.size() == 9 * rows.size());
    write(dir + "/rows.keys.u64", rows.keys.data(), rows.keys.size() * sizeof(uint64_t));
    write(dir + "/rows.normal.f32", rows.normal.data(), rows.normal.size() * sizeof(float));
    write(dir + "/rows.tangent.f32", rows.tangent.data(), rows.tangent.size() * sizeof(float));
    write(dir + "/rows.eval.f32", rows.eval.data(), rows.eval.size() * sizeof(float));
    write(dir + "/rows.members.u16", rows.members.data(), rows.members.size() * sizeof(uint16_t));
    write(dir + "/rows.label.u8", rows.label.data(), rows.label.size());
    write(dir + "/rows.flags.u8", rows.flags.data(), rows.flags.size());
    write(dir + "/rows.moments.i64", rows.moments.data(), rows.moments.size() * sizeof(int64_t));
    // every solved row comes back from its moments through dsi::pca_solve (the canonical sign: compared up to the orientation)
    const dsi::WorldMapCells all = map.extract(opts.min_points, opts.min_windows, false);  // (fetchPca's order)
    EXPECT(all.keys.size() == rows.size());
    size_t solved = 0;
    for (size_t i = 0; i < rows.size() && i < all.keys.size(); ++i) {
        if (!rows.label[i]) continue;
        const double p[3] = {all.xyz[3 * i], all.xyz[3 * i + 1], all.xyz[3 * i + 2]};
        const dsi::PcaRow r = dsi::pca_solve(rows.members[i], &rows.moments[9 * i], &rows.moments[9 * i + 3], o[0] / 1024.0, opts.viewpoint, p);
        EXPECT(all.keys[i] == rows.keys[i] && r.label == rows.label[i] && r.flags == rows.flags[i]);
        EXPECT(std::memcmp(r.normal, &rows.normal[3 * i], sizeof r.normal) == 0 && std::memcmp(r.tangent, &rows.tangent[3 * i], sizeof r.tangent) == 0 &&
               std::memcmp(r.eval, &rows.eval[3 * i], sizeof r.eval) == 0);
        ++solved;
    }
    EXPECT(solved == q.n_cells - q.n_sparse);
    std::vector<uint64_t> info = {q.n_cells, q.n_unqueried, q.n_sparse, q.n_label[0], q.n_label[1], q.n_label[2], q.n_normal_determined,
                                  q.n_tangent_determined, q.sum_members, (uint64_t)q.reach};
    const dsi::MapPcaSelectInfo done = map.pruneShapes(dsi::MapPcaSelection((uint32_t)o[10], true, true));
    info.push_back(done.n_cells);
    info.push_back(done.n_kept);
    for (int r = 0; r < 3; ++r) info.push_back(done.n_removed[r]);
    info.push_back(done.capacity);
    write(dir + "/info.u64", info.data(), info.size() * sizeof(uint64_t));
    const dsi_map_info_t after = map.info();
    EXPECT(after.occupied == done.n_kept && after.capacity == done.capacity && after.calls == before.calls &&
           after.accepted == before.accepted && after.growths == before.growths);
    EXPECT(refused([&] { map.pruneShapes(); }, DSI_ERR_INVALID));  // the prune invalidated the pass
    EXPECT(refused([&] { map.fetchPca(); }, DSI_ERR_INVALID));
    const dsi::WorldMapCells cells = map.extract();
    write(dir + "/cells.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
    write(dir + "/cells.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
    write(dir + "/cells.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
    write(dir + "/cells.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
    opts.k = 17;
    EXPECT(refused([&] { map.pca(opts); }, DSI_ERR_INVALID));
    opts.k = 4;
    EXPECT(refused([&] { map.pruneShapes(dsi::MapPcaSelection(0)); }, DSI_ERR_INVALID));
    const int64_t s[3] = {20, 0, 0}, ss[6] = {100, 0, 0, 100, 0, 100};
    EXPECT(refused([&] { dsi::pca_solve(3, s, ss, 1e-3); }, DSI_ERR_INVALID));  // m ss < s^2
    std::printf("%llu queries, %llu sparse, %llu kept\n", (unsigned long long)q.n_cells, (unsigned long long)q.n_sparse,
                (unsigned long long)done.n_kept);
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
