// dsi::WorldMap::prune / classifyPrune / fetchPruneReasons on the hand cases of tests/map_prune_reference.py.  Run by
// tests/test_gpu_map_prune_cpp.py, which writes the cases this program reads and compares the files it writes with the
// numpy restatement.
//   test_map_prune DIR n_cases
// reads  DIR/case_<i>.opts.f64 = leaf, n_calls, min_points, min_windows, max_age (-1: off), use_box, lo[3], hi[3], reach,
//        min_neighbors (14 doubles) and DIR/case_<i>_<k>.f32 (N x 3 floats per call, integrated with the identity pose)
// writes DIR/case_<i>.{keys.u64,reason.u8} (the dry run's verdicts), DIR/case_<i>.info.u64 = n_cells, n_kept, n_removed[5],
//        capacity of the dry run, then the same eight of the prune (shrink = 1), and DIR/case_<i>.cells.{keys.u64,n.u32,
//        windows.u32,xyz.f32}: the pruned map
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

void put(std::vector<uint64_t>& v, const dsi::MapPruneInfo& i)
{
    v.push_back(i.n_cells);
    v.push_back(i.n_kept);
    for (int r = 0; r < 5; ++r) v.push_back(i.n_removed[r]);
    v.push_back(i.capacity);
}

int run(char** a)
{
    const std::string dir = a[1];
    const int n_cases = std::atoi(a[2]);
    dsi::Context ctx(0);
    const std::array<double, 12> identity = dsi::pose_matrix(dsi::Transformation());
    for (int c = 0; c < n_cases; ++c) {
        const std::string base = dir + "/case_" + std::to_string(c);
        const auto o = read<double>(base + ".opts.f64");
        EXPECT(o.size() == 14);
        dsi::WorldMap map(ctx, o[0], 8);
        EXPECT(refused([&] { map.fetchPruneReasons(); }, DSI_ERR_INVALID));  // nothing classified yet
        for (int k = 0; k < (int)o[1]; ++k) {
            const auto pts = read<float>(base + "_" + std::to_string(k) + ".f32");
            EXPECT(map.integrate(pts.data(), 3, pts.size() / 3, identity) == 0);
        }
        dsi::MapPruneOptions opts;
        {  // the defaults switch every criterion off
            const dsi::MapPruneInfo none = map.classifyPrune(opts);
            EXPECT(none.n_kept == none.n_cells && none.n_cells == map.count());
        }
        opts.min_points = (uint32_t)o[2];
        opts.min_windows = (uint32_t)o[3];
        opts.max_age = (int64_t)o[4];
        if (o[5] != 0.0) opts.box({o[6], o[7], o[8]}, {o[9], o[10], o[11]});
        opts.reach = (int32_t)o[12];
        opts.min_neighbors = (uint32_t)o[13];
        std::vector<uint64_t> info;
        const dsi_map_info_t before = map.info();
        const dsi::MapPruneInfo dry = map.classifyPrune(opts);
        put(info, dry);
        EXPECT(dry.capacity == before.capacity && map.info().occupied == before.occupied);
        const dsi::MapPruneReasons verdicts = map.fetchPruneReasons();
        EXPECT(verdicts.size() == dry.n_cells);
        write(base + ".keys.u64", verdicts.keys.data(), verdicts.keys.size() * sizeof(uint64_t));
        write(base + ".reason.u8", verdicts.reason.data(), verdicts.reason.size());
        opts.shrink = 1;
        const dsi::MapPruneInfo done = map.prune(opts);
        put(info, done);
        write(base + ".info.u64", info.data(), info.size() * sizeof(uint64_t));
        const dsi_map_info_t after = map.info();
        EXPECT(after.occupied == done.n_kept && after.capacity == done.capacity && after.calls == before.calls &&
               after.accepted == before.accepted && after.growths == before.growths);
        EXPECT(refused([&] { map.fetchPruneReasons(); }, DSI_ERR_INVALID));  // the prune invalidated the dry run
        const dsi::WorldMapCells cells = map.extract();
        write(base + ".cells.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
        write(base + ".cells.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
        write(base + ".cells.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
        write(base + ".cells.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
        opts.reach = 3;
        EXPECT(refused([&] { map.prune(opts); }, DSI_ERR_INVALID));
        std::printf("case %d: %llu cells, %llu kept\n", c, (unsigned long long)dry.n_cells, (unsigned long long)dry.n_kept);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s DIR n_cases\n", argv[0]);
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
