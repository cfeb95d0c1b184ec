// dsi::WorldMap::merge / exportState / importState on two cuts of the scene of tests/map_prune_reference.py.  Run by
// tests/test_gpu_map_merge_cpp.py, which writes the calls this program reads and compares the files it writes with the
// numpy restatement (tests/map_merge_reference.py).
//   test_map_merge DIR leaf n_calls cut [cut ...]
// reads  DIR/call_<k>.f32 (N x 3 floats per call, integrated with the identity pose)
// writes per cut c, DIR/cut_<c>.merged.* = the state of the map of calls [0, c) after merge(map of calls [c, n_calls)),
//        DIR/cut_<c>.imported.* = the state of an empty map after importState of that state and then of nothing else,
//        each as {keys.u64, n.u32, S.u64, windows.u32, stamp.u32, header.f64 = leaf, calls, accepted, rejected}, and
//        DIR/cut_<c>.info.u64 = n_src_cells, n_new, n_common, capacity, growths of the merge, then of the import
#include <cstdio>
#include <cstdlib>
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

std::vector<float> read(const std::string& path)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot read " + path);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> v((size_t)bytes / sizeof(float));
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

void dump(const std::string& base, const dsi::MapState& s)
{
    write(base + ".keys.u64", s.keys.data(), s.keys.size() * sizeof(uint64_t));
    write(base + ".n.u32", s.n.data(), s.n.size() * sizeof(uint32_t));
    write(base + ".S.u64", s.S.data(), s.S.size() * sizeof(uint64_t));
    write(base + ".windows.u32", s.windows.data(), s.windows.size() * sizeof(uint32_t));
    write(base + ".stamp.u32", s.stamp.data(), s.stamp.size() * sizeof(uint32_t));
    const double header[4] = {s.leaf, (double)s.calls, (double)s.accepted, (double)s.rejected};
    write(base + ".header.f64", header, sizeof header);
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

void put(std::vector<uint64_t>& v, const dsi::MapMergeInfo& i)
{
    v.push_back(i.n_src_cells);
    v.push_back(i.n_new);
    v.push_back(i.n_common);
    v.push_back(i.capacity);
    v.push_back(i.growths);
}

int run(int argc, char** a)
{
    const std::string dir = a[1];
    const double leaf = std::atof(a[2]);
    const int n_calls = std::atoi(a[3]);
    dsi::Context ctx(0), other(0);
    const std::array<double, 12> identity = dsi::pose_matrix(dsi::Transformation());
    std::vector<std::vector<float>> calls;
    for (int k = 0; k < n_calls; ++k) calls.push_back(read(dir + "/call_" + std::to_string(k) + ".f32"));
    for (int i = 4; i < argc; ++i) {
        const int cut = std::atoi(a[i]);
        const std::string base = dir + "/cut_" + std::to_string(cut);
        dsi::WorldMap first(ctx, leaf, 8), rest(ctx, leaf, 10);
        for (int k = 0; k < n_calls; ++k)
            EXPECT((k < cut ? first : rest).integrate(calls[(size_t)k].data(), 3, calls[(size_t)k].size() / 3, identity) == 0);
        const dsi::MapState rest_before = rest.exportState();
        EXPECT(rest_before.size() == rest.count(0, 0) && rest_before.S.size() == 3 * rest_before.size());
        std::vector<uint64_t> info;
        const dsi_map_info_t before = first.info();
        const dsi::MapMergeInfo m = first.merge(rest);
        put(info, m);
        const dsi_map_info_t after = first.info();
        EXPECT(m.n_src_cells == rest_before.size() && m.n_new + m.n_common == m.n_src_cells);
        EXPECT(after.occupied == before.occupied + m.n_new && after.capacity == m.capacity && after.growths == before.growths + m.growths);
        EXPECT(after.calls == (uint64_t)n_calls && after.accepted == before.accepted + rest_before.accepted);
        const dsi::MapState rest_after = rest.exportState();  // the source is unchanged
        EXPECT(rest_after.keys == rest_before.keys && rest_after.S == rest_before.S && rest_after.stamp == rest_before.stamp &&
               rest_after.calls == rest_before.calls);
        const dsi::MapState merged = first.exportState();
        dump(base + ".merged", merged);
        // the state restored on another context, from the table's order
        dsi::WorldMap back(other, leaf, 8);
        const dsi::MapMergeInfo r = back.importState(first.exportState(false));
        put(info, r);
        EXPECT(r.n_new == merged.size() && r.n_common == 0 && back.info().calls == merged.calls);
        dump(base + ".imported", back.exportState());
        write(base + ".info.u64", info.data(), info.size() * sizeof(uint64_t));
        // refusals leave the map as it is
        EXPECT(refused([&] { first.merge(first); }, DSI_ERR_INVALID));
        EXPECT(refused([&] { back.merge(first); }, DSI_ERR_CONTEXT));
        dsi::MapState bad = merged;
        if (!bad.keys.empty()) {
            bad.keys[0] = 0;
            EXPECT(refused([&] { back.importState(bad); }, DSI_ERR_INVALID));
            bad = merged;
            bad.stamp.pop_back();
            EXPECT(refused([&] { back.importState(bad); }, DSI_ERR_INVALID));
        }
        const dsi::MapState still = back.exportState();
        EXPECT(still.keys == merged.keys && still.n == merged.n && still.S == merged.S && still.windows == merged.windows &&
               still.stamp == merged.stamp && still.calls == merged.calls && still.accepted == merged.accepted);
        std::printf("cut %d: %llu + %llu new cells, %llu common\n", cut, (unsigned long long)before.occupied, (unsigned long long)m.n_new,
                    (unsigned long long)m.n_common);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s DIR leaf n_calls cut [cut ...]\n", argv[0]);
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
