// dsi::WorldMap::observe / fetchVisibility / selectCarved / pruneCarved on the scene of tests/map_pca_reference.py with the views
// of tests/map_visibility_reference.py.  Run by tests/test_gpu_map_visibility_cpp.py, which writes the calls and views this
// program reads and compares the files it writes with the Python rows and the restatement.
//   test_map_visibility DIR
// reads  DIR/opts.f64 = leaf, n_calls, n_views, min_through, agree_weight (5 doubles),
//        DIR/call_<k>.f32 (N x 3 floats per call, integrated with the identity pose) and per view DIR/view_<k>.obs.f64 =
//        width, height, window, fx, fy, cx, cy, min_depth, max_depth, abs_tol, rel_tol, T_v_w[12] (23 doubles),
//        DIR/view_<k>.depth.f32 and DIR/view_<k>.mask.u8 (empty: no mask)
// writes DIR/rows.{keys.u64,seen.u32,agree.u32,through.u32,reason.u8}: fetchVisibility's rows after the selection;
//        DIR/info.u64 = per view n_cells, n_clipped, n_outside, n_unseen, n_agree, n_through, n_behind, n_valid_pixels, views,
//        then n_cells, n_kept, n_removed, capacity of the selection and of the prune (shrink = 1);
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
    EXPECT(o.size() == 5);
    dsi::WorldMap map(ctx, o[0], 8);
    EXPECT(refused([&] { map.fetchVisibility(); }, DSI_ERR_INVALID));  // no observation yet
    EXPECT(refused([&] { map.selectCarved(); }, DSI_ERR_INVALID));
    EXPECT(refused([&] { map.pruneCarved(); }, DSI_ERR_INVALID));
    for (int k = 0; k < (int)o[1]; ++k) {
        const auto pts = read<float>(dir + "/call_" + std::to_string(k) + ".f32");
        (void)map.integrate(pts.data(), 3, pts.size() / 3, identity);
    }
    const dsi_map_info_t before = map.info();
    std::vector<uint64_t> info;
    for (int k = 0; k < (int)o[2]; ++k) {
        const std::string stem = dir + "/view_" + std::to_string(k);
        const auto v = read<double>(stem + ".obs.f64");
        const auto depth = read<float>(stem + ".depth.f32");
        const auto mask = read<uint8_t>(stem + ".mask.u8");
        EXPECT(v.size() == 23 && depth.size() == (size_t)(v[0] * v[1]) && (mask.empty() || mask.size() == depth.size()));
        std::array<double, 12> T;
        std::copy(v.begin() + 11, v.end(), T.begin());
        const dsi::MapObservation obs((int)v[0], (int)v[1], v[3], v[4], v[5], v[6], v[7], v[8], T, (int)v[2], v[9], v[10]);
        const dsi::MapObserveInfo c = map.observe(depth.data(), mask.empty() ? nullptr : mask.data(), obs);
        EXPECT(c.n_cells == before.occupied && c.views == (uint64_t)k + 1 &&
               c.n_cells == c.n_clipped + c.n_outside + c.n_unseen + c.n_agree + c.n_through + c.n_behind);
        for (uint64_t x : {c.n_cells, c.n_clipped, c.n_outside, c.n_unseen, c.n_agree, c.n_through, c.n_behind, c.n_valid_pixels, c.views})
            info.push_back(x);
        if (k == 0) {  // a violated bound is refused and leaves the tally as it was
            dsi::MapObservation bad = obs;
            bad.window = 4;
            EXPECT(refused([&] { map.observe(depth.data(), nullptr, bad); }, DSI_ERR_INVALID));
            bad = obs;
            bad.abs_tol = -1.0;
            EXPECT(refused([&] { map.observe(depth.data(), nullptr, bad); }, DSI_ERR_INVALID));
        }
    }
    EXPECT(map.fetchVisibility().reason.empty());  // no selection yet
    const dsi::MapVisibilitySelection sel((uint32_t)o[3], (uint32_t)o[4], true);
    const dsi::MapVisibilitySelectInfo dry = map.selectCarved(sel);
    const dsi::MapVisibility rows = map.fetchVisibility();
    EXPECT(rows.size() == before.occupied && rows.seen.size() == rows.size() && rows.reason.size() == rows.size());
    const dsi::MapVisibility unsorted = map.fetchVisibility(false);
    const dsi::WorldMapCells all = map.extract(1, 1, false);  // (fetchVisibility's order)
    EXPECT(unsorted.keys == all.keys && unsorted.keys != rows.keys);
    write(dir + "/rows.keys.u64", rows.keys.data(), rows.keys.size() * sizeof(uint64_t));
    write(dir + "/rows.seen.u32", rows.seen.data(), rows.seen.size() * sizeof(uint32_t));
    write(dir + "/rows.agree.u32", rows.agree.data(), rows.agree.size() * sizeof(uint32_t));
    write(dir + "/rows.through.u32", rows.through.data(), rows.through.size() * sizeof(uint32_t));
    write(dir + "/rows.reason.u8", rows.reason.data(), rows.reason.size());
    const dsi_map_info_t same = map.info();
    EXPECT(same.occupied == before.occupied && same.capacity == before.capacity && dry.capacity == before.capacity);
    const dsi::MapVisibilitySelectInfo done = map.pruneCarved(sel);
    for (const dsi::MapVisibilitySelectInfo& s : {dry, done})
        for (uint64_t x : {s.n_cells, s.n_kept, s.n_removed, s.capacity}) info.push_back(x);
    write(dir + "/info.u64", info.data(), info.size() * sizeof(uint64_t));
    const dsi_map_info_t after = map.info();
    EXPECT(after.occupied == done.n_kept && after.capacity == done.capacity && after.calls == before.calls &&
           after.accepted == before.accepted && after.growths == before.growths);
    EXPECT(refused([&] { map.pruneCarved(); }, DSI_ERR_INVALID));  // the prune ended the tally
    EXPECT(refused([&] { map.fetchVisibility(); }, DSI_ERR_INVALID));
    const dsi::WorldMapCells cells = map.extract();
    write(dir + "/cells.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
    write(dir + "/cells.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
    write(dir + "/cells.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
    write(dir + "/cells.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
    EXPECT(refused([&] { map.selectCarved(dsi::MapVisibilitySelection(0)); }, DSI_ERR_INVALID));
    map.clearVisibility();
    EXPECT(refused([&] { map.fetchVisibility(); }, DSI_ERR_INVALID));
    std::printf("%llu cells, %llu carved, %llu kept\n", (unsigned long long)done.n_cells, (unsigned long long)done.n_removed,
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
