// dsi::WorldMap::components / fetchComponents / listComponents / selectComponents / pruneComponents on the random scene of
// tests/map_prune_reference.py.  Run by tests/test_gpu_map_components_cpp.py, which writes the calls this program reads and
// compares the files it writes with the restatement of tests/map_components_reference.py.
//   test_map_components DIR
// reads  DIR/opts.f64 = leaf, n_calls, min_points, min_windows, connectivity, min_cells, min_component_points, keep_largest
//        (8 doubles) and DIR/call_<k>.f32 (N x 3 floats per call, integrated with the identity pose)
// writes DIR/info.u64 = the labelling's seven counts, then n_cells, n_kept, n_removed[4], n_components_kept, capacity of the
//        dry run, then the same eight of the prune (shrink = 1); DIR/rows.{keys,labels}.u64 and DIR/rows.reason.u8 (one row
//        per labelled cell, after the dry run), DIR/list.{labels,cells,points}.u64 (one row per component) and
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

void put(std::vector<uint64_t>& v, const dsi::MapComponentsSelectInfo& i)
{
    v.push_back(i.n_cells);
    v.push_back(i.n_kept);
    for (int r = 0; r < 4; ++r) v.push_back(i.n_removed[r]);
    v.push_back(i.n_components_kept);
    v.push_back(i.capacity);
}

int run(char** a)
{
    const std::string dir = a[1];
    dsi::Context ctx(0);
    const std::array<double, 12> identity = dsi::pose_matrix(dsi::Transformation());
    const auto o = read<double>(dir + "/opts.f64");
    EXPECT(o.size() == 8);
    dsi::WorldMap map(ctx, o[0], 8);
    EXPECT(refused([&] { map.fetchComponents(); }, DSI_ERR_INVALID));  // nothing labelled yet
    EXPECT(refused([&] { map.listComponents(); }, DSI_ERR_INVALID));
    EXPECT(refused([&] { map.selectComponents(); }, DSI_ERR_INVALID));
    EXPECT(refused([&] { map.pruneComponents(); }, DSI_ERR_INVALID));
    for (int k = 0; k < (int)o[1]; ++k) {
        const auto pts = read<float>(dir + "/call_" + std::to_string(k) + ".f32");
        (void)map.integrate(pts.data(), 3, pts.size() / 3, identity);
    }
    {  // the defaults label every cell at connectivity 26 and keep every labelled cell
        const dsi::MapComponentsInfo all = map.components();
        EXPECT(all.n_cells == map.count() && all.n_unlabelled == 0);
        const dsi::MapComponentsSelectInfo none = map.selectComponents();
        EXPECT(none.n_kept == none.n_cells && none.n_components_kept == all.n_components);
    }
    dsi::MapComponentsOptions opts;
    opts.min_points = (uint32_t)o[2];
    opts.min_windows = (uint32_t)o[3];
    opts.connectivity = (int32_t)o[4];
    const dsi_map_info_t before = map.info();
    const dsi::MapComponentsInfo lab = map.components(opts);
    EXPECT(refused([&] { map.fetchComponents(true); }, DSI_ERR_INVALID));  // no selection on this labelling yet
    std::vector<uint64_t> info = {lab.n_cells,       lab.n_unlabelled,  lab.n_components,  lab.n_singletons,
                                  lab.largest_label, lab.largest_cells, lab.largest_points};
    const dsi::MapComponentList list = map.listComponents();
    EXPECT(list.size() == lab.n_components);
    write(dir + "/list.labels.u64", list.labels.data(), list.size() * sizeof(uint64_t));
    write(dir + "/list.cells.u64", list.cells.data(), list.size() * sizeof(uint64_t));
    write(dir + "/list.points.u64", list.points.data(), list.size() * sizeof(uint64_t));
    dsi::MapComponentsSelection sel;
    sel.min_cells = (uint64_t)o[5];
    sel.min_component_points = (uint64_t)o[6];
    sel.keep_largest = (int32_t)o[7];
    const dsi::MapComponentsSelectInfo dry = map.selectComponents(sel);
    put(info, dry);
    EXPECT(dry.capacity == before.capacity && map.info().occupied == before.occupied);
    const dsi::MapComponentLabels rows = map.fetchComponents(true);
    EXPECT(rows.size() == lab.n_cells && rows.reason.size() == rows.size());
    write(dir + "/rows.keys.u64", rows.keys.data(), rows.size() * sizeof(uint64_t));
    write(dir + "/rows.labels.u64", rows.labels.data(), rows.size() * sizeof(uint64_t));
    write(dir + "/rows.reason.u8", rows.reason.data(), rows.size());
    sel.shrink = 1;
    const dsi::MapComponentsSelectInfo done = map.pruneComponents(sel);
    put(info, done);
    write(dir + "/info.u64", info.data(), info.size() * sizeof(uint64_t));
    const dsi_map_info_t after = map.info();
    EXPECT(after.occupied == done.n_kept && after.capacity == done.capacity && after.calls == before.calls &&
           after.accepted == before.accepted && after.growths == before.growths);
    EXPECT(refused([&] { map.fetchComponents(); }, DSI_ERR_INVALID));  // the prune invalidated the labelling
    EXPECT(refused([&] { map.pruneComponents(sel); }, DSI_ERR_INVALID));
    const dsi::WorldMapCells cells = map.extract();
    write(dir + "/cells.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
    write(dir + "/cells.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
    write(dir + "/cells.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
    write(dir + "/cells.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
    opts.connectivity = 27;
    EXPECT(refused([&] { map.components(opts); }, DSI_ERR_INVALID));
    sel.keep_largest = 17;
    EXPECT(refused([&] { map.selectComponents(sel); }, DSI_ERR_INVALID));
    std::printf("%llu cells in %llu components, %llu kept in %llu\n", (unsigned long long)lab.n_cells, (unsigned long long)lab.n_components,
                (unsigned long long)dry.n_kept, (unsigned long long)dry.n_components_kept);
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
