// dsi::WorldMap through dsi::full_sequence_depth_maps: every window's cloud goes into a world-frame map on the device.
// Run by tests/test_gpu_world_map_cpp.py, which writes the rig this program reads and compares the map it writes with the
// numpy restatement of the arithmetic (tests/world_map_reference.py) on the clouds it writes.
//   test_world_map DIR width height fx fy cx cy dimZ min_depth max_depth t0 t1 duration leaf radius min_neighbors
// reads  DIR/ev<c>_x.u16 ev<c>_y.u16 ev<c>_t.f64 traj<c>_t.f64 traj<c>_p.f64 (7 doubles per pose), c = 0, 1
// writes DIR/window_<k>.cloud.f32 (N x 4), window_<k>.T_rv_w.f64 (7), window_<k>.T_w_rv.f64 (12, row-major [R | t]), map.xyz.f32 map.n.u32 map.windows.u32 map.keys.u64
//        (by ascending key), map.info.u64 (occupied, calls, accepted, rejected)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dsi_engine.hpp"
#include "dsi_process.hpp"

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

std::vector<float> flat(const dsi::PointCloud& pc)
{
    std::vector<float> v;
    for (const auto& p : pc.points) v.insert(v.end(), {p.x, p.y, p.z, p.intensity});
    return v;
}

int run(char** a)
{
    const std::string dir = a[1];
    dsi::PinholeCameraModel cam;
    cam.width = std::atoi(a[2]);
    cam.height = std::atoi(a[3]);
    cam.fx = (float)std::atof(a[4]);
    cam.fy = (float)std::atof(a[5]);
    cam.cx = (float)std::atof(a[6]);
    cam.cy = (float)std::atof(a[7]);
    const EMVS::ShapeDSI shape(0, 0, std::atoi(a[8]), (float)std::atof(a[9]), (float)std::atof(a[10]), 0.f);
    const double t0 = std::atof(a[11]), t1 = std::atof(a[12]), duration = std::atof(a[13]), leaf = std::atof(a[14]);
    EMVS::OptionsDepthMap opts_depth_map;
    EMVS::OptionsPointCloud opts_pc;
    opts_pc.radius_search_ = (float)std::atof(a[15]);
    opts_pc.min_num_neighbors_ = std::atoi(a[16]);
    std::vector<dsi::Event> ev[2];
    LinearTrajectory::PoseMap poses[2];
    for (int c = 0; c < 2; ++c) {
        const std::string s = std::to_string(c);
        const auto x = read<uint16_t>(dir + "/ev" + s + "_x.u16"), y = read<uint16_t>(dir + "/ev" + s + "_y.u16");
        const auto t = read<double>(dir + "/ev" + s + "_t.f64");
        const auto tt = read<double>(dir + "/traj" + s + "_t.f64"), tp = read<double>(dir + "/traj" + s + "_p.f64");
        EXPECT(x.size() == y.size() && x.size() == t.size() && tp.size() == 7 * tt.size() && !tt.empty());
        ev[c].resize(x.size());
        for (size_t k = 0; k < x.size(); ++k) {
            ev[c][k].x = x[k];
            ev[c][k].y = y[k];
            ev[c][k].ts = t[k];
        }
        for (size_t k = 0; k < tt.size(); ++k) poses[c][tt[k]] = dsi::Transformation::from7(&tp[7 * k]);
    }
    const LinearTrajectory trajectory0(poses[0]), trajectory1(poses[1]);
    dsi::Context ctx(0);
    dsi::WorldMap map(ctx, leaf, 8);
    std::vector<std::vector<float>> clouds;
    const size_t nw = dsi::full_sequence_depth_maps(
        0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], t0, t1, duration, duration, /*forward_looking=*/true,
        /*fusion_method=*/2,
        [&](const dsi::WindowDepthMap& w) {
            clouds.push_back(flat(w.point_cloud));
            double T7[7];
            w.T_rv_w.to7(T7);
            const std::string base = dir + "/window_" + std::to_string(w.index);
            write(base + ".cloud.f32", clouds.back().data(), clouds.back().size() * sizeof(float));
            write(base + ".T_rv_w.f64", T7, sizeof T7);
            const std::array<double, 12> T_w_rv = dsi::invert_pose(w.T_rv_w);  // (what the stream integrated the window with)
            write(base + ".T_w_rv.f64", T_w_rv.data(), sizeof(double) * 12);
            EXPECT(map.info().calls == (uint64_t)w.index + 1);  // the window is in the map when it is delivered
        },
        2, 0.0, &opts_depth_map, nullptr, &opts_pc, &map);
    EXPECT(nw == clouds.size() && nw >= 3);
    // without the map the windows' clouds are the same
    size_t k = 0;
    dsi::full_sequence_depth_maps(
        0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], t0, t1, duration, duration, true, 2,
        [&](const dsi::WindowDepthMap& w) {
            const std::vector<float> c = flat(w.point_cloud);
            EXPECT(k < clouds.size() && c.size() == clouds[k].size() && std::memcmp(c.data(), clouds[k].data(), c.size() * sizeof(float)) == 0);
            ++k;
        },
        2, 0.0, &opts_depth_map, nullptr, &opts_pc);
    EXPECT(k == nw);
    const dsi::WorldMapCells cells = map.extract();
    const dsi_map_info_t info = map.info();
    size_t points = 0;
    for (const auto& c : clouds) points += c.size() / 4;
    EXPECT(cells.size() == info.occupied && cells.size() == map.count() && info.accepted + info.rejected == points && info.calls == nw);
    EXPECT(map.extract(1, 2).size() <= cells.size());
    // the host path on the same clouds and poses gives the same map
    dsi::WorldMap host(ctx, leaf, 16);
    for (size_t i = 0; i < clouds.size(); ++i) {
        const auto T7 = read<double>(dir + "/window_" + std::to_string(i) + ".T_rv_w.f64");
        host.integrate(clouds[i].data(), 4, clouds[i].size() / 4, dsi::invert_pose(dsi::Transformation::from7(T7.data())));
    }
    const dsi::WorldMapCells again = host.extract();
    EXPECT(again.keys == cells.keys && again.n == cells.n && again.windows == cells.windows &&
           again.xyz.size() == cells.xyz.size() && std::memcmp(again.xyz.data(), cells.xyz.data(), cells.xyz.size() * sizeof(float)) == 0);
    // the Alg. 2 stream: the time_camera output's clouds go into the map
    {
        dsi::WorldMap map2(ctx, leaf, 8), host2(ctx, leaf, 16);
        const size_t nw2 = dsi::full_sequence_depth_maps_alg2(
            0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], t0, t1, duration, duration, true, dsi::Alg2Options(),
            [&](const dsi::WindowDepthMapsAlg2& w) {
                const std::vector<float> c = flat(w.time_camera.point_cloud);
                host2.integrate(c.data(), 4, c.size() / 4, dsi::invert_pose(w.time_camera.T_rv_w));
            },
            2, &opts_depth_map, nullptr, &opts_pc, &map2);
        const dsi::WorldMapCells c1 = map2.extract(), c2 = host2.extract();
        EXPECT(nw2 == nw && map2.info().calls == nw2 && c1.size() > 0);
        EXPECT(c1.keys == c2.keys && c1.n == c2.n && c1.windows == c2.windows && c1.xyz.size() == c2.xyz.size() &&
               std::memcmp(c1.xyz.data(), c2.xyz.data(), c1.xyz.size() * sizeof(float)) == 0);
        std::printf("alg2: %zu windows, %zu cells\n", nw2, c1.size());
    }
    // a mapper of another context is refused; a map without options_point_cloud too
    {
        dsi::Context other(0);
        EMVS::MapperEMVS m(other, cam, shape);
        bool refused = false;
        try {
            map.integrateMapper(m, opts_pc, dsi::invert_pose(dsi::Transformation()));
        } catch (const dsi::Error&) {
            refused = true;
        }
        EXPECT(refused);
        refused = false;
        try {
            dsi::full_sequence_depth_maps(0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], t0, t1, duration, duration, true, 2,
                                          [](const dsi::WindowDepthMap&) {}, 2, 0.0, &opts_depth_map, nullptr, nullptr, &map);
        } catch (const dsi::Error&) {
            refused = true;
        }
        EXPECT(refused);
    }
    write(dir + "/map.xyz.f32", cells.xyz.data(), cells.xyz.size() * sizeof(float));
    write(dir + "/map.n.u32", cells.n.data(), cells.n.size() * sizeof(uint32_t));
    write(dir + "/map.windows.u32", cells.windows.data(), cells.windows.size() * sizeof(uint32_t));
    write(dir + "/map.keys.u64", cells.keys.data(), cells.keys.size() * sizeof(uint64_t));
    const uint64_t iv[4] = {info.occupied, info.calls, info.accepted, info.rejected};
    write(dir + "/map.info.u64", iv, sizeof iv);
    std::printf("world map: %zu windows, %zu points, %zu cells\n", nw, points, cells.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 17) {
        std::fprintf(stderr, "usage: %s DIR width height fx fy cx cy dimZ min_depth max_depth t0 t1 duration leaf radius min_neighbors\n", argv[0]);
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
