// dsi::WorldMap::render / fetch_render and DepthScore::addMapRender.  Run by tests/test_gpu_world_map_render_cpp.py, which
// writes the calls and the view this program reads and compares the images it writes with the numpy restatement
// (tests/world_map_render_reference.py).
//   test_world_map_render DIR leaf n_calls width height fx fy cx cy min_depth max_depth
// reads  DIR/call_<k>.f32 (N x 3 floats, integrated with the identity pose), DIR/T_v_w.f64 (12 doubles)
// writes DIR/render_s<splat>_w<min_windows>.{depth.f32,windows.u32,hits.u32,mask.u8,info.u64} for splat 0, 1, 2 and
//        min_windows 1, 2; info = n_cells, n_clipped, n_outside, n_drawn, n_pixels, width, height
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
    const double leaf = std::atof(a[2]);
    const int n_calls = std::atoi(a[3]);
    dsi::MapView view{};
    view.width = std::atoi(a[4]);
    view.height = std::atoi(a[5]);
    view.fx = std::atof(a[6]);
    view.fy = std::atof(a[7]);
    view.cx = std::atof(a[8]);
    view.cy = std::atof(a[9]);
    view.min_depth = std::atof(a[10]);
    view.max_depth = std::atof(a[11]);
    view.min_points = 1;
    const auto T = read<double>(dir + "/T_v_w.f64");
    EXPECT(T.size() == 12);
    std::memcpy(view.T_v_w, T.data(), sizeof view.T_v_w);

    dsi::Context ctx(0);
    dsi::WorldMap map(ctx, leaf, 8);
    // nothing rendered yet
    EXPECT(refused([&] { map.fetch_render(); }, DSI_ERR_INVALID));
    const std::array<double, 12> identity = dsi::pose_matrix(dsi::Transformation());
    for (int k = 0; k < n_calls; ++k) {
        const auto pts = read<float>(dir + "/call_" + std::to_string(k) + ".f32");
        EXPECT(map.integrate(pts.data(), 3, pts.size() / 3, identity) == 0);
    }
    const size_t npix = (size_t)view.width * (size_t)view.height;
    for (int splat = 0; splat <= 2; ++splat)
        for (uint32_t mw = 1; mw <= 2; ++mw) {
            view.splat = splat;
            view.min_windows = mw;
            const dsi::MapRenderInfo info = map.render(view);
            EXPECT(info.n_cells == map.count(1, mw) && info.n_cells == info.n_clipped + info.n_outside + info.n_drawn);
            EXPECT(info.width == view.width && info.height == view.height);
            const dsi::MapRenderImages img = map.fetch_render();
            EXPECT(img.width == view.width && img.height == view.height && img.depth.size() == npix && img.mask.size() == npix);
            // the pointer form with outputs left out gives the same depth
            std::vector<float> depth(npix);
            map.fetch_render(depth.data());
            EXPECT(std::memcmp(depth.data(), img.depth.data(), npix * sizeof(float)) == 0);
            uint64_t covered = 0;
            for (size_t i = 0; i < npix; ++i) covered += img.mask[i] ? 1 : 0;
            EXPECT(covered == info.n_pixels);
            const std::string base = dir + "/render_s" + std::to_string(splat) + "_w" + std::to_string(mw);
            write(base + ".depth.f32", img.depth.data(), npix * sizeof(float));
            write(base + ".windows.u32", img.windows.data(), npix * sizeof(uint32_t));
            write(base + ".hits.u32", img.hits.data(), npix * sizeof(uint32_t));
            write(base + ".mask.u8", img.mask.data(), npix);
            const uint64_t iv[7] = {info.n_cells, info.n_clipped, info.n_outside, info.n_drawn, info.n_pixels, (uint64_t)info.width,
                                    (uint64_t)info.height};
            write(base + ".info.u64", iv, sizeof iv);
            // scored against itself: every covered pixel is a joint pixel without error (depths >= min_depth > gt_min)
            dsi::DepthScore score(ctx, npix, 0.5, view.fx, 0.05);
            score.addMapRender(map, img.depth.data());
            const dsi_score_metrics_t m = score.metrics();
            EXPECT(m.n_est == covered && m.n_gt == covered && m.n_joint == covered && m.sum_abs == 0.0);
            std::printf("splat %d min_windows %u: %llu cells, %llu drawn, %llu pixels\n", splat, mw, (unsigned long long)info.n_cells,
                        (unsigned long long)info.n_drawn, (unsigned long long)info.n_pixels);
        }
    // a changed map has no render; a score of another context is refused
    {
        dsi::Context other(0);
        dsi::DepthScore foreign(other, npix, 0.5, view.fx, 0.05);
        std::vector<float> gt(npix, 1.f);
        EXPECT(refused([&] { foreign.addMapRender(map, gt.data()); }, DSI_ERR_CONTEXT));
        const float p[3] = {0.f, 0.f, 1.f};
        map.integrate(p, 3, 1, identity);
        dsi::DepthScore score(ctx, npix, 0.5, view.fx, 0.05);
        EXPECT(refused([&] { map.fetch_render(); }, DSI_ERR_INVALID));
        EXPECT(refused([&] { score.addMapRender(map, gt.data()); }, DSI_ERR_INVALID));
        dsi::MapView bad = view;
        bad.splat = 5;
        EXPECT(refused([&] { map.render(bad); }, DSI_ERR_INVALID));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 12) {
        std::fprintf(stderr, "usage: %s DIR leaf n_calls width height fx fy cx cy min_depth max_depth\n", argv[0]);
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
