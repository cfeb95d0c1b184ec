// dsi::full_sequence_depth_maps_alg2 (main.cpp:275-299 with --process_method=2 / 5 as a stream) against the materialising
// path window by window: ::process_2 / ::process_5 on fresh mappers, then getDepthMapFromDSI of mapper_fused and of
// mapper_fused_camera_time -- raw maps, filtered maps and point clouds compared with memcmp.  Run by
// tests/test_gpu_alg2_stream.py; tests/test_alg2_cpu.py builds it and checks that it refuses to run without a GPU.
//   exit 0 + "OK": all equal      exit 2 + "no GPU": no HIP device      else: failure
#include <cmath>
#include <cstdio>
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

struct Lcg {
    uint64_t s;
    double uni()
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) / 9007199254740992.0;
    }
};

template <typename Img>
bool same(const Img& a, const Img& b)
{
    return a.rows == b.rows && a.cols == b.cols && a.data.size() == b.data.size() &&
           std::memcmp(a.data.data(), b.data.data(), a.data.size() * sizeof(a.data[0])) == 0;
}

bool same_cloud(const dsi::PointCloud& a, const dsi::PointCloud& b)
{
    return a.points.size() == b.points.size() &&
           std::memcmp(a.points.data(), b.points.data(), a.points.size() * sizeof(a.points[0])) == 0;
}

}  // namespace

int main()
{
    if (dsi_device_count() <= 0) {
        std::printf("no GPU: nothing to run\n");
        return 2;
    }
    try {
        dsi::PinholeCameraModel cam;
        cam.width = 160;
        cam.height = 120;
        cam.fx = cam.fy = 80.f;
        cam.cx = 80.f;
        cam.cy = 60.f;
        const EMVS::ShapeDSI shape(0, 0, 40, 4.f, 100.f, 0.f);
        const double seconds = 0.4, duration = 0.05;
        std::vector<dsi::Event> ev[2];
        LinearTrajectory::PoseMap poses[2];
        for (int c = 0; c < 2; ++c) {  // points 6..40 m ahead; the rig moves along x at 1 m/s, camera 1 0.3 m to the right
            Lcg rng{31u + (uint64_t)c};
            const int npts = 2000;
            std::vector<double> P(3 * npts);
            for (int i = 0; i < npts; ++i) {
                const double z = 6.0 + 34.0 * rng.uni();
                P[3 * i] = (rng.uni() - 0.5) * 2.0 * z;
                P[3 * i + 1] = (rng.uni() - 0.5) * 1.5 * z;
                P[3 * i + 2] = z;
            }
            const double x_off = 0.3 * c;
            for (int k = 0; k < 60; ++k) {
                dsi::Transformation T;
                T.t[0] = 0.01 * k - 0.1 + x_off;
                poses[c][0.01 * k - 0.1] = T;
            }
            const size_t n = 320000 + 777 * (size_t)c;  // (sub-interval tails dropped; process_5's wrap)
            for (size_t k = 0; k < n; ++k) {
                const double t = seconds * (double)k / (double)n;
                const int i = (int)(rng.uni() * npts) % npts;
                const double u = cam.fx * (P[3 * i] - (t + x_off)) / P[3 * i + 2] + cam.cx;
                const double v = cam.fy * P[3 * i + 1] / P[3 * i + 2] + cam.cy;
                dsi::Event e;
                e.ts = t;
                if (u < 0 || v < 0 || u >= cam.width - 1 || v >= cam.height - 1) {
                    e.x = (uint16_t)(rng.uni() * cam.width);
                    e.y = (uint16_t)(rng.uni() * cam.height);
                } else {
                    e.x = (uint16_t)std::lround(u);
                    e.y = (uint16_t)std::lround(v);
                }
                ev[c].push_back(e);
            }
        }
        const LinearTrajectory trajectory0(poses[0]), trajectory1(poses[1]);
        EMVS::OptionsDepthMap opts_dm;
        EMVS::OptionsPointCloud opts_pc;
        opts_pc.radius_search_ = 1.0f;
        opts_pc.min_num_neighbors_ = 2;
        dsi::Context ctx(0);
        struct Case {
            int pm, n_sub, sf, tf, camera_time;
            bool filters;
        };
        // (n_sub 9: the planner's materialising path; tf 3: no vote at all)
        const Case cases[] = {{2, 3, 2, 2, -1, true}, {5, 4, 4, 4, -1, true}, {5, 2, 3, 2, 1, false}, {2, 9, 2, 4, -1, false},
                              {2, 2, 1, 3, -1, false}};
        for (const Case& cs : cases) {
            dsi::Alg2Options o;
            o.process_method = cs.pm;
            o.num_subintervals = cs.n_sub;
            o.stereo_fusion = cs.sf;
            o.temporal_fusion = cs.tf;
            o.camera_time = cs.camera_time;
            size_t windows = 0;
            const size_t nw = dsi::full_sequence_depth_maps_alg2(
                0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], 0.0, seconds - 1e-9, duration, duration, true, o,
                [&](const dsi::WindowDepthMapsAlg2& w) {
                    const dsi::WindowDepthMap& tc = w.time_camera;
                    EXPECT(w.has_camera_time == (cs.camera_time < 0 ? cs.pm == 2 : cs.camera_time != 0));
                    std::vector<dsi::Event> we[2];
                    for (int c = 0; c < 2; ++c) {
                        size_t a = 0, b = 0;
                        dsi::window_event_range(ev[c], tc.t_start, tc.t_stop, &a, &b);
                        we[c].assign(ev[c].begin() + (long)a, ev[c].begin() + (long)b);
                    }
                    EMVS::MapperEMVS fused(ctx, cam, shape), cam_time(ctx, cam, shape);
                    ::process_2(ctx, cam, cam, trajectory0, trajectory1, we[0], we[1], shape, cs.n_sub, fused, cam_time, tc.ts,
                                cs.sf, cs.tf, cs.pm == 5);
                    EMVS::MapperEMVS* refs[2] = {&fused, &cam_time};
                    const dsi::WindowDepthMap* gots[2] = {&w.time_camera, &w.camera_time};
                    for (int k = 0; k < (w.has_camera_time ? 2 : 1); ++k) {
                        dsi::Image<float> depth, conf;
                        dsi::Image<uint8_t> idx, mask;
                        refs[k]->getDepthMapFromDSI(depth, conf, idx);
                        EXPECT(same(depth, gots[k]->depth_map) && same(conf, gots[k]->confidence_map) &&
                               same(idx, gots[k]->depth_cell_indices));
                        if (cs.filters) {
                            refs[k]->getDepthMapFromDSI(depth, conf, mask, opts_dm);
                            EXPECT(same(depth, gots[k]->filtered_depth_map) && same(conf, gots[k]->filtered_confidence_map) &&
                                   same(mask, gots[k]->semidense_mask));
                            dsi::PointCloud pc;
                            refs[k]->getPointcloud(opts_pc, pc);
                            EXPECT(same_cloud(pc, gots[k]->point_cloud));
                        }
                    }
                    ++windows;
                },
                2, cs.filters ? &opts_dm : nullptr, nullptr, cs.filters ? &opts_pc : nullptr);
            EXPECT(nw == windows && windows >= 7);
            std::printf("process_method %d, N %d, sf %d, tf %d: %zu windows\n", cs.pm, cs.n_sub, cs.sf, cs.tf, windows);
        }
        // argument checks
        bool bad_op = false, bad_pc = false;
        try {
            dsi::Alg2Options o;
            o.stereo_fusion = 7;
            dsi::full_sequence_depth_maps_alg2(0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], 0.0, seconds, duration,
                                               duration, true, o, [](const dsi::WindowDepthMapsAlg2&) {});
        } catch (const dsi::Error& e) {
            bad_op = e.code == DSI_ERR_BAD_OP;
        }
        try {
            dsi::full_sequence_depth_maps_alg2(0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], 0.0, seconds, duration,
                                               duration, true, dsi::Alg2Options{}, [](const dsi::WindowDepthMapsAlg2&) {}, 1, nullptr,
                                               nullptr, &opts_pc);
        } catch (const dsi::Error& e) {
            bad_pc = e.code == DSI_ERR_INVALID;
        }
        EXPECT(bad_op && bad_pc);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
