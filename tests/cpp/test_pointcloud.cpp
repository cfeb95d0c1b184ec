// The point cloud through the C++ adapter at its call sites: MapperEMVS::getPointcloud spelled as main.cpp:396 spells it,
// with a pcl-shaped cloud (a stand-in of pcl::PointCloud<pcl::PointXYZI>, no PCL here) and with dsi::PointCloud, and
// dsi::full_sequence_depth_maps with point clouds on.  Run by tests/test_gpu_pointcloud.py, which compares what this
// program writes with the Python path and the restatement.
//   test_pointcloud --cloud DIR    depth.f32 mask.u8 (dimY x dimX) and cloud.f32 (N x 4) of one getPointcloud call
//   test_pointcloud --stream DIR   window_<k>.{depth.f32,mask.u8,cloud.f32} of a short window stream
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dsi_engine.hpp"
#include "dsi_process.hpp"

namespace pcl {  // the members of PCL's types the reference's code and dsi::point_cloud_assign use
struct PointXYZI {
    float x, y, z, _pad, intensity, _pad2[3];  // (PCL's layout: data[4] then intensity)
};
template <typename PointT>
struct PointCloud {
    typedef std::shared_ptr<PointCloud<PointT>> Ptr;
    std::vector<PointT> points;
    uint32_t width = 0, height = 0;
    bool is_dense = true;
    void clear()
    {
        points.clear();
        width = height = 0;
    }
    void push_back(const PointT& p)
    {
        points.push_back(p);
        width = (uint32_t)points.size();
        height = 1;
    }
    size_t size() const { return points.size(); }
};
}  // namespace pcl

typedef pcl::PointXYZI PointType;             // mapper_emvs_stereo.hpp
typedef pcl::PointCloud<PointType> PointCloud;

namespace {

int failures = 0;
#define EXPECT(c)                                                              \
    do {                                                                       \
        if (!(c)) {                                                            \
            std::fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

void write(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    if (bytes) std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

template <typename CloudT>
std::vector<float> flat(const CloudT& pc)
{
    std::vector<float> v;
    for (const auto& p : pc.points) v.insert(v.end(), {p.x, p.y, p.z, p.intensity});
    return v;
}

struct Lcg {
    uint64_t s;
    double uni()
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) / 9007199254740992.0;
    }
};

dsi::PinholeCameraModel camera(int w, int h)
{
    dsi::PinholeCameraModel cam;
    cam.width = w;
    cam.height = h;
    cam.fx = cam.fy = 0.5f * (float)w;
    cam.cx = 0.5f * (float)w;
    cam.cy = 0.5f * (float)h;
    return cam;
}

int run_cloud(const std::string& dir)
{
    const dsi::PinholeCameraModel cam = camera(346, 260);
    EMVS::MapperEMVS mapper_fused(cam, EMVS::ShapeDSI(0, 0, 100, 4.f, 200.f, 0.f));
    // a semi-dense map: depth layers 5..40 m in patches, 30 % of the pixels
    dsi::Image<float> depth_map(260, 346);
    dsi::Image<uint8_t> semidense_mask(260, 346);
    Lcg rng{7};
    for (int y = 0; y < 260; ++y)
        for (int x = 0; x < 346; ++x) {
            depth_map.at(y, x) = 5.f + 5.f * (float)((x / 40 + y / 30) % 8) + (float)(0.01 * rng.uni());
            semidense_mask.at(y, x) = rng.uni() < 0.3 ? 1 : 0;
        }
    EMVS::OptionsPointCloud opts_pc;  // main.cpp:393-395
    opts_pc.radius_search_ = 0.5f;
    opts_pc.min_num_neighbors_ = 3;
    PointCloud::Ptr pc(new PointCloud);
    mapper_fused.getPointcloud(depth_map, semidense_mask, opts_pc, pc);  // main.cpp:396
    EXPECT(pc->width == pc->size() && pc->height == 1 && pc->size() > 0);
    EXPECT(mapper_fused.pointsBeforeFilter() > pc->size());
    dsi::PointCloud::Ptr pc2;  // an empty Ptr is created
    mapper_fused.getPointcloud(depth_map, semidense_mask, opts_pc, pc2);
    dsi::PointCloud pc3;
    pc3.push_back(dsi::PointXYZI{1.f, 2.f, 3.f, 4.f});  // (replaced, like pc_->clear() does in the reference)
    mapper_fused.getPointcloud(depth_map, semidense_mask, opts_pc, pc3);
    const std::vector<float> a = flat(*pc), b = flat(*pc2), c = flat(pc3);
    EXPECT(a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
    EXPECT(a.size() == c.size() && std::memcmp(a.data(), c.data(), a.size() * sizeof(float)) == 0);
    write(dir + "/depth.f32", depth_map.data.data(), depth_map.data.size() * sizeof(float));
    write(dir + "/mask.u8", semidense_mask.data.data(), semidense_mask.data.size());
    write(dir + "/cloud.f32", a.data(), a.size() * sizeof(float));
    std::printf("cloud: %zu points of %zu\n", pc->size(), mapper_fused.pointsBeforeFilter());
    return 0;
}

int run_stream(const std::string& dir)
{
    const dsi::PinholeCameraModel cam = camera(240, 180);
    const EMVS::ShapeDSI shape(0, 0, 64, 4.f, 100.f, 0.f);
    const double seconds = 0.4, duration = 0.05;
    std::vector<dsi::Event> ev[2];
    LinearTrajectory::PoseMap poses[2];
    for (int c = 0; c < 2; ++c) {  // points 6..40 m ahead; the rig moves along x at 1 m/s, camera 1 0.3 m to the right
        Lcg rng{21u + (uint64_t)c};
        const int npts = 3000;
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
        const size_t n = 800000;
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
    EMVS::OptionsDepthMap opts_depth_map;
    EMVS::OptionsPointCloud opts_pc;
    opts_pc.radius_search_ = 1.0f;
    opts_pc.min_num_neighbors_ = 2;
    dsi::Context ctx(0);
    EMVS::MapperEMVS check(ctx, cam, shape);  // the host-map call on each window's filtered maps
    size_t windows = 0, points = 0;
    const size_t nw = dsi::full_sequence_depth_maps(
        0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], 0.0, seconds - 1e-9, duration, duration,
        /*forward_looking=*/true, /*fusion_method=*/2,
        [&](const dsi::WindowDepthMap& w) {
            dsi::PointCloud again;
            check.getPointcloud(w.filtered_depth_map, w.semidense_mask, opts_pc, again);
            const std::vector<float> a = flat(w.point_cloud), b = flat(again);
            EXPECT(a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
            const std::string base = dir + "/window_" + std::to_string(w.index);
            write(base + ".depth.f32", w.filtered_depth_map.data.data(), w.filtered_depth_map.data.size() * sizeof(float));
            write(base + ".mask.u8", w.semidense_mask.data.data(), w.semidense_mask.data.size());
            write(base + ".cloud.f32", a.data(), a.size() * sizeof(float));
            points += w.point_cloud.size();
            ++windows;
        },
        2, 0.0, &opts_depth_map, nullptr, &opts_pc);
    EXPECT(nw == windows && windows >= 6 && points > 0);
    // the point cloud needs the filtered maps
    bool refused = false;
    try {
        dsi::full_sequence_depth_maps(0, cam, cam, shape, trajectory0, trajectory1, ev[0], ev[1], 0.0, seconds - 1e-9, duration,
                                      duration, true, 2, [](const dsi::WindowDepthMap&) {}, 1, 0.0, nullptr, nullptr, &opts_pc);
    } catch (const dsi::Error&) {
        refused = true;
    }
    EXPECT(refused);
    std::printf("stream: %zu windows, %zu points\n", windows, points);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s --cloud|--stream DIR\n", argv[0]);
        return 2;
    }
    try {
        const std::string mode = argv[1], dir = argv[2];
        if (mode == "--cloud") run_cloud(dir);
        else if (mode == "--stream") run_stream(dir);
        else return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
