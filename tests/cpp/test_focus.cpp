// The focus-based collapses through the C++ adapter: getDepthMapFromDSIByFocus, the focus half of getDepthMapFromDSI's
// method switch (mapper_emvs_stereo.cpp:348-364), Grid3D::collapseZSliceByDoG / collapseMinZSlice / computeLocalFocusInPlace
// (cartesian3dgrid.h:207-216) and fuseDSIs_HarmonicMeanOfLocalFocus (utils.hpp:54-60) with its seven arguments.  Run by
// tests/test_gpu_focus.py, which compares what this program writes with the restatement of tests/focus_reference.py.
//   test_focus DIR   dsi0.f32 dsi1.f32 (the inputs, dimZ x dimY x dimX), method3.{depth,conf}.f32 method3.mask.u8,
//                    dog.{conf.f32,idx.u8}, min.{val.f32,idx.u8}, lms.f32 (computeLocalFocusInPlace(1)), fused.f32
#include <cstdio>
#include <stdexcept>
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

void write(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    if (bytes) std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

struct Lcg {
    uint64_t s;
    float uni()
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (float)((double)(s >> 40) / 16777216.0);
    }
};

template <typename T>
void write_img(const std::string& path, const dsi::Image<T>& img)
{
    write(path, img.data.data(), img.data.size() * sizeof(T));
}

void run(const std::string& dir)
{
    dsi::PinholeCameraModel cam;
    cam.width = 96;
    cam.height = 72;
    cam.fx = cam.fy = 48.f;
    cam.cx = 48.f;
    cam.cy = 36.f;
    const EMVS::ShapeDSI shape(0, 0, 40, 4.f, 200.f, 0.f);
    EMVS::MapperEMVS mapper0(cam, shape), mapper1(cam, shape), mapper_fused(cam, shape);
    int nx, ny, nz;
    mapper0.dsi_.getDimensions(&nx, &ny, &nz);
    const size_t n = (size_t)nx * ny * nz;
    std::vector<float> v0(n), v1(n);
    Lcg rng{12345};
    for (size_t i = 0; i < n; ++i) {  // sparse, vote-like volumes: mostly small integers, some zeros
        v0[i] = rng.uni() < 0.3f ? 0.f : (float)(int)(rng.uni() * 9.f);
        v1[i] = rng.uni() < 0.3f ? 0.f : (float)(int)(rng.uni() * 9.f) + 0.5f * rng.uni();
    }
    mapper0.dsi_.upload(v0);
    mapper1.dsi_.upload(v1);
    write(dir + "/dsi0.f32", v0.data(), n * sizeof(float));
    write(dir + "/dsi1.f32", v1.data(), n * sizeof(float));

    // mapper_emvs_stereo.hpp:108 with method 3 (LaplacianMag), on the mapper's own DSI
    EMVS::OptionsDepthMap opts;
    dsi::Image<float> depth_map, confidence_map;
    dsi::Image<uint8_t> semidense_mask;
    mapper0.getDepthMapFromDSIByFocus(depth_map, confidence_map, semidense_mask, opts, 3);
    EXPECT(depth_map.rows == ny && depth_map.cols == nx && semidense_mask.rows == ny);
    write_img(dir + "/method3.depth.f32", depth_map);
    write_img(dir + "/method3.conf.f32", confidence_map);
    write_img(dir + "/method3.mask.u8", semidense_mask);

    dsi::Image<float> c;
    dsi::Image<uint8_t> i;
    mapper0.dsi_.collapseZSliceByDoG(&c, &i);
    EXPECT(c.rows == ny && c.cols == nx && i.rows == ny && i.cols == nx);
    write_img(dir + "/dog.conf.f32", c);
    write_img(dir + "/dog.idx.u8", i);
    mapper0.dsi_.collapseMinZSlice(&c, &i);
    write_img(dir + "/min.val.f32", c);
    write_img(dir + "/min.idx.u8", i);

    Grid3D grid(nx, ny, nz);  // cartesian3dgrid.h:26
    grid.resetGrid();
    grid.addTwoGrids(mapper0.dsi_);
    grid.computeLocalFocusInPlace(1);
    const std::vector<float> lms = grid.download();
    write(dir + "/lms.f32", lms.data(), n * sizeof(float));
    EXPECT(mapper0.dsi_.download() == v0);  // the copy was transformed, not the source

    // utils.hpp:54-60: the variance-based local focus (0), harmonic mean
    fuseDSIs_HarmonicMeanOfLocalFocus(mapper0, mapper1, cam, cam, shape, 0, mapper_fused);
    const std::vector<float> fused = mapper_fused.dsi_.download();
    write(dir + "/fused.f32", fused.data(), n * sizeof(float));
    EXPECT(mapper1.dsi_.download() == v1);

    bool kept = false;  // the reference-spelled overload keeps refusing 0..4
    try {
        mapper0.getDepthMapFromDSI(depth_map, confidence_map, semidense_mask, opts, 3);
    } catch (const dsi::Error& e) {
        kept = e.code == DSI_ERR_BAD_OP;
    }
    EXPECT(kept);

    bool refused = false;  // an unknown focus method is refused by the C layer
    try {
        float cf[1];
        uint8_t ix[1];
        dsi::check(dsi_grid_collapse_focus(grid.handle(), 5, 1, cf, ix));
    } catch (const dsi::Error&) {
        refused = true;
    }
    EXPECT(refused);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_focus DIR\n");
        return 2;
    }
    try {
        run(argv[1]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
