// The Grid3D members added with the slice / min-max / slice-image work, called as the reference spells them
// (cartesian3dgrid.h:40-58,95-109,166-204,222,228; cartesian3dgrid.cpp:72-113,177-188), each compared with memcmp against
// the C ABI's result on the same data.  Run by tests/test_gpu_grid3d.py, which also decodes the PNG files written here.
//   test_grid3d DIR   vol.f32 (the volume, dimZ x dimY x dimX), u8_<dim>.bin (slicesU8(dim, true)), x_NNN.png / y_NNN.png /
//                     z_NNN.png (imwriteSlices), w_NNN.png (imwriteSlices through an imwrite_gray8 overload)
#include <cstdio>
#include <cstring>
#include <stdexcept>
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

// an image type of the caller's own, with its own writer: found by ADL, preferred to dsi::imwrite_gray8
struct MyImage : dsi::Image<uint8_t> {};
int my_writes = 0;
inline bool imwrite_gray8(const std::string& path, const MyImage& img)
{
    ++my_writes;
    return dsi::write_png_gray8(path, img.data.data(), img.rows, img.cols);
}

template <typename F>
bool throws_invalid(F f)
{
    try {
        f();
    } catch (const dsi::Error& e) {
        return e.code == DSI_ERR_INVALID;
    }
    return false;
}

void run(const std::string& dir)
{
    const unsigned nx = 37, ny = 21, nz = 12;
    const size_t n = (size_t)nx * ny * nz;
    Lcg rng{42};
    std::vector<float> a(n), b(n);
    for (size_t i = 0; i < n; ++i) {
        a[i] = rng.uni() * 50.f - 5.f;
        b[i] = rng.uni() * 50.f;
    }
    write(dir + "/vol.f32", a.data(), n * sizeof(float));
    Grid3D ga(nx, ny, nz), gb(nx, ny, nz), gc(nx, ny, nz);
    gb.upload(b);

    // ---- the four voxel-wise members against dsi_grid_binary_op
    for (int op = 1; op <= 4; ++op) {
        ga.upload(a);
        gc.upload(a);
        if (op == 1) ga.subtractTwoGrids(gb);
        if (op == 2) ga.ratioTwoGrids(gb);
        if (op == 3) ga.quadraticMeanTwoGrids(gb);
        if (op == 4) ga.cubicMeanTwoGrids(gb);
        dsi::check(dsi_grid_binary_op(gc.handle(), gb.handle(), op));
        const std::vector<float> x = ga.download(), y = gc.download();
        EXPECT(std::memcmp(x.data(), y.data(), n * sizeof(float)) == 0);
        EXPECT(std::memcmp(x.data(), a.data(), n * sizeof(float)) != 0);
    }
    EXPECT(throws_invalid([&] { ga.ratioTwoGrids(gb, 1e-2f); }));
    ga.upload(a);
    ga.ratioTwoGrids(gb, 1e-1);  // the default, spelled out as a double literal like the reference's declaration

    // ---- getMinMax
    ga.upload(a);
    {
        float mn, mx, mn2, mx2;
        unsigned long mn_pos = 0, mx_pos = 0;
        uint64_t p0, p1;
        ga.getMinMax(&mn, &mx, &mn_pos, &mx_pos);
        dsi::check(dsi_grid_min_max(ga.handle(), &mn2, &mx2, &p0, &p1));
        EXPECT(std::memcmp(&mn, &mn2, 4) == 0 && std::memcmp(&mx, &mx2, 4) == 0 && mn_pos == p0 && mx_pos == p1);
        size_t lo = 0, hi = 0;
        for (size_t i = 1; i < n; ++i) {
            if (a[i] < a[lo]) lo = i;
            if (!(a[i] < a[hi])) hi = i;
        }
        EXPECT(mn_pos == lo && mx_pos == hi && mn == a[lo] && mx == a[hi]);
        float mn3, mx3;
        ga.getMinMax(&mn3, &mx3);  // positions default to NULL
        EXPECT(mn3 == mn && mx3 == mx);
    }

    // ---- single voxels
    {
        const unsigned p = 5 + nx * (7 + ny * 3);
        EXPECT(ga.getGridValueAt(p) == a[p] && ga.getGridValueAt(5, 7, 3) == a[p]);
        ga.setGridValueAt(p, 2.5f);
        ga.accumulateGridValueAt(p, 0.75f);
        EXPECT(ga.getGridValueAt(p) == 3.25f);
        float v = 0;
        dsi::check(dsi_grid_value_at(ga.handle(), p, &v));
        EXPECT(v == 3.25f);
        ga.setGridValueAt(p, a[p]);
        EXPECT(throws_invalid([&] { ga.getGridValueAt((unsigned)n); }));
        EXPECT(throws_invalid([&] { ga.getGridValueAt(nx, 0, 0); }));
        EXPECT(throws_invalid([&] { ga.setGridValueAt((unsigned)n, 1.f); }));
        EXPECT(throws_invalid([&] { ga.accumulateGridValueAt((unsigned)n, 1.f); }));
    }

    // ---- getSlice: the reference's loops, on the host copy
    for (unsigned dim = 0; dim < 3; ++dim) {
        const unsigned size = dim == 0 ? nx : (dim == 1 ? ny : nz);
        for (unsigned s = 0; s < size; s += (dim == 2 ? 1 : 5)) {
            const dsi::Image<float> slice = ga.getSlice(s, dim);
            const unsigned rows = dim == 1 ? nx : ny, cols = dim == 2 ? nx : nz;
            EXPECT(slice.rows == (int)rows && slice.cols == (int)cols);
            std::vector<float> c((size_t)rows * cols);
            dsi::check(dsi_grid_get_slice(ga.handle(), s, dim, c.data()));
            EXPECT(std::memcmp(c.data(), slice.data.data(), c.size() * sizeof(float)) == 0);
            bool same = true;
            for (unsigned v = 0; v < rows; ++v)
                for (unsigned u = 0; u < cols; ++u) {
                    const float want = dim == 0 ? a[s + nx * (v + ny * u)] : (dim == 1 ? a[v + nx * (s + ny * u)] : a[u + nx * (v + ny * s)]);
                    same = same && slice.at((int)v, (int)u) == want;
                }
            EXPECT(same);
        }
        EXPECT(throws_invalid([&] { ga.getSlice(size, dim); }));
    }
    EXPECT(throws_invalid([&] { ga.getSlice(0, 3); }));

    // ---- accumulateZSliceAt with an image smaller than the plane
    {
        dsi::Image<float> img(9, 14);
        for (auto& v : img.data) v = rng.uni();
        ga.accumulateZSliceAt(4, img);
        const std::vector<float> got = ga.download();
        bool same = true;
        for (unsigned iz = 0; iz < nz; ++iz)
            for (unsigned iy = 0; iy < ny; ++iy)
                for (unsigned ix = 0; ix < nx; ++ix) {
                    const size_t p = ix + nx * (iy + ny * iz);
                    const float want = (iz == 4 && iy < 9 && ix < 14) ? a[p] + img.at((int)iy, (int)ix) : a[p];
                    same = same && got[p] == want;
                }
        EXPECT(same);
        EXPECT(throws_invalid([&] { ga.accumulateZSliceAt(nz, img); }));
        dsi::Image<float> wide(2, (int)nx + 1);
        EXPECT(throws_invalid([&] { ga.accumulateZSliceAt(0, wide); }));
        ga.upload(a);
    }

    // ---- slice images and imwriteSlices
    const char* names[3] = {"x_", "y_", "z_"};
    for (unsigned dim = 0; dim < 3; ++dim) {
        const std::vector<uint8_t> u = ga.slicesU8(dim, true);
        std::vector<uint8_t> c(n);
        dsi::check(dsi_grid_slices_u8(ga.handle(), dim, 1, c.data()));
        EXPECT(u.size() == n && std::memcmp(u.data(), c.data(), n) == 0);
        write(dir + "/u8_" + std::to_string(dim) + ".bin", u.data(), n);
        ga.imwriteSlices((dir + "/" + names[dim]).c_str(), dim);
    }
    {
        const std::vector<uint8_t> u = ga.slicesU8(1, false);
        write(dir + "/u8_1_per_slice.bin", u.data(), n);
        ga.imwriteSlices<MyImage>((dir + "/w_").c_str(), 1, false);
        EXPECT(my_writes == (int)ny);
    }
    EXPECT(throws_invalid([&] { ga.slicesU8(3); }));
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    try {
        run(argv[1]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
