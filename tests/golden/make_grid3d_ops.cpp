// Generator of tests/golden/grid3d_ops.npz: runs the GENUINE Grid3D members subtractTwoGrids, ratioTwoGrids,
// quadraticMeanTwoGrids and cubicMeanTwoGrids of the reference's cartesian3dgrid.h on input pairs read from a file.
// The reference header is included BY PATH from wherever the reference tree lies (-I <reference>/cartesian3dgrid/include);
// <opencv2/core/core.hpp> is a stand-in that make_grid3d_ops.py writes into a temporary directory (a cv::Mat with rows,
// cols and at<T>()).  Nothing of the reference is copied here: the four constructors / allocators the header only declares
// are defined below in the obvious way.  Built and run by make_grid3d_ops.py; neither the binary nor its inputs are kept.
//
//   g++ -O2 -std=c++17 -I <tmp>/standin -I <reference>/cartesian3dgrid/include make_grid3d_ops.cpp -o gen
//   ./gen pairs.bin out.bin      pairs.bin: n x (a, g) float32;  out.bin: 4 x n float32 (subtract, ratio, quadratic, cubic)
//
// It also prints which overload the header's unqualified fabs() resolves to in this translation unit.
#include <cartesian3dgrid/cartesian3dgrid.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

Grid3D::Grid3D() { deallocate(); }
Grid3D::Grid3D(const unsigned int dimX, const unsigned int dimY, const unsigned int dimZ) { allocate(dimX, dimY, dimZ); }
Grid3D::~Grid3D() {}
void Grid3D::allocate(const unsigned int dimX, const unsigned int dimY, const unsigned int dimZ)
{
    size_[0] = dimX;
    size_[1] = dimY;
    size_[2] = dimZ;
    numCells_ = dimX * dimY * dimZ;
    data_array_.assign(numCells_, 0.f);
}
void Grid3D::deallocate()
{
    size_[0] = size_[1] = size_[2] = 0;
    numCells_ = 0;
    data_array_.clear();
}

static void fill(Grid3D& g, const std::vector<float>& v)
{
    for (unsigned p = 0; p < v.size(); ++p) g.setGridValueAt(p, v[p]);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    // the same expression as cartesian3dgrid.h:107, seen after the same includes
    const bool fabs_is_double = std::is_same<decltype(fabs(0.f)), double>::value;
    std::printf("fabs(float) resolves to the %s overload\n", fabs_is_double ? "double" : "float");
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / (2 * sizeof(float));
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> ag(2 * n), a(n), g(n);
    if (std::fread(ag.data(), sizeof(float), 2 * n, f) != 2 * n) return 4;
    std::fclose(f);
    for (size_t i = 0; i < n; ++i) {
        a[i] = ag[2 * i];
        g[i] = ag[2 * i + 1];
    }
    Grid3D gb((unsigned)n, 1, 1);
    fill(gb, g);
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    for (int op = 0; op < 4; ++op) {
        Grid3D ga((unsigned)n, 1, 1);
        fill(ga, a);
        if (op == 0) ga.subtractTwoGrids(gb);
        if (op == 1) ga.ratioTwoGrids(gb);
        if (op == 2) ga.quadraticMeanTwoGrids(gb);
        if (op == 3) ga.cubicMeanTwoGrids(gb);
        std::vector<float> out(n);
        for (unsigned p = 0; p < n; ++p) out[p] = ga.getGridValueAt(p);
        if (std::fwrite(out.data(), sizeof(float), n, f) != n) return 6;
    }
    std::fclose(f);
    return 0;
}
