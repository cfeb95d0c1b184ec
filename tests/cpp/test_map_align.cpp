// dsi::WorldMap::align_step / align / integrate_map and dsi::compose_pose on the first scene of
// tests/map_align_reference.py.  Run by tests/test_gpu_map_align_cpp.py, which writes the calls this program reads and
// compares what it writes with the Python path.
//   test_map_align DIR leaf_a n_calls_a leaf_b n_calls_b radius max_iterations min_matched eps_rot eps_trans
// reads  DIR/a_<k>.f32, DIR/b_<k>.f32 (N x 3 floats per call, integrated with the identity pose), DIR/T_step.f64 (12 doubles)
// writes DIR/moments.i64 = n_cells, n_matched, n_unmatched, su[3], sv[3], suv_hi[9], suv_lo[9], e2, reach of
//        align_step(b, radius, T_step); DIR/T_out.f64 = align's pose; DIR/info.f64 = iterations, converged, stopped,
//        n_matched_first, n_matched_last, rms_first, rms_last, angle_last, trans_last; DIR/T_solve.f64 = solve_alignment of the
//        moments composed with T_step; DIR/moved.* = the state of a map of leaf_b after integrate_map(a, T_out, 2, 1)
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

void fill(dsi::WorldMap& m, const std::string& dir, const char* name, int n_calls)
{
    for (int k = 0; k < n_calls; ++k) {
        const std::vector<float> pts = read<float>(dir + "/" + name + "_" + std::to_string(k) + ".f32");
        EXPECT(m.integrate(pts.data(), 3, pts.size() / 3, dsi::kIdentityPose) == 0);
    }
}

int run(char** a)
{
    const std::string dir = a[1];
    const double leaf_a = std::atof(a[2]), leaf_b = std::atof(a[4]);
    dsi::Context ctx(0), other(0);
    dsi::WorldMap ma(ctx, leaf_a, 8), mb(ctx, leaf_b, 8);
    fill(ma, dir, "a", std::atoi(a[3]));
    fill(mb, dir, "b", std::atoi(a[5]));
    dsi::MapAlignOptions opts(std::atof(a[6]));
    std::array<double, 12> T_step;
    const std::vector<double> t = read<double>(dir + "/T_step.f64");
    for (size_t k = 0; k < 12; ++k) T_step[k] = t[k];

    // one pass, its solve and the composition
    const dsi::MapAlignMoments m = ma.align_step(mb, opts, T_step);
    std::vector<int64_t> mo = {(int64_t)m.n_cells, (int64_t)m.n_matched, (int64_t)m.n_unmatched};
    mo.insert(mo.end(), m.su, m.su + 3);
    mo.insert(mo.end(), m.sv, m.sv + 3);
    mo.insert(mo.end(), m.suv_hi, m.suv_hi + 9);
    for (int k = 0; k < 9; ++k) mo.push_back((int64_t)m.suv_lo[k]);
    mo.push_back((int64_t)m.e2);
    mo.push_back(m.reach);
    write(dir + "/moments.i64", mo.data(), mo.size() * sizeof(int64_t));
    EXPECT(m.n_cells == m.n_matched + m.n_unmatched && m.n_cells == ma.count() && m.quantum == leaf_b / 1024.0);
    dsi::MapAlignSolveInfo si;
    const std::array<double, 12> T_solve = dsi::compose_pose(dsi::solve_alignment(m, &si), T_step);
    write(dir + "/T_solve.f64", T_solve.data(), sizeof(double) * 12);
    EXPECT(si.n_matched == m.n_matched && si.rms > 0.0);

    // the loop; one round of it is the above
    opts.max_iterations = 1;
    const dsi::MapAlignResult one = ma.align(mb, opts, T_step);
    EXPECT(one.ok && one.T == T_solve && one.info.iterations == 1 && one.info.rms_first == si.rms);
    opts.max_iterations = std::atoi(a[7]);
    opts.min_matched = (uint64_t)std::atoll(a[8]);
    opts.eps_rot = std::atof(a[9]);
    opts.eps_trans = std::atof(a[10]);
    const dsi::MapAlignResult r = ma.align(mb, opts);
    EXPECT(r.ok && r.info.stopped == 0);
    write(dir + "/T_out.f64", r.T.data(), sizeof(double) * 12);
    const double info[9] = {(double)r.info.iterations, (double)r.info.converged, (double)r.info.stopped, (double)r.info.n_matched_first,
                            (double)r.info.n_matched_last, r.info.rms_first, r.info.rms_last, r.info.angle_last, r.info.trans_last};
    write(dir + "/info.f64", info, sizeof info);
    // too few matches: no exception, the last good pose
    dsi::MapAlignOptions strict = opts;
    strict.min_matched = m.n_cells + 1;
    const dsi::MapAlignResult none = ma.align(mb, strict, T_step);
    EXPECT(!none.ok && none.info.stopped == 1 && none.T == T_step && none.info.iterations == 1);

    // a into a map of b's leaf at the pose found
    dsi::WorldMap moved(ctx, leaf_b, 8);
    uint64_t rejected = 7;
    const uint64_t n = moved.integrate_map(ma, r.T, 2, 1, &rejected);
    EXPECT(n == ma.count(2, 1) && rejected == 0 && moved.info().calls == 1 && moved.info().accepted == n);
    const dsi::MapState s = moved.exportState();
    write(dir + "/moved.keys.u64", s.keys.data(), s.keys.size() * sizeof(uint64_t));
    write(dir + "/moved.n.u32", s.n.data(), s.n.size() * sizeof(uint32_t));
    write(dir + "/moved.S.u64", s.S.data(), s.S.size() * sizeof(uint64_t));
    // refusals
    dsi::WorldMap foreign(other, leaf_b, 8);
    EXPECT(refused([&] { moved.integrate_map(moved); }, DSI_ERR_INVALID));
    EXPECT(refused([&] { moved.integrate_map(foreign); }, DSI_ERR_CONTEXT));
    EXPECT(refused([&] { ma.align_step(foreign, opts); }, DSI_ERR_CONTEXT));
    EXPECT(refused([&] { ma.align(foreign, opts); }, DSI_ERR_CONTEXT));
    dsi::MapAlignOptions wide(4.0 * leaf_b);
    EXPECT(refused([&] { ma.align_step(mb, wide); }, DSI_ERR_INVALID));
    std::printf("matched %llu of %llu; %d rounds, rms %.6f -> %.6f; %llu cells moved\n", (unsigned long long)m.n_matched,
                (unsigned long long)m.n_cells, r.info.iterations, r.info.rms_first, r.info.rms_last, (unsigned long long)n);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 11) {
        std::fprintf(stderr, "usage: %s DIR leaf_a n_calls_a leaf_b n_calls_b radius max_iterations min_matched eps_rot eps_trans\n", argv[0]);
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
