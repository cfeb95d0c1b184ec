// The lens rectification path through the C++ adapter (include/dsi_engine.hpp), with stand-ins for the
// types image_geometry::PinholeCameraModel hands out (cv::Matx33d / cv::Matx34d / cv::Mat_<double>): no OpenCV here.
//   test_rectify --lens-of   host only: dsi::lens_of on two stand-in camera types; prints what it extracted, one line per
//                            field, for tests/test_rectify_cpu.py; the host camera_of(cam, &out) still refuses fisheye
//   test_rectify DIR         on the GPU, run by tests/test_gpu_rectify.py: camera_of(ctx, cam, &out) for both models,
//                            MapperEMVS(ctx, cam, lens, shape) against MapperEMVS(ctx, cam-with-table, shape) and a mapper
//                            without a table; writes plumb_bob.lut.f32 and fisheye.lut.f32 (the tables) into DIR
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dsi_engine.hpp"

namespace cvlike {
template <int R, int C>
struct Matx {  // cv::Matx<double, R, C>: operator()(row, col)
    double v[R * C];
    double operator()(int r, int c) const { return v[r * C + c]; }
};
struct MatD {  // cv::Mat_<double>, a row or column vector: total(), operator()(index)
    std::vector<double> v;
    size_t total() const { return v.size(); }
    double operator()(int i) const { return v[(size_t)i]; }
};
struct Mat64 {  // a plain cv::Mat of CV_64F: at<double>(row, col), at<double>(index), total()
    int rows = 0, cols = 0;
    std::vector<double> v;
    size_t total() const { return v.size(); }
    template <typename T> const T& at(int r, int c) const { return v[(size_t)r * cols + c]; }
    template <typename T> const T& at(int i) const { return v[(size_t)i]; }
};
struct Size {
    int width, height;
};
struct Point2d {
    double x, y;
    Point2d(double x_ = 0, double y_ = 0) : x(x_), y(y_) {}
};
}  // namespace cvlike

namespace {

// plumb_bob A of tests/rectify_cases.py
const double kA_K[9] = {226.38, 0.0, 173.65, 0.0, 226.15, 133.73, 0.0, 0.0, 1.0};
const double kA_D[4] = {-0.09, 0.19, 8e-5, 2e-3};
const double kA_P[12] = {199.65, 0.0, 177.43, -19.94, 0.0, 199.65, 126.81, 0.0, 0.0, 0.0, 1.0, 0.0};
// a fisheye lens of the same size
const double kF_K[9] = {180.5, 0.0, 172.0, 0.0, 180.1, 131.0, 0.0, 0.0, 1.0};
const double kF_D[4] = {-0.04, 0.003, -0.002, 0.0003};

void rot_y(double deg, double* R)
{
    const double a = deg * 3.14159265358979323846 / 180.0;
    const double r[9] = {std::cos(a), 0.0, std::sin(a), 0.0, 1.0, 0.0, -std::sin(a), 0.0, std::cos(a)};
    std::memcpy(R, r, sizeof r);
}

// image_geometry::PinholeCameraModel's accessors; D as cv::Mat_<double>
class MatxCamera {
public:
    struct CameraInfo {
        std::string distortion_model;
    };
    MatxCamera(int w, int h, const char* model, const double* K, const double* D, int nd, const double* R, const double* P)
        : w_(w), h_(h)
    {
        info_.distortion_model = model;
        std::memcpy(K_.v, K, sizeof K_.v);
        std::memcpy(R_.v, R, sizeof R_.v);
        std::memcpy(P_.v, P, sizeof P_.v);
        D_.v.assign(D, D + nd);
    }
    const CameraInfo& cameraInfo() const { return info_; }
    cvlike::Size fullResolution() const { return cvlike::Size{w_, h_}; }
    double fx() const { return P_(0, 0); }  // image_geometry: of the projection matrix
    double fy() const { return P_(1, 1); }
    double cx() const { return P_(0, 2); }
    double cy() const { return P_(1, 2); }
    const cvlike::Matx<3, 3>& intrinsicMatrix() const { return K_; }
    const cvlike::MatD& distortionCoeffs() const { return D_; }
    const cvlike::Matx<3, 3>& rotationMatrix() const { return R_; }
    const cvlike::Matx<3, 4>& fullProjectionMatrix() const { return P_; }
    // the host path's hook: must not be reached by the device path
    cvlike::Point2d rectifyPoint(const cvlike::Point2d& p) const
    {
        ++rectify_calls;
        return p;
    }
    mutable long rectify_calls = 0;

private:
    int w_, h_;
    CameraInfo info_;
    cvlike::Matx<3, 3> K_, R_;
    cvlike::Matx<3, 4> P_;
    cvlike::MatD D_;
};

// a camera type that keeps plain matrices (cv::Mat of CV_64F) and a std::vector of coefficients, and has no cameraInfo()
class PlainCamera {
public:
    PlainCamera(const double* K, const std::vector<double>& D, const double* R, const double* P) : D_(D)
    {
        K_.rows = K_.cols = R_.rows = R_.cols = 3;
        P_.rows = 3;
        P_.cols = 4;
        K_.v.assign(K, K + 9);
        R_.v.assign(R, R + 9);
        P_.v.assign(P, P + 12);
    }
    const cvlike::Mat64& intrinsicMatrix() const { return K_; }
    const std::vector<double>& distortionCoeffs() const { return D_; }
    const cvlike::Mat64& rotationMatrix() const { return R_; }
    const cvlike::Mat64& fullProjectionMatrix() const { return P_; }

private:
    cvlike::Mat64 K_, R_, P_;
    std::vector<double> D_;
};

void print_lens(const char* name, const dsi::Lens& L)
{
    std::printf("%s model %s n_dist %d\n", name, L.model_name().c_str(), L.n_dist);
    const struct {
        const char* tag;
        const double* p;
        int n;
    } rows[4] = {{"K", L.K, 9}, {"D", L.D, 8}, {"R", L.R, 9}, {"P", L.P, 12}};
    for (const auto& r : rows) {
        std::printf("%s %s", name, r.tag);
        for (int i = 0; i < r.n; ++i) std::printf(" %.17g", r.p[i]);
        std::printf("\n");
    }
}

int lens_of_mode()
{
    double R[9];
    rot_y(2.0, R);
    const MatxCamera a(346, 260, "plumb_bob", kA_K, kA_D, 4, R, kA_P);
    print_lens("matx", dsi::lens_of(a));
    const double D8[8] = {-0.12, 0.03, 1e-3, -5e-4, -0.004, 0.02, 0.005, 0.001};
    const MatxCamera f(346, 260, "fisheye", kF_K, kF_D, 4, R, kA_P);
    print_lens("fisheye", dsi::lens_of(f));
    const PlainCamera p(kA_K, std::vector<double>(D8, D8 + 8), R, kA_P);  // no cameraInfo(): plumb_bob
    print_lens("plain", dsi::lens_of(p));
    dsi::lens_of(a).check();
    dsi::lens_of(f).check();
    dsi::lens_of(p).check();

    try {  // a model the reference does not know
        dsi::lens_of(MatxCamera(346, 260, "equidistant", kF_K, kF_D, 4, R, kA_P));
        return 31;
    } catch (const dsi::Error& e) {
        if (e.code != DSI_ERR_INVALID) return 32;
    }
    try {  // 12 coefficients: thin-prism terms
        const double D12[12] = {0};
        dsi::lens_of(MatxCamera(346, 260, "plumb_bob", kA_K, D12, 12, R, kA_P));
        return 33;
    } catch (const dsi::Error& e) {
        if (e.code != DSI_ERR_INVALID) return 34;
    }
    try {  // 6 coefficients pass lens_of and are refused by the engine's check
        const double D6[6] = {0};
        dsi::lens_of(MatxCamera(346, 260, "plumb_bob", kA_K, D6, 6, R, kA_P)).check();
        return 35;
    } catch (const dsi::Error& e) {
        if (e.code != DSI_ERR_INVALID) return 36;
    }
    // dsi::Lens on its own: the defaults
    dsi::Lens L;
    L.set_K(100.0, 101.0, 50.0, 40.0).set_D({0.1, 0.2, 0.0, 0.0});
    print_lens("own", L);
    L.check();

    // the host path is what it was: plumb_bob through the camera's rectifyPoint, fisheye refused
    dsi::PinholeCameraModel out;
    const MatxCamera small(8, 6, "plumb_bob", kA_K, kA_D, 4, R, kA_P);
    dsi::camera_of(small, &out);
    if (small.rectify_calls != 48 || out.rectified_points.size() != 96 || out.rectified_points[2 * (3 * 8 + 5)] != 5.f) return 37;
    try {
        dsi::camera_of(MatxCamera(8, 6, "fisheye", kF_K, kF_D, 4, R, kA_P), &out);
        return 38;
    } catch (const dsi::Error& e) {
        if (e.code != DSI_ERR_INVALID || std::string(e.what()).find("fisheye") == std::string::npos) return 39;
    }
    std::printf("OK\n");
    return 0;
}

struct Lcg {
    uint64_t s;
    double uni()
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) / 9007199254740992.0;
    }
};

void write(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    if (bytes) std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

int gpu_mode(const std::string& dir)
{
    const int W = 346, H = 260;
    double R[9];
    rot_y(2.0, R);
    const MatxCamera a(W, H, "plumb_bob", kA_K, kA_D, 4, R, kA_P), f(W, H, "fisheye", kF_K, kF_D, 4, R, kA_P);
    dsi::Context ctx(0);

    dsi::PinholeCameraModel cam_a, cam_f;
    dsi::camera_of(ctx, a, &cam_a);  // both models through the engine
    dsi::camera_of(ctx, f, &cam_f);
    if (a.rectify_calls != 0 || f.rectify_calls != 0) return 41;
    if (cam_a.width != W || cam_a.height != H || cam_a.fx != 199.65f || cam_a.cy != 126.81f) return 42;
    if (cam_a.rectified_points.size() != (size_t)2 * W * H || cam_f.rectified_points.size() != (size_t)2 * W * H) return 43;
    if (cam_a.rectified_points != dsi::rectified_points(ctx, dsi::lens_of(a), W, H)) return 44;
    write(dir + "/plumb_bob.lut.f32", cam_a.rectified_points.data(), cam_a.rectified_points.size() * sizeof(float));
    write(dir + "/fisheye.lut.f32", cam_f.rectified_points.data(), cam_f.rectified_points.size() * sizeof(float));

    // one batch of 8 packets through three mappers: the lens constructor, the table, no table
    dsi::PinholeCameraModel bare = cam_a;
    bare.rectified_points.clear();
    const EMVS::ShapeDSI shape(0, 0, 32, 1.0f, 5.0f, 0.f);
    EMVS::MapperEMVS with_lens(ctx, bare, dsi::lens_of(a), shape), with_table(ctx, cam_a, shape), without(ctx, bare, shape);
    std::vector<dsi::Event> events(8192);
    Lcg rng{77};
    for (size_t i = 0; i < events.size(); ++i) {
        events[i].x = (uint16_t)(rng.uni() * W);
        events[i].y = (uint16_t)(rng.uni() * H);
        events[i].ts = (double)i / (double)events.size();
    }
    LinearTrajectory::PoseMap poses;
    for (int k = 0; k <= 12; ++k) {
        dsi::Transformation T;
        T.t[0] = 0.4 * (0.1 * k - 0.1);
        poses[0.1 * k - 0.1] = T;
    }
    const LinearTrajectory trajectory(poses);
    dsi::Transformation T_rv_w;
    T_rv_w.t[0] = -0.2;
    if (!with_lens.evaluateDSI(events, trajectory, T_rv_w) || !with_table.evaluateDSI(events, trajectory, T_rv_w) ||
        !without.evaluateDSI(events, trajectory, T_rv_w))
        return 45;
    const std::vector<float> d_lens = with_lens.dsi_.download(), d_table = with_table.dsi_.download(), d_none = without.dsi_.download();
    if (d_lens.size() != (size_t)W * H * 32) return 46;
    if (std::memcmp(d_lens.data(), d_table.data(), d_lens.size() * sizeof(float)) != 0) return 47;
    if (d_lens == d_none) return 48;  // the lens is applied
    double sum = 0;
    for (float v : d_lens) sum += v;
    if (!(sum > 0)) return 49;

    try {  // a camera that already holds a table, and a lens
        EMVS::MapperEMVS both(ctx, cam_a, dsi::lens_of(a), shape);
        return 50;
    } catch (const dsi::Error& e) {
        if (e.code != DSI_ERR_INVALID) return 51;
    }
    std::printf("OK\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_rectify --lens-of | DIR\n");
        return 2;
    }
    try {
        return std::string(argv[1]) == "--lens-of" ? lens_of_mode() : gpu_mode(argv[1]);
    } catch (const dsi::Error& e) {
        std::printf("dsi::Error %d: %s\n", e.code, e.what());
        return e.code == DSI_ERR_NO_DEVICE ? 3 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
