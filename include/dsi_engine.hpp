// dsi_engine.hpp -- header-only C++ adapter over the C ABI (dsi_engine.h) that re-creates
// the reference's class and method names on the hot path, so that the reference's
// process_1 / process_2 orchestration (process1.cpp, process2.cpp) can call the GPU engine
// with the code it already has:
//
//   Grid3D                       cartesian3dgrid/include/cartesian3dgrid/cartesian3dgrid.h:22-247
//   EMVS::ShapeDSI               mapper_emvs_stereo/include/mapper_emvs_stereo/mapper_emvs_stereo.hpp:40-65
//   EMVS::MapperEMVS             mapper_emvs_stereo.hpp:94-155
//   LinearTrajectory             mapper_emvs_stereo/include/mapper_emvs_stereo/trajectory.hpp:81-128
//
// Types the reference takes from third-party packages are replaced by plain structs:
//   dvs_msgs::Event                      -> dsi::Event {x, y, ts (seconds), polarity}
//   geometry_utils::Transformation       -> dsi::Transformation {t[3], q[4] = w,x,y,z}
//   image_geometry::PinholeCameraModel   -> dsi::PinholeCameraModel {width,height,fx,fy,cx,cy,lut}; its K, D, R, P ->
//                                           dsi::Lens (the table is then made on the device)
//   cv::Mat (CV_32F / CV_8U)             -> cv::Mat itself (anything with create / ptr<T> / isContinuous / release, see
//                                           image_create below), or dsi::Image<float> / dsi::Image<uint8_t>
// Where the reference glog-CHECK-aborts or throws std::out_of_range this adapter throws
// dsi::Error (carrying the C status code).
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dsi_engine.h"
#include "dsi_map_eval.h"
#include "dsi_map_components.h"
#include "dsi_map_knn.h"
#include "dsi_map_pca.h"
#include "dsi_map_visibility.h"
#include "dsi_map_prune.h"
#include "dsi_map_merge.h"
#include "dsi_map_align.h"

namespace dsi {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc)
{
    if (rc != DSI_OK) throw Error(rc, dsi_last_error());
}

struct Event {  // fields MapperEMVS reads from dvs_msgs::Event (mapper_emvs_stereo.cpp:91,131,134)
    uint16_t x = 0, y = 0;
    double ts = 0;  // seconds
    bool polarity = false;
};

struct Transformation {  // T_A_B as translation + unit quaternion (w,x,y,z)
    double t[3] = {0, 0, 0};
    double q[4] = {1, 0, 0, 0};
    void to7(double* p) const
    {
        p[0] = t[0]; p[1] = t[1]; p[2] = t[2];
        p[3] = q[0]; p[4] = q[1]; p[5] = q[2]; p[6] = q[3];
    }
    static Transformation from7(const double* p)
    {
        Transformation T;
        T.t[0] = p[0]; T.t[1] = p[1]; T.t[2] = p[2];
        T.q[0] = p[3]; T.q[1] = p[4]; T.q[2] = p[5]; T.q[3] = p[6];
        return T;
    }
};

struct PinholeCameraModel {
    int width = 0, height = 0;      // fullResolution()
    float fx = 0, fy = 0, cx = 0, cy = 0;  // projection-matrix intrinsics (mapper_emvs_stereo.cpp:46-48)
    std::vector<float> rectified_points;   // optional LUT, 2*W*H, entry y*W+x (precomputeRectifiedPoints)
};

template <typename T>
struct Image {  // a single-channel image of T when the caller has no cv::Mat
    int rows = 0, cols = 0;
    std::vector<T> data;
    Image() = default;
    Image(int r, int c) : rows(r), cols(c), data((size_t)r * c) {}
    T& at(int y, int x) { return data[(size_t)y * cols + x]; }
    const T& at(int y, int x) const { return data[(size_t)y * cols + x]; }
};

// How the image-typed OUTPUTS of the path (Grid3D::collapseMaxZSlice, cartesian3dgrid.h:207; MapperEMVS::getDepthMapFromDSI,
// mapper_emvs_stereo.hpp:108-109) are written into the caller's image type -- the reference's is cv::Mat.  Every such
// member of this header is a template over the image type and goes through these three customisation points:
//   image_create<T>(img, rows, cols)  make img a rows x cols single-channel image of T, return its first pixel
//                                     (rows * cols contiguous elements)
//   image_data<T>(img)                first pixel of an existing image of T
//   image_release(img)                make img empty (cv::Mat() / Image<T>())
// Defaults: dsi::Image<T>, and any type with OpenCV's Mat members create(rows, cols, type), ptr<T>(row),
// isContinuous(), release() -- i.e. cv::Mat itself, with no OpenCV header needed here: the depth codes are the
// constants of <opencv2/core/hal/interface.h> (CV_8U 0, CV_32F 5; a single channel's type IS its depth code).
// Overload them (in the image type's namespace, or in namespace dsi before this header) for anything else.
template <typename T> struct cv_depth;
template <> struct cv_depth<uint8_t> { enum { value = 0 }; };  // CV_8U
template <> struct cv_depth<float> { enum { value = 5 }; };    // CV_32F

template <typename T>
inline T* image_create(Image<T>& img, int rows, int cols)
{
    img = Image<T>(rows, cols);
    return img.data.data();
}
template <typename T, typename ImgT>
inline auto image_create(ImgT& img, int rows, int cols)
    -> decltype(img.create(rows, cols, 0), img.isContinuous(), img.template ptr<T>(0))
{
    img.create(rows, cols, (int)cv_depth<T>::value);  // cv::Mat::create: a fresh matrix is continuous
    if (!img.isContinuous()) throw Error(DSI_ERR_INVALID, "image_create: the image type returned non-contiguous rows");
    return img.template ptr<T>(0);
}
template <typename T>
inline T* image_data(Image<T>& img)
{
    return img.data.data();
}
template <typename T, typename ImgT>
inline auto image_data(ImgT& img) -> decltype(img.isContinuous(), img.template ptr<T>(0))
{
    if (!img.isContinuous()) throw Error(DSI_ERR_INVALID, "image_data: non-contiguous image");
    return img.template ptr<T>(0);
}
template <typename T>
inline void image_release(Image<T>& img)
{
    img = Image<T>();
}
template <typename ImgT>
inline auto image_release(ImgT& img) -> decltype(img.release(), void())
{
    img.release();
}

// Customisation point for depth_map_dense, the 5th argument of getDepthMapFromDSI (mapper_emvs_stereo.cpp:430-436):
//     cv::Mat inpaint_mask = 1 - mask;
//     cv::inpaint(depth_cell_indices_filtered, inpaint_mask, depth_cell_indices_inpainted, 3, cv::INPAINT_TELEA);
// Telea's fast-marching inpainting is OpenCV arithmetic (photo module) and stays on the host side of the boundary, like
// the rectification of fisheye cameras above.  A maintainer with OpenCV adds, in namespace cv or in namespace dsi
// before this header,
//     inline bool inpaint_depth_cell_indices(const cv::Mat& filtered, const cv::Mat& inpaint_mask, cv::Mat& inpainted)
//     { cv::inpaint(filtered, inpaint_mask, inpainted, 3, cv::INPAINT_TELEA); return true; }
// and getDepthMapFromDSI then fills depth_map_dense with convertDepthIndicesToValues of the result (:436).  The default
// returns false: depth_map_dense is left EMPTY (image_release), never a guess.
template <typename ImgT>
inline bool inpaint_depth_cell_indices(const ImgT& /*filtered u8*/, const ImgT& /*inpaint_mask u8 = 1 - mask*/,
                                       ImgT& /*inpainted u8*/)
{
    return false;
}

// Customisation point for Grid3D::imwriteSlices (cartesian3dgrid_IO.cpp:74: imwrite(ss.str(), slice_u)).  The default
// writes an 8-bit grayscale PNG with a minimal encoder of its own -- signature, IHDR, one IDAT whose zlib stream holds
// STORED deflate blocks (no compression), every scanline with filter type 0, IEND; CRC-32 per chunk, Adler-32 of the raw
// scanlines -- because neither libpng nor OpenCV may be assumed here.  Any PNG reader decodes it to the pixels written.  A
// caller with OpenCV adds, in namespace cv or in namespace dsi before this header,
//     inline bool imwrite_gray8(const std::string& path, const cv::Mat& img) { return cv::imwrite(path, img); }
// and calls imwriteSlices<cv::Mat>(...): the overload is found by ADL and wins over this template.
// write_png_rgb8 is its colour twin (colour type 2) for OpenCV-ordered pixels: B G R in memory, swapped to R G B on writing.
inline bool write_png8(const std::string& path, const uint8_t* pixels, int rows, int cols, int channels)
{
    if (!pixels || rows < 1 || cols < 1 || (channels != 1 && channels != 3)) return false;
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t n = 0; n < 256; ++n) {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[n] = c;
        }
        return t;
    }();
    auto be32 = [](std::vector<uint8_t>& v, uint32_t x) {
        for (int sh = 24; sh >= 0; sh -= 8) v.push_back((uint8_t)(x >> sh));
    };
    auto chunk = [&](std::vector<uint8_t>& file, const char kind[4], const std::vector<uint8_t>& body) {
        be32(file, (uint32_t)body.size());
        const size_t start = file.size();
        file.insert(file.end(), kind, kind + 4);
        file.insert(file.end(), body.begin(), body.end());
        uint32_t c = 0xffffffffu;
        for (size_t i = start; i < file.size(); ++i) c = table[(c ^ file[i]) & 0xffu] ^ (c >> 8);
        be32(file, c ^ 0xffffffffu);
    };
    std::vector<uint8_t> raw;  // the scanlines, each behind its filter byte
    const size_t pitch = (size_t)cols * channels;
    raw.reserve((size_t)rows * (pitch + 1));
    for (int y = 0; y < rows; ++y) {
        raw.push_back(0);
        const uint8_t* row = pixels + (size_t)y * pitch;
        if (channels == 1) {
            raw.insert(raw.end(), row, row + pitch);
        } else {
            for (int x = 0; x < cols; ++x)
                for (int k = 2; k >= 0; --k) raw.push_back(row[3 * x + k]);
        }
    }
    std::vector<uint8_t> z = {0x78, 0x01};  // zlib header: deflate, 32 KiB window, no preset dictionary
    uint32_t a = 1, b = 0;
    for (size_t pos = 0; pos < raw.size();) {
        const size_t len = std::min<size_t>(65535, raw.size() - pos);
        z.push_back(pos + len == raw.size() ? 1 : 0);  // BFINAL, BTYPE = 00 (stored)
        z.push_back((uint8_t)(len & 0xff));
        z.push_back((uint8_t)(len >> 8));
        z.push_back((uint8_t)(~len & 0xff));
        z.push_back((uint8_t)((~len >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + (long)pos, raw.begin() + (long)(pos + len));
        for (size_t i = pos; i < pos + len; ++i) {
            a = (a + raw[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        pos += len;
    }
    be32(z, (b << 16) | a);
    std::vector<uint8_t> file = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<uint8_t> ihdr;
    be32(ihdr, (uint32_t)cols);
    be32(ihdr, (uint32_t)rows);
    // bit depth 8, colour type 0 (grayscale) or 2 (truecolour), deflate, adaptive filtering, no interlace
    const uint8_t rest[5] = {8, (uint8_t)(channels == 3 ? 2 : 0), 0, 0, 0};
    ihdr.insert(ihdr.end(), rest, rest + 5);
    chunk(file, "IHDR", ihdr);
    chunk(file, "IDAT", z);
    chunk(file, "IEND", std::vector<uint8_t>());
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(file.data(), 1, file.size(), f) == file.size();
    return (std::fclose(f) == 0) && ok;
}
inline bool write_png_gray8(const std::string& path, const uint8_t* pixels, int rows, int cols)
{
    return write_png8(path, pixels, rows, cols, 1);
}
inline bool write_png_rgb8(const std::string& path, const uint8_t* pixels_bgr, int rows, int cols)
{
    return write_png8(path, pixels_bgr, rows, cols, 3);
}
template <typename ImgT>
inline bool imwrite_gray8(const std::string& path, const ImgT& img)
{
    return write_png_gray8(path, dsi::image_data<uint8_t>(const_cast<ImgT&>(img)), img.rows, img.cols);
}

// The point cloud of MapperEMVS::getPointcloud (mapper_emvs_stereo.cpp:440-480): pcl::PointXYZI's four fields, and a
// default cloud with the members of pcl::PointCloud<PointT> the reference's callers use (points, width, height, clear,
// push_back, size, Ptr) -- no PCL header needed here.
struct PointXYZI {
    float x, y, z, intensity;
};
struct PointCloud {
    typedef std::shared_ptr<PointCloud> Ptr;
    std::vector<PointXYZI> points;
    uint32_t width = 0, height = 0;  // unorganised: width = size(), height = 1 once it holds points
    void clear()
    {
        points.clear();
        width = height = 0;
    }
    void push_back(const PointXYZI& p)
    {
        points.push_back(p);
        width = (uint32_t)points.size();
        height = 1;
    }
    size_t size() const { return points.size(); }
};

// Customisation point: how the n points (x, y, z, intensity) of the engine's cloud are written into the caller's cloud
// type.  Defaults: dsi::PointCloud and any pcl-like PointCloud<PointT> (points, clear(), width, height; PointT with
// x y z intensity), and a smart pointer to either (Ptr: created when empty, then filled through it).  Overload it (in
// the cloud type's namespace, or in namespace dsi before this header) for anything else.
template <typename CloudT>
inline auto point_cloud_assign(CloudT& cloud, const PointXYZI* p, size_t n)
    -> decltype(cloud.clear(), cloud.points.resize(n), cloud.width = 0u, cloud.height = 0u, void())
{
    cloud.clear();
    cloud.points.resize(n);
    for (size_t i = 0; i < n; ++i) {
        cloud.points[i].x = p[i].x;
        cloud.points[i].y = p[i].y;
        cloud.points[i].z = p[i].z;
        cloud.points[i].intensity = p[i].intensity;
    }
    cloud.width = (uint32_t)n;  // pcl::PointCloud::push_back's bookkeeping
    cloud.height = 1;
}
template <typename PtrT>
inline auto point_cloud_assign(PtrT& cloud, const PointXYZI* p, size_t n)
    -> decltype(cloud.reset(new typename PtrT::element_type), void())
{
    if (!cloud) cloud.reset(new typename PtrT::element_type);
    point_cloud_assign(*cloud, p, n);
}

// One GPU + one stream; shared by every Grid3D / MapperEMVS created from it.
class Context {
public:
    explicit Context(int device = 0) { check(dsi_context_create(device, &h_)); }
    ~Context()
    {
        // the C side refuses (and destroys nothing) while grids, mappers or batches of this context are alive: a wrong
        // destruction order would be a silent, permanent leak of the stream, the pool and the scratch -- say so
        if (dsi_context_destroy(h_) != DSI_OK) std::fprintf(stderr, "dsi::Context: NOT destroyed: %s\n", dsi_last_error());
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    dsi_context_t* handle() const { return h_; }
    void wait_for(Context& other) { check(dsi_context_wait_for(h_, other.h_)); }
    void synchronize() { check(dsi_context_synchronize(h_)); }

private:
    dsi_context_t* h_ = nullptr;
};

// The reference's classes are constructed without a device argument (MapperEMVS(cam, shape),
// Grid3D(dimX, dimY, dimZ): mapper_emvs_stereo.hpp:101, cartesian3dgrid.h:26).  Those arities use this
// process-wide context: GPU `DSI_DEVICE` (environment, default 0), created on first use.
inline Context& default_context()
{
    static Context ctx([] {
        const char* e = std::getenv("DSI_DEVICE");
        return e ? std::atoi(e) : 0;
    }());
    return ctx;
}

// How the reference's third-party value types are read.  Specialise (or overload) for other types;
// the defaults cover: timestamps that are a double or have .toSec() (ros::Time), poses that are a
// dsi::Transformation or have getPosition() / getRotation().w() ... (kindr::minimal::QuatTransformation,
// the reference's geometry_utils::Transformation), cameras that are a dsi::PinholeCameraModel or
// have fullResolution() / fx() / fy() / cx() / cy() (image_geometry::PinholeCameraModel).
inline double to_seconds(double t) { return t; }
template <typename TimeT>
inline auto to_seconds(const TimeT& t) -> decltype(t.toSec())
{
    return t.toSec();
}

inline void to_pose7(const Transformation& T, double* p) { T.to7(p); }
template <typename PoseT>
inline auto to_pose7(const PoseT& T, double* p) -> decltype(T.getRotation().w(), void())
{
    const auto pos = T.getPosition();
    const auto rot = T.getRotation();
    p[0] = pos[0]; p[1] = pos[1]; p[2] = pos[2];
    p[3] = rot.w(); p[4] = rot.x(); p[5] = rot.y(); p[6] = rot.z();
}

inline void camera_of(const PinholeCameraModel& c, PinholeCameraModel* out) { *out = c; }

// The distortion model the reference reads from cam.cameraInfo().distortion_model
// (mapper_emvs_stereo.cpp:62): "plumb_bob" -> rectifyPoint, "fisheye" -> fisheye_rectifyPoint =
// cv::fisheye::undistortPoints(K, D, R, P) (:243-254, :256-299).  A camera type without cameraInfo() is taken as
// plumb_bob (image_geometry's default model).  Both models are computed by the engine itself from K, D, R, P --
// dsi::lens_of(cam) reads them, camera_of(ctx, cam, &out) / rectified_points / MapperEMVS(ctx, cam, lens, shape) make the
// table on the device, no OpenCV needed; camera_of(cam, &out) without a context is the older path that
// calls the camera's own rectifyPoint on the host.
template <typename CamT>
inline auto distortion_model_of(const CamT& c, int) -> decltype(std::string(c.cameraInfo().distortion_model))
{
    return std::string(c.cameraInfo().distortion_model);
}
template <typename CamT>
inline std::string distortion_model_of(const CamT&, long)
{
    return "plumb_bob";
}

// Customisation point of the host path camera_of(cam, &out) for fisheye cameras (the device path, camera_of(ctx, cam,
// &out), needs none: the engine has the Kannala-Brandt inverse).  A caller who wants OpenCV's own binary
// to make the table overloads this for its camera type -- in that type's namespace (camera_of finds it by
// argument-dependent lookup) or in namespace dsi before this header -- with the reference's own four lines --
//   cv::Point2f raw32(x, y), rect32;  cv::fisheye::undistortPoints(src(raw32), dst(rect32), c.intrinsicMatrix(),
//   c.distortionCoeffs(), c.rotationMatrix(), c.fullProjectionMatrix());  *u = rect32.x; *v = rect32.y;
// (mapper_emvs_stereo.cpp:243-254).  The default refuses: a plumb_bob LUT for a fisheye lens would shift
// every vote without any error being reported.
template <typename CamT>
inline void fisheye_rectify_point(const CamT&, double, double, double*, double*)
{
    throw Error(DSI_ERR_INVALID,
                "fisheye distortion model: overload dsi::fisheye_rectify_point for this camera type "
                "(cv::fisheye::undistortPoints with K, D, R, P, mapper_emvs_stereo.cpp:243-254), or build the "
                "rectification LUT yourself and pass a dsi::PinholeCameraModel");
}

template <typename CamT>
inline auto camera_of(const CamT& c, PinholeCameraModel* out) -> decltype(c.fullResolution(), void())
{
    // mapper_emvs_stereo.cpp:34-48: size from fullResolution(), K from the projection matrix
    out->width = c.fullResolution().width;
    out->height = c.fullResolution().height;
    out->fx = (float)c.fx();
    out->fy = (float)c.fy();
    out->cx = (float)c.cx();
    out->cy = (float)c.cy();
    // precomputeRectifiedPoints (mapper_emvs_stereo.cpp:256-299): raw pixel -> rectified pixel by the model
    // the camera declares (OpenCV arithmetic stays on the host side of the boundary)
    const std::string model = distortion_model_of(c, 0);
    const bool plumb_bob = model == "plumb_bob", fisheye = model == "fisheye";
    if (!plumb_bob && !fisheye)  // the reference logs "Distortion model not set properly!" and goes on with an
                                 // uninitialised table (:289-293); here the caller gets to know
        throw Error(DSI_ERR_INVALID, "Distortion model not set properly: '" + model + "' (expected plumb_bob or fisheye)");
    out->rectified_points.resize((size_t)2 * out->width * out->height);
    for (int y = 0; y < out->height; ++y)
        for (int x = 0; x < out->width; ++x) {
            double u, v;
            if (plumb_bob) {
                const auto r = c.rectifyPoint(decltype(c.rectifyPoint({}))((double)x, (double)y));
                u = r.x;
                v = r.y;
            } else {
                fisheye_rectify_point(c, (double)x, (double)y, &u, &v);
            }
            out->rectified_points[2 * ((size_t)y * out->width + x)] = (float)u;
            out->rectified_points[2 * ((size_t)y * out->width + x) + 1] = (float)v;
        }
}

// ---- lens rectification on the device (dsi_engine.h "lens rectification") ----

// dsi_lens_t with the defaults of a camera without a rectifying pair: plumb_bob, no coefficients, R = I.  K and P are the
// caller's (set_K fills P = [K | 0] as well).  All matrices row-major, as in sensor_msgs::CameraInfo.
struct Lens : dsi_lens_t {
    Lens() : dsi_lens_t{}
    {
        model = DSI_LENS_PLUMB_BOB;
        R[0] = R[4] = R[8] = 1.0;
    }
    Lens& set_K(double fx, double fy, double cx, double cy)
    {
        const double k[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) P[4 * i + j] = j < 3 ? k[3 * i + j] : 0.0;
        std::copy(k, k + 9, K);
        return *this;
    }
    Lens& set_D(const std::vector<double>& d)
    {
        if (d.size() > 8) throw Error(DSI_ERR_INVALID, "Lens: at most 8 distortion coefficients");
        std::fill(D, D + 8, 0.0);
        std::copy(d.begin(), d.end(), D);
        n_dist = (int)d.size();
        return *this;
    }
    void check() const { dsi::check(dsi_lens_check(this)); }
    std::string model_name() const { return model == DSI_LENS_FISHEYE ? "fisheye" : model == DSI_LENS_PLUMB_BOB ? "plumb_bob" : "?"; }
};

// How lens_of reads the camera's matrices: element (r, c) of K, R, P and the count / the i-th of the distortion
// coefficients.  Defaults, tried in this order: m(r, c) (cv::Matx, cv::Mat_<double>, Eigen), m.at<double>(r, c) (cv::Mat of
// CV_64F); d.total() (cv::Mat), d.size() (std::vector, Eigen); d(i) (cv::Mat_<double>, Eigen), d[i] (std::vector),
// d.at<double>(i).  Overload lens_element / lens_count / lens_coefficient for anything else (in the matrix type's
// namespace, or in namespace dsi before this header).  No OpenCV header is needed here.
namespace detail {
template <int N> struct prio : prio<N - 1> {};
template <> struct prio<0> {};
template <typename M>
inline auto element(const M& m, int r, int c, prio<1>) -> decltype((double)m(r, c)) { return (double)m(r, c); }
template <typename M>
inline auto element(const M& m, int r, int c, prio<0>) -> decltype((double)m.template at<double>(r, c))
{
    return (double)m.template at<double>(r, c);
}
template <typename V>
inline auto count(const V& d, prio<1>) -> decltype((size_t)d.total()) { return (size_t)d.total(); }
template <typename V>
inline auto count(const V& d, prio<0>) -> decltype((size_t)d.size()) { return (size_t)d.size(); }
template <typename V>
inline auto coefficient(const V& d, int i, prio<2>) -> decltype((double)d(i)) { return (double)d(i); }
template <typename V>
inline auto coefficient(const V& d, int i, prio<1>) -> decltype((double)d[i]) { return (double)d[i]; }
template <typename V>
inline auto coefficient(const V& d, int i, prio<0>) -> decltype((double)d.template at<double>(i))
{
    return (double)d.template at<double>(i);
}
}  // namespace detail
template <typename M>
inline auto lens_element(const M& m, int r, int c) -> decltype(detail::element(m, r, c, detail::prio<1>()))
{
    return detail::element(m, r, c, detail::prio<1>());
}
template <typename V>
inline auto lens_count(const V& d) -> decltype(detail::count(d, detail::prio<1>()))
{
    return detail::count(d, detail::prio<1>());
}
template <typename V>
inline auto lens_coefficient(const V& d, int i) -> decltype(detail::coefficient(d, i, detail::prio<2>()))
{
    return detail::coefficient(d, i, detail::prio<2>());
}

// The calibration numbers of a camera type with image_geometry::PinholeCameraModel's accessors: intrinsicMatrix() (K),
// distortionCoeffs() (D), rotationMatrix() (R), fullProjectionMatrix() (P), and the model of distortion_model_of.
template <typename CamT>
inline auto lens_of(const CamT& c) -> decltype(c.intrinsicMatrix(), c.distortionCoeffs(), c.rotationMatrix(), c.fullProjectionMatrix(), Lens())
{
    Lens L;
    const std::string model = distortion_model_of(c, 0);
    if (model == "plumb_bob")
        L.model = DSI_LENS_PLUMB_BOB;
    else if (model == "fisheye")
        L.model = DSI_LENS_FISHEYE;
    else
        throw Error(DSI_ERR_INVALID, "Distortion model not set properly: '" + model + "' (expected plumb_bob or fisheye)");
    const auto& K = c.intrinsicMatrix();
    const auto& D = c.distortionCoeffs();
    const auto& R = c.rotationMatrix();
    const auto& P = c.fullProjectionMatrix();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            L.K[3 * i + j] = lens_element(K, i, j);
            L.R[3 * i + j] = lens_element(R, i, j);
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) L.P[4 * i + j] = lens_element(P, i, j);
    const size_t n = lens_count(D);
    if (n > 8) throw Error(DSI_ERR_INVALID, "lens_of: " + std::to_string(n) + " distortion coefficients (thin-prism and tilt terms are not supported)");
    L.n_dist = (int)n;
    for (size_t i = 0; i < n; ++i) L.D[i] = lens_coefficient(D, (int)i);
    return L;
}

// the table of precomputeRectifiedPoints (2 * width * height floats, entry y * width + x), made on the device
inline std::vector<float> rectified_points(Context& ctx, const Lens& lens, int width, int height)
{
    std::vector<float> lut(width > 0 && height > 0 ? (size_t)2 * width * height : 0);
    check(dsi_rectify_lut(ctx.handle(), &lens, width, height, lut.empty() ? nullptr : lut.data()));
    return lut;
}

// camera_of with the table made by the engine, for both distortion models: never calls the camera's rectifyPoint or
// fisheye_rectify_point
template <typename CamT>
inline auto camera_of(Context& ctx, const CamT& c, PinholeCameraModel* out) -> decltype(c.fullResolution(), lens_of(c), void())
{
    out->width = c.fullResolution().width;
    out->height = c.fullResolution().height;
    out->fx = (float)c.fx();
    out->fy = (float)c.fy();
    out->cx = (float)c.cx();
    out->cy = (float)c.cy();
    out->rectified_points = rectified_points(ctx, lens_of(c), out->width, out->height);
}

// One rank of an RCCL communicator owned by the engine (dsi_engine.h "multi-GPU").
class Comm {
public:
    Comm() = default;
    Comm(Context& ctx, const uint8_t id[DSI_COMM_ID_BYTES], int nranks, int rank)
    {
        check(dsi_comm_create_rank(ctx.handle(), id, nranks, rank, &h_));
    }
    ~Comm() { dsi_comm_destroy(h_); }
    Comm(const Comm&) = delete;
    Comm& operator=(const Comm&) = delete;
    Comm(Comm&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    // one process, several GPUs: one communicator rank per context (distinct devices)
    static std::vector<Comm> createAll(const std::vector<Context*>& ctxs)
    {
        std::vector<dsi_context_t*> hs;
        for (Context* c : ctxs) hs.push_back(c->handle());
        std::vector<dsi_comm_t*> out(ctxs.size(), nullptr);
        check(dsi_comm_create_all(hs.data(), (int)hs.size(), out.data()));
        std::vector<Comm> v(ctxs.size());
        for (size_t i = 0; i < out.size(); ++i) v[i].h_ = out[i];
        return v;
    }
    static void uniqueId(uint8_t id[DSI_COMM_ID_BYTES]) { check(dsi_comm_unique_id(id)); }
    int rank() const { return dsi_comm_rank(h_); }
    int size() const { return dsi_comm_size(h_); }
    dsi_comm_t* handle() const { return h_; }

private:
    dsi_comm_t* h_ = nullptr;
};

}  // namespace dsi

namespace dsi {

// T_a * T_b and T^-1 for (translation, unit quaternion w,x,y,z) -- the two minkindr operations the
// callers need to place the reference view (process1.cpp:56-68, process2.cpp:79-81)
inline void quat_rotate(const double* q, const double* v, double* out)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double ux = 2 * (y * v[2] - z * v[1]), uy = 2 * (z * v[0] - x * v[2]), uz = 2 * (x * v[1] - y * v[0]);
    out[0] = v[0] + w * ux + (y * uz - z * uy);
    out[1] = v[1] + w * uy + (z * ux - x * uz);
    out[2] = v[2] + w * uz + (x * uy - y * ux);
}

inline Transformation operator*(const Transformation& a, const Transformation& b)
{
    Transformation o;
    const double *p = a.q, *r = b.q;
    o.q[0] = p[0] * r[0] - p[1] * r[1] - p[2] * r[2] - p[3] * r[3];
    o.q[1] = p[0] * r[1] + p[1] * r[0] + p[2] * r[3] - p[3] * r[2];
    o.q[2] = p[0] * r[2] + p[2] * r[0] + p[3] * r[1] - p[1] * r[3];
    o.q[3] = p[0] * r[3] + p[3] * r[0] + p[1] * r[2] - p[2] * r[1];
    double rt[3];
    quat_rotate(a.q, b.t, rt);
    for (int i = 0; i < 3; ++i) o.t[i] = a.t[i] + rt[i];
    return o;
}

inline Transformation inverse(const Transformation& T)
{
    Transformation o;
    o.q[0] = T.q[0];
    o.q[1] = -T.q[1];
    o.q[2] = -T.q[2];
    o.q[3] = -T.q[3];
    double rt[3];
    quat_rotate(o.q, T.t, rt);
    for (int i = 0; i < 3; ++i) o.t[i] = -rt[i];
    return o;
}

}  // namespace dsi

// trajectory.hpp:81-128
class LinearTrajectory {
public:
    typedef std::map<double, dsi::Transformation> PoseMap;
    LinearTrajectory() = default;
    // any std::map<TimeT, PoseT> the traits above can read (the reference's
    // std::map<ros::Time, geometry_utils::Transformation>, trajectory.hpp:84)
    template <typename TimeT, typename PoseT, typename... Rest>
    explicit LinearTrajectory(const std::map<TimeT, PoseT, Rest...>& poses)
    {
        if (poses.size() < 2) throw dsi::Error(DSI_ERR_INVALID, "At least two poses need to be provided");
        for (const auto& kv : poses) {
            times_.push_back(dsi::to_seconds(kv.first));
            double p[7];
            dsi::to_pose7(kv.second, p);
            poses_.insert(poses_.end(), p, p + 7);
        }
    }
    // Returns T_W_C; false when t cannot be interpolated (trajectory.hpp:98-113)
    bool getPoseAt(double t, dsi::Transformation& T) const
    {
        double out[7];
        if (dsi_pose_at(times_.data(), poses_.data(), times_.size(), t, out) != DSI_OK) return false;
        T = dsi::Transformation::from7(out);
        return true;
    }
    // the reference's signature getPoseAt(const ros::Time&, Transformation&) for any time type with
    // toSec() and any pose type constructible from (rotation(w,x,y,z), position(x,y,z)) like minkindr's
    template <typename TimeT, typename PoseT>
    auto getPoseAt(const TimeT& t, PoseT& T) const -> decltype(t.toSec(), T.getRotation(), bool())
    {
        dsi::Transformation D;
        if (!getPoseAt(t.toSec(), D)) return false;
        typedef typename std::decay<decltype(T.getRotation())>::type Rot;
        typedef typename std::decay<decltype(T.getPosition())>::type Pos;
        T = PoseT(Rot(D.q[0], D.q[1], D.q[2], D.q[3]), Pos(D.t[0], D.t[1], D.t[2]));
        return true;
    }
    // TrajectoryBase::applyTransformationRight / Left (trajectory.hpp:57-71): every control pose becomes pose * T / T * pose
    // -- how main.cpp:203-216 turns the recorded poses into the left camera's (hand-eye) and the other cameras' (extrinsics)
    void applyTransformationRight(const dsi::Transformation& T)
    {
        for (size_t i = 0; i < times_.size(); ++i) (dsi::Transformation::from7(&poses_[7 * i]) * T).to7(&poses_[7 * i]);
    }
    void applyTransformationLeft(const dsi::Transformation& T)
    {
        for (size_t i = 0; i < times_.size(); ++i) (T * dsi::Transformation::from7(&poses_[7 * i])).to7(&poses_[7 * i]);
    }
    // ... with the reference's pose type (geometry_utils::Transformation)
    template <typename PoseT>
    auto applyTransformationRight(const PoseT& T) -> decltype(T.getRotation(), void())
    {
        double p[7];
        dsi::to_pose7(T, p);
        applyTransformationRight(dsi::Transformation::from7(p));
    }
    template <typename PoseT>
    auto applyTransformationLeft(const PoseT& T) -> decltype(T.getRotation(), void())
    {
        double p[7];
        dsi::to_pose7(T, p);
        applyTransformationLeft(dsi::Transformation::from7(p));
    }
    // TrajectoryBase::getFirstControlPose / getLastControlPose (trajectory.hpp:28-38)
    void getFirstControlPose(dsi::Transformation* T, double* t) const
    {
        if (times_.empty()) throw dsi::Error(DSI_ERR_INVALID, "empty trajectory");
        *t = times_.front();
        *T = dsi::Transformation::from7(&poses_[0]);
    }
    void getLastControlPose(dsi::Transformation* T, double* t) const
    {
        if (times_.empty()) throw dsi::Error(DSI_ERR_INVALID, "empty trajectory");
        *t = times_.back();
        *T = dsi::Transformation::from7(&poses_[7 * (times_.size() - 1)]);
    }
    size_t getNumControlPoses() const { return times_.size(); }
    const std::vector<double>& times() const { return times_; }
    const std::vector<double>& poses7() const { return poses_; }

private:
    std::vector<double> times_, poses_;
};

// cartesian3dgrid.h:22-247, device resident.
class Grid3D {
public:
    Grid3D() = default;
    Grid3D(dsi::Context& ctx, unsigned dimX, unsigned dimY, unsigned dimZ) { allocate(ctx, dimX, dimY, dimZ); }
    // the reference's arity (cartesian3dgrid.h:26), on the process-wide default context
    Grid3D(unsigned dimX, unsigned dimY, unsigned dimZ) { allocate(dsi::default_context(), dimX, dimY, dimZ); }
    ~Grid3D() { deallocate(); }
    Grid3D(const Grid3D&) = delete;
    Grid3D& operator=(const Grid3D&) = delete;
    Grid3D(Grid3D&& o) noexcept : h_(o.h_), owned_(o.owned_) { o.h_ = nullptr; }
    Grid3D& operator=(Grid3D&& o) noexcept
    {
        if (this != &o) {
            deallocate();
            h_ = o.h_;
            owned_ = o.owned_;
            o.h_ = nullptr;
        }
        return *this;
    }

    void allocate(dsi::Context& ctx, unsigned dimX, unsigned dimY, unsigned dimZ)
    {
        deallocate();
        dsi::check(dsi_grid_create(ctx.handle(), (int)dimX, (int)dimY, (int)dimZ, &h_));
        owned_ = true;
    }
    void deallocate()
    {
        if (h_ && owned_) dsi_grid_destroy(h_);
        h_ = nullptr;
    }
    // non-owning view of a grid that belongs to a mapper (MapperEMVS::dsi_)
    static Grid3D view(dsi_grid_t* h)
    {
        Grid3D g;
        g.h_ = h;
        g.owned_ = false;
        return g;
    }
    dsi_grid_t* handle() const { return h_; }

    void getDimensions(int* dimX, int* dimY, int* dimZ) const { dsi::check(dsi_grid_dims(h_, dimX, dimY, dimZ)); }
    void resetGrid() { dsi::check(dsi_grid_reset(h_)); }

    // voxel-wise operations, same names and in-place semantics as cartesian3dgrid.h:64-192
    void addTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_accumulate(h_, grid2.h_, DSI_ACC_SUM)); }
    void addInverseOfTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_accumulate(h_, grid2.h_, DSI_ACC_INV_SUM)); }
    void computeHMfromSumOfInv(int n) { dsi::check(dsi_grid_finalize(h_, DSI_ACC_INV_SUM, n)); }
    void computeAMfromSum(int n) { dsi::check(dsi_grid_finalize(h_, DSI_ACC_SUM, n)); }
    void minTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_fuse2(h_, grid2.h_, DSI_FUSE_MIN)); }
    void harmonicMeanTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_fuse2(h_, grid2.h_, DSI_FUSE_HM)); }
    void harmonicMeanTwoGrids(const Grid3D& grid2, int n) { dsi::check(dsi_grid_fuse_hm_n(h_, grid2.h_, n)); }
    void rmsTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_fuse2(h_, grid2.h_, DSI_FUSE_RMS)); }
    void geometricMeanTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_fuse2(h_, grid2.h_, DSI_FUSE_GM)); }
    void arithmeticMeanTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_fuse2(h_, grid2.h_, DSI_FUSE_AM)); }
    void maxTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_fuse2(h_, grid2.h_, DSI_FUSE_MAX)); }
    // n-ary accumulate / finalize (dsi_acc_mode_t: the temporal accumulators above are modes 0 / 1;
    // LOG_SUM / SQ_SUM / MIN / MAX are the n-ary forms of the 2-ary camera-fusion ops, which the
    // reference lacks) and the all-reduce that joins accumulators across GPUs
    void accumulateBegin(int mode) { dsi::check(dsi_grid_accumulate_begin(h_, mode)); }
    void accumulate(const Grid3D& grid2, int mode) { dsi::check(dsi_grid_accumulate(h_, grid2.h_, mode)); }
    void finalize(int mode, int n) { dsi::check(dsi_grid_finalize(h_, mode, n)); }
    void allReduce(dsi::Comm& comm, int op) { dsi::check(dsi_grid_allreduce(comm.handle(), h_, op)); }

    // void collapseMaxZSlice(cv::Mat* max_val, cv::Mat* max_pos) const (cartesian3dgrid.h:207, cartesian3dgrid.cpp:115-137):
    // max_val becomes dimY x dimX CV_32F, max_pos dimY x dimX CV_8U ("Max 256 depth layers", :120).  Any image type the
    // dsi::image_create customisation point can write: cv::Mat (both arguments), dsi::Image<float> / <uint8_t>.
    template <typename ValImg, typename PosImg>
    void collapseMaxZSlice(ValImg* max_val, PosImg* max_pos) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        float* val = dsi::image_create<float>(*max_val, ny, nx);
        uint8_t* pos = dsi::image_create<uint8_t>(*max_pos, ny, nx);
        dsi::check(dsi_grid_collapse_max_z(h_, val, pos));
    }
    // The focus-based collapses (cartesian3dgrid.h:208-216, cartesian3dgrid.cpp:139-414) with the reference's names and
    // arities; outputs as collapseMaxZSlice's.  Arithmetic: DESIGN.md "Focus-based collapses".
    template <typename ValImg, typename PosImg>
    void collapseMinZSlice(ValImg* min_val, PosImg* min_pos) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        float* val = dsi::image_create<float>(*min_val, ny, nx);
        uint8_t* pos = dsi::image_create<uint8_t>(*min_pos, ny, nx);
        dsi::check(dsi_grid_collapse_min_z(h_, val, pos));
    }
    template <typename ValImg, typename PosImg>
    void collapseZSliceByGradMag(ValImg* confidence, PosImg* depth_cell_indices, int half_patchsize = 1)
    {
        collapseFocus(DSI_FOCUS_GRAD_MAG, half_patchsize, confidence, depth_cell_indices);
    }
    template <typename ValImg, typename PosImg>
    void collapseZSliceByLaplacianMag(ValImg* confidence, PosImg* depth_cell_indices)
    {
        collapseFocus(DSI_FOCUS_LAPLACIAN, 1, confidence, depth_cell_indices);
    }
    template <typename ValImg, typename PosImg>
    void collapseZSliceByDoG(ValImg* confidence, PosImg* depth_cell_indices)
    {
        collapseFocus(DSI_FOCUS_DOG, 1, confidence, depth_cell_indices);
    }
    template <typename ValImg, typename PosImg>
    void collapseZSliceByLocalVar(ValImg* confidence, PosImg* depth_cell_indices)
    {
        collapseFocus(DSI_FOCUS_LOCAL_VAR, 1, confidence, depth_cell_indices);
    }
    template <typename ValImg, typename PosImg>
    void collapseZSliceByLocalMeanSquare(ValImg* confidence, PosImg* depth_cell_indices)
    {
        collapseFocus(DSI_FOCUS_LOCAL_MS, 1, confidence, depth_cell_indices);
    }
    // cartesian3dgrid.cpp:417-429: focus_method 1 the local mean square, any other value the local standard deviation
    void computeLocalFocusInPlace(int focus_method) { dsi::check(dsi_grid_local_focus(h_, h_, focus_method)); }
    // this = grid2 after computeLocalFocusInPlace(focus_method), in one pass (not in the reference)
    void setToLocalFocusOf(const Grid3D& grid2, int focus_method) { dsi::check(dsi_grid_local_focus(h_, grid2.h_, focus_method)); }
    // this = op(a, b) in one pass: resetGrid(); addTwoGrids(a); <op>TwoGrids(b) (not in the reference)
    void setToFusionOf(const Grid3D& a, const Grid3D& b, int op) { dsi::check(dsi_grid_fuse2_into(h_, a.h_, b.h_, op)); }
    // the voxel-wise members that are no camera fusion (cartesian3dgrid.h:95-109,166-184; arithmetic: DESIGN.md 7d)
    void subtractTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_binary_op(h_, grid2.h_, DSI_GRID_OP_SUBTRACT)); }
    // only the reference's default eps is offered: any other value throws DSI_ERR_INVALID
    void ratioTwoGrids(const Grid3D& grid2, const float eps = 1e-1)
    {
        if (eps != 1e-1f) throw dsi::Error(DSI_ERR_INVALID, "ratioTwoGrids: only the default eps = 1e-1 is supported");
        dsi::check(dsi_grid_binary_op(h_, grid2.h_, DSI_GRID_OP_RATIO));
    }
    void quadraticMeanTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_binary_op(h_, grid2.h_, DSI_GRID_OP_QUADRATIC_MEAN)); }
    void cubicMeanTwoGrids(const Grid3D& grid2) { dsi::check(dsi_grid_binary_op(h_, grid2.h_, DSI_GRID_OP_CUBIC_MEAN)); }

    // single voxels (cartesian3dgrid.h:40-58); an index outside the grid throws DSI_ERR_INVALID where .at() throws
    float getGridValueAt(const unsigned int ix, const unsigned int iy, const unsigned int iz) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        if (ix >= (unsigned)nx || iy >= (unsigned)ny || iz >= (unsigned)nz) throw dsi::Error(DSI_ERR_INVALID, "getGridValueAt: outside the grid");
        return getGridValueAt64((uint64_t)ix + (uint64_t)nx * ((uint64_t)iy + (uint64_t)ny * iz));
    }
    float getGridValueAt(const unsigned int p) const { return getGridValueAt64(p); }
    void accumulateGridValueAt(const unsigned int p, const float fval) { dsi::check(dsi_grid_accumulate_value_at(h_, p, fval)); }
    void setGridValueAt(const unsigned int p, const float fval) { dsi::check(dsi_grid_set_value_at(h_, p, fval)); }

    // void accumulateZSliceAt(const unsigned int iz, const cv::Mat& img) (cartesian3dgrid.h:195-204): a float image no larger
    // than the plane, of any type dsi::image_data reads (members rows, cols)
    template <typename Img>
    void accumulateZSliceAt(const unsigned int iz, const Img& img)
    {
        dsi::check(dsi_grid_accumulate_z_slice(h_, iz, dsi::image_data<float>(const_cast<Img&>(img)), img.rows, img.cols));
    }
    // cv::Mat getSlice(sliceIdx, dimIdx) const (cartesian3dgrid.cpp:72-113): getSlice<cv::Mat>(...) for the reference's type
    template <typename Img = dsi::Image<float>>
    Img getSlice(const unsigned int sliceIdx, const unsigned int dimIdx) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        if (dimIdx > 2) throw dsi::Error(DSI_ERR_INVALID, "dimIdx should be 0, 1 or 2");
        Img slice;
        float* px = dsi::image_create<float>(slice, dimIdx == 1 ? nx : ny, dimIdx == 2 ? nx : nz);
        dsi::check(dsi_grid_get_slice(h_, sliceIdx, dimIdx, px));
        return slice;
    }
    // cartesian3dgrid.cpp:177-188
    void getMinMax(float* min_val, float* max_val, unsigned long* min_pos = NULL, unsigned long* max_pos = NULL) const
    {
        uint64_t lo = 0, hi = 0;
        dsi::check(dsi_grid_min_max(h_, min_val, max_val, &lo, &hi));
        if (min_pos != NULL) *min_pos = (unsigned long)lo;
        if (max_pos != NULL) *max_pos = (unsigned long)hi;
    }
    // every slice of one orientation as 8-bit images, slice after slice (what imwriteSlices computes before it writes)
    std::vector<uint8_t> slicesU8(const unsigned int dimIdx, bool normalize_by_minmax = true) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        std::vector<uint8_t> v((size_t)nx * ny * nz);
        dsi::check(dsi_grid_slices_u8(h_, dimIdx, normalize_by_minmax ? 1 : 0, v.data()));
        return v;
    }
    // cartesian3dgrid_IO.cpp:39-76: prefix + three-digit zero-padded slice index + ".png", 8-bit grayscale, through the
    // dsi::imwrite_gray8 customisation point (imwriteSlices<cv::Mat> + an overload for cv::Mat routes to cv::imwrite)
    template <typename Img = dsi::Image<uint8_t>>
    void imwriteSlices(const char prefix[], const unsigned int dimIdx, bool normalize_by_minmax = true) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        const std::vector<uint8_t> all = slicesU8(dimIdx, normalize_by_minmax);
        const int n_slices = dimIdx == 0 ? nx : (dimIdx == 1 ? ny : nz);
        const int rows = dimIdx == 1 ? nx : ny, cols = dimIdx == 2 ? nx : nz;
        for (int i = 0; i < n_slices; ++i) {
            Img slice_u;
            uint8_t* px = dsi::image_create<uint8_t>(slice_u, rows, cols);
            std::copy(all.begin() + (size_t)i * rows * cols, all.begin() + (size_t)(i + 1) * rows * cols, px);
            char num[16];
            std::snprintf(num, sizeof num, "%03d", i);  // std::setfill('0') << std::setw(3)
            using dsi::imwrite_gray8;
            if (!imwrite_gray8(std::string(prefix) + num + ".png", slice_u))
                throw dsi::Error(DSI_ERR_INVALID, std::string("imwriteSlices: cannot write ") + prefix + num + ".png");
        }
    }
    // cartesian3dgrid.cpp:164-174
    double computeMeanSquare() const
    {
        double v = 0;
        dsi::check(dsi_grid_mean_square(h_, &v));
        return v;
    }
    // cartesian3dgrid_filter.cpp and gaussianiir3d.h:27-29 (spellings and defaults); DESIGN.md 7i
    void smoothInPlace(const float sigma = 1.f) { dsi::check(dsi_grid_smooth_diffuse(h_, sigma, NULL)); }
    void smoothInPlaceIIR3D(const float sigma_x = 1.f, const float sigma_y = 1.f, const float sigma_z = 1.f)
    {
        dsi::check(dsi_grid_smooth_iir(h_, sigma_x, sigma_y, sigma_z, 3));  // cartesian3dgrid_filter.cpp:11
    }
    void laplacianInPlace() { dsi::check(dsi_grid_laplacian(h_)); }
    double computeMoranIndexGaussianWeights(float sigma) const
    {
        double v = 0;
        dsi::check(dsi_grid_moran_index(h_, sigma, &v));
        return v;
    }
    // the reference declares and calls it but never defines it: mean and population deviation, two passes, in double
    void computeMeanStd(double* mean, double* stddev) const { dsi::check(dsi_grid_mean_std(h_, mean, stddev)); }
    // host copies (the reference exposes raw pointers via getPointerToSlice; device memory
    // cannot be handed out like that, dsi_grid_device_ptr() is the device-side equivalent)
    std::vector<float> download() const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        std::vector<float> v((size_t)nx * ny * nz);
        dsi::check(dsi_grid_download(h_, v.data()));
        return v;
    }
    void upload(const std::vector<float>& v) { dsi::check(dsi_grid_upload(h_, v.data())); }

    // Grid3D::writeGridNpy (cartesian3dgrid_IO.cpp:30-36): NumPy .npy v1.0, little-endian float32,
    // C order, shape (dimZ, dimY, dimX) -- what scripts/visualize_dsi_*.py load.  Returns 0 on success.
    int writeGridNpy(const char* filename) const
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        const std::vector<float> v = download();
        std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(nz) + ", " +
                           std::to_string(ny) + ", " + std::to_string(nx) + "), }";
        while ((10 + dict.size() + 1) % 64 != 0) dict += ' ';  // header padded to a multiple of 64 bytes
        dict += '\n';
        std::FILE* f = std::fopen(filename, "wb");
        if (!f) return 1;
        const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
        const unsigned short hl = (unsigned short)dict.size();
        const unsigned char hlen[2] = {(unsigned char)(hl & 0xff), (unsigned char)(hl >> 8)};
        bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(hlen, 1, 2, f) == 2 &&
                  std::fwrite(dict.data(), 1, dict.size(), f) == dict.size() &&
                  std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
        ok = (std::fclose(f) == 0) && ok;
        return ok ? 0 : 1;
    }

private:
    template <typename ValImg, typename PosImg>
    void collapseFocus(int method, int half_patchsize, ValImg* confidence, PosImg* depth_cell_indices)
    {
        int nx, ny, nz;
        getDimensions(&nx, &ny, &nz);
        float* val = dsi::image_create<float>(*confidence, ny, nx);
        uint8_t* pos = dsi::image_create<uint8_t>(*depth_cell_indices, ny, nx);
        dsi::check(dsi_grid_collapse_focus(h_, method, half_patchsize, val, pos));
    }
    float getGridValueAt64(uint64_t p) const
    {
        float v = 0.f;
        dsi::check(dsi_grid_value_at(h_, p, &v));
        return v;
    }
    dsi_grid_t* h_ = nullptr;
    bool owned_ = false;
};

namespace EMVS {

struct ShapeDSI {  // mapper_emvs_stereo.hpp:40-65
    ShapeDSI() = default;
    ShapeDSI(size_t dimX, size_t dimY, size_t dimZ, float min_depth, float max_depth, float fov)
        : dimX_(dimX), dimY_(dimY), dimZ_(dimZ), min_depth_(min_depth), max_depth_(max_depth), fov_(fov)
    {
    }
    size_t dimX_ = 0, dimY_ = 0, dimZ_ = 100;
    float min_depth_ = 0.3f, max_depth_ = 5.f;
    float fov_ = 0.f;
};

struct OptionsDepthMap {  // mapper_emvs_stereo.hpp:68-82
    // the fields the extraction reads
    int adaptive_threshold_kernel_size_ = 5;
    double adaptive_threshold_c_ = 5.;
    double max_confidence = 0.;
    int median_filter_size_ = 5;
    // the fields main.cpp:163-171 also sets: carried for source compatibility -- they steer file output on the host
    // (save_*, full_sequence) and the reference view along the baseline (rv_pos: process1.cpp:63, the rv_pos argument of
    // process_1 / process_1_depth_map / full_sequence_depth_maps in dsi_process.hpp)
    bool full_sequence = false;
    bool save_conf_stats = false;
    bool save_mono = false;
    bool save_dsi = false;
    double rv_pos = 0.;
};

struct OptionsPointCloud {  // mapper_emvs_stereo.hpp:84-89 (defaults of main.cpp:80-81)
    float radius_search_ = 0.05f;
    int min_num_neighbors_ = 3;
};

typedef LinearTrajectory TrajectoryType;

class MapperEMVS {  // mapper_emvs_stereo.hpp:94-155
public:
    // plane_begin / plane_count: own only that range of the dimZ planes (plane sharding over GPUs;
    // 0, 0 = all planes, the reference behaviour)
    // the reference's arity MapperEMVS(cam, dsi_shape) (mapper_emvs_stereo.hpp:101) for any camera
    // type dsi::camera_of can read, on the process-wide default context
    template <typename CamT>
    MapperEMVS(const CamT& cam, const ShapeDSI& dsi_shape) : MapperEMVS(dsi::default_context(), convert(cam), dsi_shape)
    {
    }
    MapperEMVS(dsi::Context& ctx, const dsi::PinholeCameraModel& cam, const ShapeDSI& dsi_shape,
               bool inverse_depth = false, int plane_begin = 0, int plane_count = 0)
    {
        dsi_mapper_config_t cfg{};
        cfg.plane_begin = plane_begin;
        cfg.plane_count = plane_count;
        cfg.sensor_width = cam.width;
        cfg.sensor_height = cam.height;
        cfg.K[0] = cam.fx; cfg.K[1] = cam.fy; cfg.K[2] = cam.cx; cfg.K[3] = cam.cy;
        cfg.dim_x = (int)dsi_shape.dimX_;
        cfg.dim_y = (int)dsi_shape.dimY_;
        cfg.dim_z = (int)dsi_shape.dimZ_;
        cfg.min_depth = dsi_shape.min_depth_;
        cfg.max_depth = dsi_shape.max_depth_;
        cfg.fov_deg = dsi_shape.fov_;
        cfg.inverse_depth = inverse_depth ? 1 : 0;
        cfg.lut = cam.rectified_points.empty() ? nullptr : cam.rectified_points.data();
        dsi::check(dsi_mapper_create(ctx.handle(), &cfg, &h_));
        ctx_ = ctx.handle();
        dsi_ = Grid3D::view(dsi_mapper_grid(h_));
    }
    // the same with the rectification table made on the device from the calibration numbers, straight into the mapper's
    // buffer (dsi_mapper_create_with_lens); cam holds the size and fx, fy, cx, cy of P, and no table of its own
    MapperEMVS(dsi::Context& ctx, const dsi::PinholeCameraModel& cam, const dsi::Lens& lens, const ShapeDSI& dsi_shape,
               bool inverse_depth = false, int plane_begin = 0, int plane_count = 0)
    {
        if (!cam.rectified_points.empty())
            throw dsi::Error(DSI_ERR_INVALID, "MapperEMVS: a camera with rectified_points and a lens exclude each other");
        dsi_mapper_config_t cfg{};
        cfg.plane_begin = plane_begin;
        cfg.plane_count = plane_count;
        cfg.sensor_width = cam.width;
        cfg.sensor_height = cam.height;
        cfg.K[0] = cam.fx; cfg.K[1] = cam.fy; cfg.K[2] = cam.cx; cfg.K[3] = cam.cy;
        cfg.dim_x = (int)dsi_shape.dimX_;
        cfg.dim_y = (int)dsi_shape.dimY_;
        cfg.dim_z = (int)dsi_shape.dimZ_;
        cfg.min_depth = dsi_shape.min_depth_;
        cfg.max_depth = dsi_shape.max_depth_;
        cfg.fov_deg = dsi_shape.fov_;
        cfg.inverse_depth = inverse_depth ? 1 : 0;
        dsi::check(dsi_mapper_create_with_lens(ctx.handle(), &cfg, &lens, &h_));
        ctx_ = ctx.handle();
        dsi_ = Grid3D::view(dsi_mapper_grid(h_));
    }
    ~MapperEMVS()
    {
        dsi_.deallocate();
        dsi_mapper_destroy(h_);
    }
    MapperEMVS(const MapperEMVS&) = delete;
    MapperEMVS& operator=(const MapperEMVS&) = delete;

    // mapper_emvs_stereo.cpp:67-148.  Returns false when events.size() < 1024.  Any event type with
    // .x .y .ts (ts a double in seconds or with .toSec(): dvs_msgs::Event) and any pose type
    // dsi::to_pose7 can read (geometry_utils::Transformation) -- the reference's call
    // evaluateDSI(events, trajectory, T_rv_w) (process1.cpp:76) compiles as it stands.
    template <typename EventT, typename PoseT>
    bool evaluateDSI(const std::vector<EventT>& events, const TrajectoryType& trajectory, const PoseT& T_rv_w)
    {
        const size_t n = events.size();
        xs_.resize(n);
        ys_.resize(n);
        ts_.resize(n);
        for (size_t i = 0; i < n; ++i) {
            xs_[i] = (uint16_t)events[i].x;
            ys_[i] = (uint16_t)events[i].y;
            ts_[i] = dsi::to_seconds(events[i].ts);
        }
        double T7[7];
        dsi::to_pose7(T_rv_w, T7);
        size_t voted = 0;
        const int rc = dsi_mapper_evaluate(h_, xs_.data(), ys_.data(), ts_.data(), n, trajectory.times().data(),
                                           trajectory.poses7().data(), trajectory.times().size(), T7, &voted);
        if (rc == DSI_ERR_TOO_FEW_EVENTS) return false;
        dsi::check(rc);
        events_voted_ = voted;
        return true;
    }

    // The device part of getDepthMapFromDSI (mapper_emvs_stereo.cpp:339-437) WITHOUT its filters: arg-max over Z
    // (:368) and convertDepthIndicesToValues (:302-313) on the raw indices -- the map SURVEY 8(a) A11/A12 and the
    // "depth map equal to the CPU reference" statement are about.  Not a member of the reference (it keeps
    // depth_cell_indices local); hence its own name's third argument is the index map, not a mask.
    template <typename DepthImg, typename ConfImg, typename IdxImg>
    void getDepthMapFromDSI(DepthImg& depth_map, ConfImg& confidence_map, IdxImg& depth_cell_indices)
    {
        int nx, ny, nz;
        dsi_.getDimensions(&nx, &ny, &nz);
        float* depth = dsi::image_create<float>(depth_map, ny, nx);
        float* conf = dsi::image_create<float>(confidence_map, ny, nx);
        uint8_t* idx = dsi::image_create<uint8_t>(depth_cell_indices, ny, nx);
        dsi::check(dsi_mapper_depth_map(h_, depth, conf, idx));
    }

    // void getDepthMapFromDSI(cv::Mat& depth_map, cv::Mat& confidence_map, cv::Mat& mask, const OptionsDepthMap&,
    //                         int method = -1)                                   mapper_emvs_stereo.hpp:108, .cpp:331-335
    // void getDepthMapFromDSI(cv::Mat& depth_map, cv::Mat& confidence_map, cv::Mat& mask, const OptionsDepthMap&,
    //                         cv::Mat& depth_map_dense, int method = -1)         mapper_emvs_stereo.hpp:109, .cpp:338-437
    // on the device, from the mapper's OWN dsi_ like the reference (process1.cpp:208-222, process2.cpp:123-299,
    // process5.cpp:258, main.cpp:389-417 compile as spelled there): arg-max (:368), conf(0,0) = max_confidence +
    // normalisation (:393-397), Gaussian adaptive threshold (:403-409), masked Huang median (:420-423),
    // removeMaskBoundary (:426-427), index -> depth of the filtered indices (:435).  Outputs as the reference leaves
    // them: depth_map CV_32F, confidence_map CV_32F (element (0,0) overwritten), mask CV_8U in {0, 1}.
    // method: the reference's switch (:348-368) takes 0..4 to the focus-based collapses (collapseZSliceByLocalVar ...,
    // never selected by any caller: every call site passes the default) and everything else to collapseMaxZSlice.
    // These overloads refuse 0..4 with dsi::Error (DSI_ERR_BAD_OP), as they always have; anything else is the arg-max.
    // The focus-based depth map with the same filters is getDepthMapFromDSIByFocus below.
    // depth_map_dense: see dsi::inpaint_depth_cell_indices above -- filled when the caller supplies OpenCV's inpainting,
    // otherwise left empty.
    template <typename DepthImg, typename ConfImg, typename MaskImg>
    void getDepthMapFromDSI(DepthImg& depth_map, ConfImg& confidence_map, MaskImg& mask,
                            const OptionsDepthMap& options_depth_map, int method = -1)
    {
        extract(nullptr, depth_map, confidence_map, mask, options_depth_map, (MaskImg*)nullptr, (DepthImg*)nullptr, method);
    }
    template <typename DepthImg, typename ConfImg, typename MaskImg, typename DenseImg,
              typename = typename std::enable_if<!std::is_pointer<DenseImg>::value && !std::is_arithmetic<DenseImg>::value>::type>
    void getDepthMapFromDSI(DepthImg& depth_map, ConfImg& confidence_map, MaskImg& mask,
                            const OptionsDepthMap& options_depth_map, DenseImg& depth_map_dense, int method = -1)
    {
        MaskImg idx_filtered;
        extract(nullptr, depth_map, confidence_map, mask, options_depth_map, &idx_filtered, &depth_map_dense, method);
    }
    // getDepthMapFromDSI(depth_map, confidence_map, mask, options, method) for method 0..4 (mapper_emvs_stereo.cpp:350-364):
    // the focus-based collapse (dsi_mapper_depth_map_of_focus; GradMag with half_patchsize 1) of the mapper's own dsi_, or
    // of *grid, then the same filters as the overloads above.  Any other method is collapseMaxZSlice, as there.
    template <typename DepthImg, typename ConfImg, typename MaskImg>
    void getDepthMapFromDSIByFocus(DepthImg& depth_map, ConfImg& confidence_map, MaskImg& mask,
                                   const OptionsDepthMap& options_depth_map, int method, const Grid3D* grid = nullptr)
    {
        const bool focus = method >= DSI_FOCUS_LOCAL_VAR && method <= DSI_FOCUS_DOG;
        extract(grid, depth_map, confidence_map, mask, options_depth_map, (MaskImg*)nullptr, (DepthImg*)nullptr,
                focus ? method : -1, focus);
    }
    // the same for a DSI other than the mapper's own (not in the reference, which copies the DSI into a mapper first)
    template <typename DepthImg, typename ConfImg, typename MaskImg>
    void getDepthMapFromDSI(DepthImg& depth_map, ConfImg& confidence_map, MaskImg& mask,
                            const OptionsDepthMap& options_depth_map, const Grid3D* grid)
    {
        extract(grid, depth_map, confidence_map, mask, options_depth_map, (MaskImg*)nullptr, (DepthImg*)nullptr, -1);
    }

    // The filters of getDepthMapFromDSI (mapper_emvs_stereo.cpp:390-437) on the raw depth map this mapper already
    // holds on the device -- after dsi::process_1_depth_map, which votes, fuses and takes the arg-max without ever
    // writing the DSI the reference would call getDepthMapFromDSI on.  Same outputs as the overloads above.
    template <typename DepthImg, typename ConfImg, typename MaskImg>
    void filterDepthMap(DepthImg& depth_map, ConfImg& confidence_map, MaskImg& mask, const OptionsDepthMap& options_depth_map)
    {
        int nx, ny, nz;
        dsi_.getDimensions(&nx, &ny, &nz);
        float* depth = dsi::image_create<float>(depth_map, ny, nx);
        float* conf = dsi::image_create<float>(confidence_map, ny, nx);
        uint8_t* mk = dsi::image_create<uint8_t>(mask, ny, nx);
        const dsi_depthmap_options_t o = options_of(options_depth_map);
        dsi::check(dsi_mapper_filter_depth_map(h_, &o, depth, conf, mk, nullptr));
    }

    // void getPointcloud(const cv::Mat& depth_map, const cv::Mat& mask, const OptionsPointCloud&, PointCloud::Ptr& pc_)
    //                                                                          mapper_emvs_stereo.hpp:111, .cpp:440-480
    // on the device: the pixels with mask > 0 back-projected through the virtual camera (in double, like the reference),
    // in row-major order, then PCL's RadiusOutlierRemoval (radius_search_, min_num_neighbors_) as an exact count over a
    // uniform grid (dsi_mapper_get_pointcloud).  depth_map CV_32F / mask CV_8U of the DSI's size (any image type
    // dsi::image_data reads); pc_ a dsi::PointCloud, a pcl-like PointCloud<PointXYZI> or a Ptr to either
    // (dsi::point_cloud_assign).  The reference's call main.cpp:396 compiles as spelled there.
    template <typename DepthImg, typename MaskImg, typename CloudT>
    void getPointcloud(const DepthImg& depth_map, const MaskImg& mask, const OptionsPointCloud& options_pc, CloudT& pc_)
    {
        int nx, ny, nz;
        dsi_.getDimensions(&nx, &ny, &nz);
        if (depth_map.rows != ny || depth_map.cols != nx || mask.rows != ny || mask.cols != nx)
            throw dsi::Error(DSI_ERR_INVALID, "getPointcloud: depth_map and mask must be dimY x dimX");  // :446-447
        pointcloud(dsi::image_data<float>(const_cast<DepthImg&>(depth_map)),
                   dsi::image_data<uint8_t>(const_cast<MaskImg&>(mask)), options_pc, pc_);
    }
    // the same on the filtered depth map and mask the last getDepthMapFromDSI(..., options) / filterDepthMap left on the
    // device (no upload; dsi::Error if there is none since the last new depth map)
    template <typename CloudT>
    void getPointcloud(const OptionsPointCloud& options_pc, CloudT& pc_)
    {
        pointcloud(nullptr, nullptr, options_pc, pc_);
    }
    size_t pointsBeforeFilter() const { return pc_unfiltered_; }  // of the last getPointcloud

    // MapperEMVS::convertDepthIndicesToValues (mapper_emvs_stereo.cpp:302-313) on host images: depth = cellIndexToDepth(index)
    template <typename IdxImg, typename DepthImg>
    void convertDepthIndicesToValues(IdxImg& depth_cell_indices, DepthImg& depth_map)
    {
        int nx, ny, nz;
        dsi_.getDimensions(&nx, &ny, &nz);
        int dim_z = 0;
        dsi::check(dsi_mapper_full_depths(h_, nullptr, &dim_z));
        std::vector<float> z((size_t)dim_z);
        dsi::check(dsi_mapper_full_depths(h_, z.data(), nullptr));
        const uint8_t* idx = dsi::image_data<uint8_t>(depth_cell_indices);
        float* depth = dsi::image_create<float>(depth_map, ny, nx);
        for (size_t i = 0; i < (size_t)nx * ny; ++i) {
            if ((int)idx[i] >= dim_z) throw dsi::Error(DSI_ERR_INVALID, "convertDepthIndicesToValues: index beyond dimZ");
            depth[i] = z[idx[i]];
        }
    }

    std::vector<float> depthPlanes() const
    {
        int nz = 0;
        dsi::check(dsi_mapper_geometry(h_, nullptr, nullptr, nullptr, nullptr, &nz));
        std::vector<float> z(nz);
        dsi::check(dsi_mapper_geometry(h_, nullptr, z.data(), nullptr, nullptr, nullptr));
        return z;
    }
    size_t eventsVoted() const { return events_voted_; }
    dsi_mapper_t* handle() const { return h_; }
    dsi_context_t* context() const { return ctx_; }

    Grid3D dsi_;       // public member, as in the reference (mapper_emvs_stereo.hpp:116)
    std::string name;  // mapper_emvs_stereo.hpp:117

private:
    static dsi_depthmap_options_t options_of(const OptionsDepthMap& options_depth_map)
    {
        dsi_depthmap_options_t o{};
        o.adaptive_threshold_kernel_size = options_depth_map.adaptive_threshold_kernel_size_;
        o.adaptive_threshold_c = options_depth_map.adaptive_threshold_c_;
        o.median_filter_size = options_depth_map.median_filter_size_;
        o.max_confidence = options_depth_map.max_confidence;
        return o;
    }
    template <typename DepthImg, typename ConfImg, typename MaskImg, typename DenseImg>
    void extract(const Grid3D* grid, DepthImg& depth_map, ConfImg& confidence_map, MaskImg& mask,
                 const OptionsDepthMap& options_depth_map, MaskImg* idx_filtered, DenseImg* depth_map_dense, int method,
                 bool focus = false)
    {
        if (!focus && method >= 0 && method <= 4)
            throw dsi::Error(DSI_ERR_BAD_OP, "getDepthMapFromDSI: method " + std::to_string(method) +
                                                 " is one of the focus-based collapses (collapseZSliceByLocalVar / "
                                                 "LocalMeanSquare / GradMag / LaplacianMag / DoG, mapper_emvs_stereo.cpp:350-364), "
                                                 "which this overload refuses; call getDepthMapFromDSIByFocus for them, or pass "
                                                 "the default (-1): collapseMaxZSlice");
        int nx, ny, nz;
        dsi_.getDimensions(&nx, &ny, &nz);
        float* depth = dsi::image_create<float>(depth_map, ny, nx);
        float* conf = dsi::image_create<float>(confidence_map, ny, nx);
        uint8_t* mk = dsi::image_create<uint8_t>(mask, ny, nx);
        uint8_t* filtered = idx_filtered ? dsi::image_create<uint8_t>(*idx_filtered, ny, nx) : nullptr;
        const dsi_depthmap_options_t o = options_of(options_depth_map);
        if (focus) {  // :350-364
            dsi::check(dsi_mapper_depth_map_of_focus(h_, grid ? grid->handle() : dsi_.handle(), method));
            dsi::check(dsi_mapper_filter_depth_map(h_, &o, depth, conf, mk, filtered));
        } else {
            dsi::check(dsi_mapper_get_depth_map_from_dsi(h_, grid ? grid->handle() : nullptr, &o, depth, conf, mk, filtered));
        }
        if (!depth_map_dense) return;
        // mapper_emvs_stereo.cpp:430-436
        MaskImg inpaint_mask, inpainted;
        uint8_t* im = dsi::image_create<uint8_t>(inpaint_mask, ny, nx);
        for (size_t i = 0; i < (size_t)nx * ny; ++i) im[i] = (uint8_t)(1 - mk[i]);
        using dsi::inpaint_depth_cell_indices;  // the default; an overload for MaskImg found by ADL wins over it
        if (inpaint_depth_cell_indices(*idx_filtered, inpaint_mask, inpainted))
            convertDepthIndicesToValues(inpainted, *depth_map_dense);
        else
            dsi::image_release(*depth_map_dense);
    }
    template <typename CloudT>
    void pointcloud(const float* depth, const uint8_t* mask, const OptionsPointCloud& options_pc, CloudT& pc_)
    {
        int nx, ny, nz;
        dsi_.getDimensions(&nx, &ny, &nz);
        const size_t npix = (size_t)nx * ny;
        pc_buf_.resize(npix);  // (nx * ny points always fit; kept from call to call)
        dsi_pointcloud_options_t o{};
        o.radius_search = options_pc.radius_search_;
        o.min_num_neighbors = options_pc.min_num_neighbors_;
        size_t n = 0;
        dsi::check(dsi_mapper_get_pointcloud(h_, depth, mask, &o, reinterpret_cast<float*>(pc_buf_.data()), npix, &n,
                                             &pc_unfiltered_));
        using dsi::point_cloud_assign;  // the defaults; an overload for CloudT found by ADL wins over them
        point_cloud_assign(pc_, pc_buf_.data(), n);
    }
    template <typename CamT>
    static dsi::PinholeCameraModel convert(const CamT& cam)
    {
        dsi::PinholeCameraModel c;
        dsi::camera_of(cam, &c);
        return c;
    }
    dsi_mapper_t* h_ = nullptr;
    dsi_context_t* ctx_ = nullptr;
    std::vector<uint16_t> xs_, ys_;
    std::vector<double> ts_;
    size_t events_voted_ = 0;
    std::vector<dsi::PointXYZI> pc_buf_;
    size_t pc_unfiltered_ = 0;
};

}  // namespace EMVS

// ---- the run's pictures (utils.hpp:23-52, utils.cpp:22-117, 184-216; arithmetic: dsi_engine.h) ----
namespace dsi {

// Customisation point: the 256-entry colour table (B G R per entry) of saveDepthMaps' inverse-depth image.  The default is
// the engine's piecewise-linear jet (dsi_default_jet_lut), NOT OpenCV's COLORMAP_JET table.  A caller with OpenCV adds,
// in namespace dsi before this header,
//     inline bool color_map_jet(uint8_t (&lut)[256][3]) { /* cv::applyColorMap of a 0..255 ramp, COLORMAP_JET */ return true; }
// and that non-template wins over this template.  (Its argument is an array of a built-in type, which has no associated
// namespace: unlike inpaint_depth_cell_indices it cannot be found by ADL in the image type's namespace.)
template <typename Tag = void>
inline bool color_map_jet(uint8_t (&lut)[256][3])
{
    check(dsi_default_jet_lut(&lut[0][0]));
    return true;
}

// accumulateEvents(events, use_polarity, img) on the device of ctx: img is an existing 8-bit single-channel image of the
// sensor's size (cv::Mat(full_resolution, CV_8UC1), main.cpp:246-249), any type dsi::image_data reads; events any type
// with .x .y .polarity (dvs_msgs::Event).  Returns the number of events outside the image, which are dropped.
template <typename EventT, typename ImgT>
inline size_t accumulateEvents(Context& ctx, const std::vector<EventT>& events, const bool use_polarity, ImgT& img)
{
    const size_t n = events.size();
    std::vector<uint16_t> x(n), y(n);
    std::vector<uint8_t> pol(n);
    for (size_t i = 0; i < n; ++i) {
        x[i] = (uint16_t)events[i].x;
        y[i] = (uint16_t)events[i].y;
        pol[i] = events[i].polarity ? 1 : 0;
    }
    size_t dropped = 0;
    check(dsi_event_image(ctx.handle(), x.data(), y.data(), pol.data(), n, img.cols, img.rows, use_polarity ? 1 : 0,
                          img.rows > 0 && img.cols > 0 ? dsi::image_data<uint8_t>(img) : nullptr, &dropped));
    return dropped;
}

// saveDepthMaps on the device of ctx: depth_points_<suffix>.txt (utils.cpp:31-46), confidence_map_negated_<suffix>.png
// (:55-58, through dsi::imwrite_gray8) and inv_depth_colored_dilated_<suffix>.png (:82-93, dsi::write_png_rgb8), each
// prefixed by out_path.  conf_negated / inv_depth_bgr (may be NULL) receive the two images.
template <typename DepthImg, typename ConfImg, typename MaskImg>
inline void saveDepthMaps(Context& ctx, const DepthImg& depth_map, const ConfImg& confidence_map, const MaskImg& semidense_mask,
                          const float min_depth, const float max_depth, const std::string& suffix, const std::string& out_path,
                          std::vector<uint8_t>* conf_negated = nullptr, std::vector<uint8_t>* inv_depth_bgr = nullptr)
{
    const int rows = depth_map.rows, cols = depth_map.cols;
    if (confidence_map.rows != rows || confidence_map.cols != cols || semidense_mask.rows != rows || semidense_mask.cols != cols)
        throw Error(DSI_ERR_INVALID, "saveDepthMaps: the three maps must have one size");
    const float* depth = dsi::image_data<float>(const_cast<DepthImg&>(depth_map));
    const float* conf = dsi::image_data<float>(const_cast<ConfImg&>(confidence_map));
    const uint8_t* mask = dsi::image_data<uint8_t>(const_cast<MaskImg&>(semidense_mask));
    if (std::FILE* of = std::fopen((out_path + "depth_points_" + suffix + ".txt").c_str(), "w")) {  // :31-46
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c)
                if (mask[(size_t)r * cols + c] > 0)  // operator<<(float): %g
                    std::fprintf(of, "%d %d %g\n", c, r, (double)depth[(size_t)r * cols + c]);
        std::fclose(of);
    }
    uint8_t lut[256][3];
    const bool own_table = color_map_jet(lut);
    MaskImg negated;
    uint8_t* neg = dsi::image_create<uint8_t>(negated, rows, cols);
    std::vector<uint8_t> bgr((size_t)rows * cols * 3);
    check(dsi_depth_images(ctx.handle(), depth, conf, mask, rows, cols, min_depth, max_depth, own_table ? &lut[0][0] : nullptr, neg,
                           bgr.data()));
    using dsi::imwrite_gray8;
    if (!imwrite_gray8(out_path + "confidence_map_negated_" + suffix + ".png", negated))
        throw Error(DSI_ERR_INVALID, "saveDepthMaps: cannot write " + out_path + "confidence_map_negated_" + suffix + ".png");
    if (!write_png_rgb8(out_path + "inv_depth_colored_dilated_" + suffix + ".png", bgr.data(), rows, cols))
        throw Error(DSI_ERR_INVALID, "saveDepthMaps: cannot write " + out_path + "inv_depth_colored_dilated_" + suffix + ".png");
    if (conf_negated) conf_negated->assign(neg, neg + (size_t)rows * cols);
    if (inv_depth_bgr) inv_depth_bgr->swap(bgr);
}

// Ground-truth depth from DSEC disparity images on the device (dsi_gt_*): what the reference's
// scripts/evaluate_mcemvs_dsec.py:108-122 computes per frame.  Q[16], T[16] (the matrix that is applied: the script's
// inv(T_rect0_0)) and K[12] (3 x 4, the script's K_0) are row-major doubles.  Images are of any type dsi::image_data reads.
class GroundTruthProjector {
public:
    GroundTruthProjector(Context& ctx, int width, int height, const double* Q, const double* T, const double* K,
                         int mode = DSI_GT_AS_SCRIPT)
        : width_(width), height_(height)
    {
        check(dsi_gt_create(ctx.handle(), width, height, Q, T, K, mode, &h_));
    }
    ~GroundTruthProjector() { dsi_gt_destroy(h_); }
    GroundTruthProjector(const GroundTruthProjector&) = delete;
    GroundTruthProjector& operator=(const GroundTruthProjector&) = delete;
    dsi_gt_t* handle() const { return h_; }
    int width() const { return width_; }
    int height() const { return height_; }

    // disparity: float32 [height][width], the script's disp.astype(np.float32) * 256; queued on the context's stream
    template <typename DispImg>
    void project(const DispImg& disparity)
    {
        check_size(disparity.rows, disparity.cols);
        check(dsi_gt_project(h_, dsi::image_data<float>(const_cast<DispImg&>(disparity))));
    }
    // raw: the uint16 samples of the disparity PNG; converted on the device
    template <typename RawImg>
    void projectPng16(const RawImg& raw)
    {
        check_size(raw.rows, raw.cols);
        check(dsi_gt_project_u16(h_, dsi::image_data<uint16_t>(const_cast<RawImg&>(raw))));
    }
    // the last projection's depth map (float32, created as height x width) and counts; synchronises
    template <typename DepthImg>
    void fetch(DepthImg& depth, uint64_t* n_points = nullptr, uint64_t* n_outside = nullptr) const
    {
        check(dsi_gt_fetch(h_, dsi::image_create<float>(depth, height_, width_), n_points, n_outside));
    }
    float* devicePtr() const { return dsi_gt_device_ptr(h_); }

private:
    void check_size(int rows, int cols) const
    {
        if (rows != height_ || cols != width_) throw Error(DSI_ERR_INVALID, "GroundTruthProjector: the image must be height x width");
    }
    dsi_gt_t* h_ = nullptr;
    int width_ = 0, height_ = 0;
};

// Depth maps scored against ground-truth depth on the device (dsi_score_*): the metrics of the reference's
// scripts/depth_metrics.py and the curves of precision_completeness.py over every window added.  Images are of any type
// dsi::image_data reads (cv::Mat CV_32FC1 / CV_8UC1, dsi::Image<T>).
struct ScoreCurves {  // precision_completeness.py:43-92, one entry per error bin
    std::vector<double> base, precision, recall, f1, outliers;
};
class DepthScore {
public:
    DepthScore(Context& ctx, size_t capacity_points, double baseline, double focal, double gt_min = 0.05)
    {
        check(dsi_score_create(ctx.handle(), capacity_points, baseline, focal, gt_min, &h_));
    }
    ~DepthScore() { dsi_score_destroy(h_); }
    DepthScore(const DepthScore&) = delete;
    DepthScore& operator=(const DepthScore&) = delete;
    dsi_score_t* handle() const { return h_; }

    // one window: the estimated depth (f32), its mask (u8, non-zero = estimated) and the ground truth (f32), of one size
    template <typename DepthImg, typename MaskImg, typename GtImg>
    void add(const DepthImg& depth_map, const MaskImg& mask, const GtImg& ground_truth)
    {
        if (mask.rows != depth_map.rows || mask.cols != depth_map.cols || ground_truth.rows != depth_map.rows ||
            ground_truth.cols != depth_map.cols)
            throw Error(DSI_ERR_INVALID, "DepthScore::add: the three maps must have one size");
        check(dsi_score_add(h_, dsi::image_data<float>(const_cast<DepthImg&>(depth_map)),
                            dsi::image_data<uint8_t>(const_cast<MaskImg&>(mask)),
                            dsi::image_data<float>(const_cast<GtImg&>(ground_truth)), (size_t)depth_map.rows * depth_map.cols));
    }
    // one window from the filtered maps a mapper's getDepthMapFromDSI(..., options) left on the device
    template <typename MapperT, typename GtImg>
    void addMapper(MapperT& mapper, const GtImg& ground_truth)
    {
        check(dsi_score_add_mapper(h_, mapper.handle(), dsi::image_data<float>(const_cast<GtImg&>(ground_truth))));
    }
    // one window against the depth map a projector last made: the ground truth is read where it lies on the device
    template <typename DepthImg, typename MaskImg>
    void add(const DepthImg& depth_map, const MaskImg& mask, const GroundTruthProjector& projector)
    {
        if (mask.rows != depth_map.rows || mask.cols != depth_map.cols)
            throw Error(DSI_ERR_INVALID, "DepthScore::add: depth_map and mask must have one size");
        check(dsi_score_add_gt(h_, dsi::image_data<float>(const_cast<DepthImg&>(depth_map)),
                               dsi::image_data<uint8_t>(const_cast<MaskImg&>(mask)), (size_t)depth_map.rows * depth_map.cols,
                               projector.handle()));
    }
    // a mapper's filtered maps against a projector's depth map: nothing is uploaded
    template <typename MapperT>
    void addMapper(MapperT& mapper, const GroundTruthProjector& projector)
    {
        check(dsi_score_add_mapper_gt(h_, mapper.handle(), projector.handle()));
    }
    // one frame from the depth image and mask that WorldMap::render left on the device, against ground_truth[height * width]
    // of the render's size: only it is uploaded
    template <typename MapT>
    void addMapRender(MapT& world_map, const float* ground_truth)
    {
        check(dsi_score_add_map_render(h_, world_map.handle(), ground_truth));
    }
    // the same against a projector's depth map: nothing is uploaded
    template <typename MapT>
    void addMapRender(MapT& world_map, const GroundTruthProjector& projector)
    {
        check(dsi_score_add_map_render_gt(h_, world_map.handle(), projector.handle()));
    }
    dsi_score_metrics_t metrics() const
    {
        dsi_score_metrics_t m;
        check(dsi_score_metrics(h_, &m));
        return m;
    }
    double median() const
    {
        double v = 0;
        check(dsi_score_median(h_, &v));
        return v;
    }
    // np.histogram(err, bins = int(max(err) / binwidth)): the counts; [first_edge, last_edge] is the range
    std::vector<uint64_t> histogram(double binwidth, double* first_edge = nullptr, double* last_edge = nullptr) const
    {
        size_t n = 0;
        double lo = 0, hi = 0;
        check(dsi_score_histogram(h_, binwidth, nullptr, 0, &n, &lo, &hi));
        std::vector<uint64_t> counts(n);
        if (n) check(dsi_score_histogram(h_, binwidth, counts.data(), n, &n, &lo, &hi));
        if (first_edge) *first_edge = lo;
        if (last_edge) *last_edge = hi;
        return counts;
    }
    // host arithmetic on the exact counts, written as the script writes it; base = np.linspace(first, last, bins + 1)[:-1]
    ScoreCurves curves(double binwidth = 0.01) const
    {
        const dsi_score_metrics_t m = metrics();
        double lo = 0, hi = 0;
        const std::vector<uint64_t> counts = histogram(binwidth, &lo, &hi);
        ScoreCurves c;
        const size_t nb = counts.size();
        const double delta = hi - lo, step = nb ? delta / (double)nb : 0.0;
        uint64_t cum = 0;
        for (size_t i = 0; i < nb; ++i) {
            cum += counts[i];
            c.base.push_back(step != 0.0 ? (double)i * step + lo : ((double)i / (double)nb) * delta + lo);
            const double p = (double)cum / (double)m.n_est * 100.0, r = (double)cum / (double)m.n_gt * 100.0;
            c.precision.push_back(p);
            c.recall.push_back(r);
            c.f1.push_back(2.0 * p * r / (p + r));
            c.outliers.push_back((double)(m.n_joint - cum) / (double)m.n_joint * 100.0);
        }
        return c;
    }
    void reset() { check(dsi_score_reset(h_)); }

private:
    dsi_score_t* h_ = nullptr;
};

// A rigid pose as the 12 doubles, row-major [R | t], that the world map takes
inline std::array<double, 12> pose_matrix(const Transformation& T)
{
    const double w = T.q[0], x = T.q[1], y = T.q[2], z = T.q[3];
    return {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), T.t[0],
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), T.t[1],
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), T.t[2]};
}
// its inverse (dsi_invert_pose, the routine the Python binding calls too): R' = R^T, t'_i = -((r0i t0 + r1i t1) + r2i t2) --
// a window's T_rv_w to the T_w_rv that WorldMap::integrate takes
inline std::array<double, 12> invert_pose(const std::array<double, 12>& T)
{
    std::array<double, 12> out;
    check(dsi_invert_pose(T.data(), out.data()));
    return out;
}
inline std::array<double, 12> invert_pose(const Transformation& T) { return invert_pose(pose_matrix(T)); }
// A o B (dsx_pose_compose, the routine the Python binding calls too): R = A_R B_R, t = A_R B_t + A_t, every dot product
// ((a0 b0 + a1 b1) + a2 b2) in double without FMA
inline std::array<double, 12> compose_pose(const std::array<double, 12>& A, const std::array<double, 12>& B)
{
    std::array<double, 12> out;
    check(dsx_pose_compose(A.data(), B.data(), out.data()));
    return out;
}

// What WorldMap's members share (DESIGN.md 7j "The map's bindings").
namespace detail {
// f(args..., &info), checked: the counts of a pass
template <typename Info, typename F, typename... Args>
inline Info info_of(F f, Args... args)
{
    Info info;
    check(f(args..., &info));
    return info;
}
// null for a vector without elements: an output that is not asked for
template <typename T>
inline T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
// The two calls of a fetch.  call(0, &n) asks for the number of rows -- it is refused for want of room as soon as there are
// rows, so its refusal counts only when it leaves n at 0 --, room(n) makes room, and call(n, &n) fills it; with
// fill_when_empty == false the second call is left out when there is no row.
template <typename Call, typename Room>
inline size_t fetch_rows(Call call, Room room, bool fill_when_empty = true)
{
    size_t n = 0;
    const int rc = call((size_t)0, &n);
    if (rc != DSI_OK && n == 0) check(rc);
    room(n);
    if (n || fill_when_empty) check(call(n, &n));
    return n;
}
// rows[i] <- rows[order[i]] of a column of order.size() rows; a column without elements (an optional one) stays so
template <typename T>
inline void gather_rows(const std::vector<size_t>& order, std::vector<T>& column)
{
    if (column.empty()) return;
    const size_t width = column.size() / order.size();
    std::vector<T> out(column.size());
    for (size_t i = 0; i < order.size(); ++i) std::copy_n(column.begin() + width * order[i], width, out.begin() + width * i);
    column.swap(out);
}
template <typename T, typename... Rest>
inline void gather_rows(const std::vector<size_t>& order, std::vector<T>& column, std::vector<Rest>&... rest)
{
    gather_rows(order, column);
    gather_rows(order, rest...);
}
// the n rows of the columns in the order of less(a, b) over their indices, which may read the columns: they move afterwards
template <typename Less, typename... Columns>
inline void sort_rows(size_t n, Less less, Columns&... columns)
{
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), less);
    gather_rows(order, columns...);
}
// by ascending key: the order of a sorted fetch
template <typename... Columns>
inline void sort_rows_by_key(std::vector<uint64_t>& keys, Columns&... columns)
{
    sort_rows(keys.size(), [&](size_t a, size_t b) { return keys[a] < keys[b]; }, keys, columns...);
}
}  // namespace detail

// A persistent world-frame map on the device (dsi_map_*): every integrate call moves one window's cloud from
// its reference view to the world frame and merges it into cubic cells of edge `leaf` -- a centroid per cell (PCL's
// VoxelGrid), the number of points and the number of calls (windows) that reached the cell.  The arithmetic is stated in
// dsi_engine.h; the map's bits depend neither on the order of the points nor on how they are split into calls.
struct WorldMapCells {  // by ascending key when sorted
    std::vector<float> xyz;  // 3 per cell
    std::vector<uint32_t> n, windows;
    std::vector<uint64_t> keys;
    size_t size() const { return keys.size(); }
};
// a view of the map and what a render of it counts (dsi_map_view_t: size, splat, filter, fx fy cx cy, depth range, T_v_w)
using MapView = dsi_map_view_t;
using MapRenderInfo = dsi_map_render_info_t;
struct MapRenderImages {  // height x width, row-major
    int width = 0, height = 0;
    std::vector<float> depth;
    std::vector<uint32_t> windows, hits;
    std::vector<uint8_t> mask;
};
// map-to-map distances (dsi_map_eval.h: dsx_map_compare): the options, and what a compare counts
using MapCompareOptions = dsx_map_compare_opts_t;
struct MapCompareResult {
    dsx_map_compare_info_t info{};
    std::vector<uint64_t> hist;  // n_bins counts, bins of width radius / n_bins
    double radius = 0.0;
    // the mean of the matched distances: sum_q * radius / 2^32 / n_matched (0 without a matched cell)
    double mean() const { return info.n_matched ? (double)info.sum_q * radius / 4294967296.0 / (double)info.n_matched : 0.0; }
};
struct MapDistances {  // by ascending key when sorted
    std::vector<uint64_t> keys;
    std::vector<float> dist;  // +inf where the cell is unmatched
    size_t size() const { return keys.size(); }
};
// pruning (dsi_map_prune.h: dsx_map_prune): the options -- the defaults switch every criterion off -- and what a prune counts
struct MapPruneOptions : dsx_map_prune_opts_t {
    MapPruneOptions() : dsx_map_prune_opts_t{}
    {
        min_points = min_windows = 1;
        max_age = -1;
    }
    // criterion 4: the closed box [lo, hi]
    MapPruneOptions& box(const std::array<double, 3>& lo, const std::array<double, 3>& hi)
    {
        use_box = 1;
        for (int a = 0; a < 3; ++a) box_lo[a] = lo[(size_t)a], box_hi[a] = hi[(size_t)a];
        return *this;
    }
};
using MapPruneInfo = dsx_map_prune_info_t;
struct MapPruneReasons {  // by ascending key when sorted
    std::vector<uint64_t> keys;
    std::vector<uint8_t> reason;  // 0 kept, 1..5 the first criterion that failed
    size_t size() const { return keys.size(); }
};
// connected components (dsi_map_components.h): the labelling's options -- the defaults label every cell at connectivity
// 26 --, the selection's -- the defaults keep every labelled cell --, and what comes back
struct MapComponentsOptions : dsx_map_components_opts_t {
    MapComponentsOptions() : dsx_map_components_opts_t{}
    {
        min_points = min_windows = 1;
        connectivity = 26;
    }
};
struct MapComponentsSelection : dsx_map_components_selection_t {
    MapComponentsSelection() : dsx_map_components_selection_t{} { min_cells = min_component_points = 1; }
};
using MapComponentsInfo = dsx_map_components_info_t;
using MapComponentsSelectInfo = dsx_map_components_select_info_t;
struct MapComponentLabels {  // one row per labelled cell, by ascending key when sorted
    std::vector<uint64_t> keys, labels;
    std::vector<uint8_t> reason;  // with_reasons only: 0 kept, 1..4 the first reason of the selection that holds
    size_t size() const { return keys.size(); }
};
struct MapComponentList {  // one row per component, by cells descending, then label ascending
    std::vector<uint64_t> labels, cells, points;
    size_t size() const { return labels.size(); }
};
// the k nearest cells and the statistical outliers (dsi_map_knn.h): the query's options -- the defaults ask every cell for
// its 8 nearest and score a cell that found one --, the selection's -- one deviation above the mean --, and what comes back
struct MapKnnOptions : dsx_map_knn_opts_t {
    explicit MapKnnOptions(double radius_, int k_ = 8) : dsx_map_knn_opts_t{}
    {
        min_points = min_windows = 1;
        k = k_;
        min_found = 1;
        radius = radius_;
    }
};
struct MapKnnSelection : dsx_map_knn_selection_t {
    explicit MapKnnSelection(double std_mult_ = 1.0, bool shrink_ = false) : dsx_map_knn_selection_t{}
    {
        std_mult = std_mult_;
        shrink = shrink_ ? 1 : 0;
    }
};
using MapKnnInfo = dsx_map_knn_info_t;
using MapKnnSelectInfo = dsx_map_knn_select_info_t;
struct MapNeighbours {  // one row of k per query point: keys padded with 0, dist with +inf
    int k = 0;
    std::vector<uint64_t> keys;
    std::vector<float> dist;
    std::vector<uint8_t> found;
    size_t size() const { return found.size(); }
};
struct MapKnnThreshold {
    double mu = 0.0, sigma = 0.0;
    uint64_t T_q = 0;
};
// the outlier threshold of a self query's moments (dsx_map_knn_threshold; no device is touched)
inline MapKnnThreshold knn_threshold(uint64_t n_scored, uint64_t sum_q, const uint64_t sum_q2[2], double std_mult)
{
    MapKnnThreshold t;
    check(dsx_map_knn_threshold(n_scored, sum_q, sum_q2, std_mult, &t.mu, &t.sigma, &t.T_q));
    return t;
}
inline MapKnnThreshold knn_threshold(const MapKnnInfo& info, double std_mult)
{
    return knn_threshold(info.n_scored, info.sum_q, info.sum_q2, std_mult);
}
// the local shape (dsi_map_pca.h): the pass's options -- the defaults take the 8 nearest cells within the radius and ask
// for two of them --, the selection's -- curves and surfaces stay, scattered and sparse cells leave --, and what comes back
struct MapPcaOptions : dsx_map_pca_opts_t {
    explicit MapPcaOptions(double radius_, int k_ = 8) : dsx_map_pca_opts_t{}
    {
        min_points = min_windows = 1;
        k = k_;
        min_found = 2;
        radius = radius_;
    }
    MapPcaOptions& lookAt(double x, double y, double z)  // the normals turn towards this point
    {
        orient = 1;
        viewpoint[0] = x, viewpoint[1] = y, viewpoint[2] = z;
        return *this;
    }
};
struct MapPcaSelection : dsx_map_pca_selection_t {
    explicit MapPcaSelection(uint32_t keep_ = DSX_PCA_LINEAR | DSX_PCA_PLANAR, bool remove_sparse_ = true, bool shrink_ = false)
        : dsx_map_pca_selection_t{}
    {
        keep_labels = keep_;
        remove_sparse = remove_sparse_ ? 1 : 0;
        shrink = shrink_ ? 1 : 0;
    }
};
using MapPcaInfo = dsx_map_pca_info_t;
using MapPcaSelectInfo = dsx_map_pca_select_info_t;
using PcaRow = dsx_pca_row_t;
struct MapShapes {  // one row per query, in extract's order under the pass's filter: normal, tangent, eval 3 floats each
    std::vector<uint64_t> keys;
    std::vector<float> normal, tangent, eval;
    std::vector<uint16_t> members;
    std::vector<uint8_t> label, flags;
    std::vector<int64_t> moments;  // 9 per row (s[3], ss[6]) when the pass kept them, else empty
    size_t size() const { return keys.size(); }
};
// one cell's local shape from its integer moments (dsx_pca_solve; no device is touched); viewpoint and p orient the normal
inline PcaRow pca_solve(uint32_t m, const int64_t s[3], const int64_t ss[6], double quantum, const double* viewpoint = nullptr,
                        const double* p = nullptr)
{
    PcaRow r;
    check(dsx_pca_solve(m, s, ss, quantum, viewpoint ? 1 : 0, viewpoint, p, &r));
    return r;
}
// carving by free space (dsi_map_visibility.h): one observation -- a depth image's size, pinhole, depth range and pose
// world -> view; the defaults judge a cell by the 3 x 3 pixels around its own with no tolerance --, the selection's options
// -- a cell leaves when two views look through it, and more views than agree with it --, and what comes back
struct MapObservation : dsx_map_observation_t {
    MapObservation(int width_, int height_, double fx_, double fy_, double cx_, double cy_, double min_depth_, double max_depth_,
                   const std::array<double, 12>& T_v_w_, int window_ = 1, double abs_tol_ = 0.0, double rel_tol_ = 0.0)
        : dsx_map_observation_t{}
    {
        width = width_, height = height_, window = window_;
        fx = fx_, fy = fy_, cx = cx_, cy = cy_;
        min_depth = min_depth_, max_depth = max_depth_;
        abs_tol = abs_tol_, rel_tol = rel_tol_;
        std::copy(T_v_w_.begin(), T_v_w_.end(), T_v_w);
    }
};
struct MapVisibilitySelection : dsx_map_visibility_selection_t {
    explicit MapVisibilitySelection(uint32_t min_through_ = 2, uint32_t agree_weight_ = 1, bool shrink_ = false)
        : dsx_map_visibility_selection_t{}
    {
        min_through = min_through_;
        agree_weight = agree_weight_;
        shrink = shrink_ ? 1 : 0;
    }
};
using MapObserveInfo = dsx_map_observe_info_t;
using MapVisibilitySelectInfo = dsx_map_visibility_select_info_t;
struct MapVisibility {  // one row per cell: the views with a verdict on it, and those that agreed and looked through
    std::vector<uint64_t> keys;
    std::vector<uint32_t> seen, agree, through;
    std::vector<uint8_t> reason;  // after selectCarved() on this tally (1 carved, 0 kept), else empty
    size_t size() const { return keys.size(); }
};
// merging and moving the state (dsi_map_merge.h): a map's exact state on the host, and what a merge counts
struct MapState {  // by ascending key when sorted
    double leaf = 0.0;
    uint64_t calls = 0, accepted = 0, rejected = 0;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> n;
    std::vector<uint64_t> S;  // 3 per cell: the sums of the 32-bit cell fractions
    std::vector<uint32_t> windows, stamp;
    size_t size() const { return keys.size(); }
};
using MapMergeInfo = dsx_map_merge_info_t;
// aligning (dsi_map_align.h): the options -- the defaults make one pass with the filters open --, the exact integer moments
// of a correspondence pass, and what the ICP loop reports
struct MapAlignOptions : dsx_map_align_opts_t {
    explicit MapAlignOptions(double radius_) : dsx_map_align_opts_t{}
    {
        min_points_a = min_windows_a = min_points_b = min_windows_b = 1;
        radius = radius_;
        max_iterations = 1;
    }
};
using MapAlignMoments = dsx_map_align_moments_t;
using MapAlignSolveInfo = dsx_map_align_solve_info_t;
struct MapAlignResult {
    std::array<double, 12> T{};  // the frame of the aligned map in the other's; the last good pose when !ok
    dsx_map_align_info_t info{};
    bool ok = false;             // false: a round matched fewer than min_matched cells or its pairs were degenerate
};
constexpr std::array<double, 12> kIdentityPose = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
// the rigid motion of a pass's moments (dsx_map_align_solve; no device is touched); throws for fewer than 3 pairs and for
// pairs that do not determine a rotation
inline std::array<double, 12> solve_alignment(const MapAlignMoments& moments, MapAlignSolveInfo* info = nullptr)
{
    std::array<double, 12> T;
    check(dsx_map_align_solve(&moments, T.data(), info));
    return T;
}
class WorldMap {
public:
    WorldMap(Context& ctx, double leaf, int capacity_log2 = 16) : ctx_(ctx) { check(dsi_map_create(ctx.handle(), leaf, capacity_log2, &h_)); }
    ~WorldMap() { dsi_map_destroy(h_); }
    WorldMap(const WorldMap&) = delete;
    WorldMap& operator=(const WorldMap&) = delete;
    dsi_map_t* handle() const { return h_; }
    Context& context() const { return ctx_; }

    // one call of n host points, stride 3 or 4 floats (x, y, z first); returns the number of points rejected
    size_t integrate(const float* xyz, size_t stride_floats, size_t n, const std::array<double, 12>& T_w_rv)
    {
        size_t rejected = 0;
        check(dsi_map_integrate(h_, xyz, stride_floats, n, T_w_rv.data(), &rejected));
        return rejected;
    }
    size_t integrate(const PointCloud& pc, const std::array<double, 12>& T_w_rv)
    {
        static_assert(sizeof(PointXYZI) == 4 * sizeof(float), "PointXYZI is x, y, z, intensity");
        return integrate(pc.points.empty() ? nullptr : &pc.points[0].x, 4, pc.points.size(), T_w_rv);
    }
    // one call of the cloud mapper.getPointcloud(options_pc, cloud) would return, where it lies on the device; the mapper
    // must live on the map's context.  Returns the number of points rejected; *n_points: the cloud's size.
    template <typename MapperT, typename OptionsT>
    size_t integrateMapper(MapperT& mapper, const OptionsT& options_pc, const std::array<double, 12>& T_w_rv, size_t* n_points = nullptr)
    {
        dsi_pointcloud_options_t o{};
        o.radius_search = options_pc.radius_search_;
        o.min_num_neighbors = options_pc.min_num_neighbors_;
        size_t n = 0, rejected = 0;
        check(dsi_map_integrate_mapper(h_, mapper.handle(), &o, T_w_rv.data(), &n, &rejected));
        if (n_points) *n_points = n;
        return rejected;
    }
    size_t count(uint32_t min_points = 1, uint32_t min_windows = 1) const
    {
        size_t n = 0;
        check(dsi_map_count(h_, min_points, min_windows, &n));
        return n;
    }
    // the cells with n >= min_points and windows >= min_windows; sort: by ascending key (reproducible files)
    WorldMapCells extract(uint32_t min_points = 1, uint32_t min_windows = 1, bool sort = true) const
    {
        WorldMapCells out;
        size_t n = count(min_points, min_windows);
        out.xyz.resize(3 * n);
        out.n.resize(n);
        out.windows.resize(n);
        out.keys.resize(n);
        check(dsi_map_extract(h_, min_points, min_windows, out.xyz.data(), out.n.data(), out.windows.data(), out.keys.data(), n, &n));
        if (sort) detail::sort_rows_by_key(out.keys, out.xyz, out.n, out.windows);
        return out;
    }
    dsi_map_info_t info() const { return detail::info_of<dsi_map_info_t>(dsi_map_info, h_); }
    void reset() { check(dsi_map_reset(h_)); }

    // the depth image the map presents to a pinhole camera (dsi_map_render; the arithmetic is stated in dsi_engine.h): the
    // images stay on the device for fetch_render and DepthScore::addMapRender until the map changes
    MapRenderInfo render(const MapView& view)
    {
        const MapRenderInfo info = detail::info_of<MapRenderInfo>(dsi_map_render, h_, &view);
        width_ = info.width;
        height_ = info.height;
        return info;
    }
    // the last render's images, height * width elements each; any may be nullptr
    void fetch_render(float* depth, uint32_t* windows = nullptr, uint32_t* hits = nullptr, uint8_t* mask = nullptr) const
    {
        check(dsi_map_render_fetch(h_, depth, windows, hits, mask));
    }
    MapRenderImages fetch_render() const
    {
        MapRenderImages out;
        out.width = width_;
        out.height = height_;
        const size_t n = (size_t)width_ * (size_t)height_;
        out.depth.resize(n);
        out.windows.resize(n);
        out.hits.resize(n);
        out.mask.resize(n);
        fetch_render(out.depth.data(), out.windows.data(), out.hits.data(), out.mask.data());
        return out;
    }

    // one call of a host depth image (height x width, row-major; mask may be nullptr) seen by a pinhole camera at T_w_c
    // (dsx_map_integrate_depth): bit for bit integrate() of the back-projected float32 points.  Returns the number of pixels
    // integrated; *n_rejected: those of them rejected
    uint64_t integrateDepth(const float* depth, const uint8_t* mask, int width, int height, double fx, double fy, double cx, double cy,
                            double min_depth, double max_depth, const std::array<double, 12>& T_w_c, uint64_t* n_rejected = nullptr)
    {
        uint64_t n = 0;
        check(dsx_map_integrate_depth(h_, depth, mask, width, height, fx, fy, cx, cy, min_depth, max_depth, T_w_c.data(), &n, n_rejected));
        return n;
    }
    // the same of the depth map the projector last made, where it lies on the device, at the projector's size
    uint64_t integrateGroundTruth(const GroundTruthProjector& projector, double fx, double fy, double cx, double cy, double min_depth,
                                  double max_depth, const std::array<double, 12>& T_w_c, uint64_t* n_rejected = nullptr)
    {
        uint64_t n = 0;
        check(dsx_map_integrate_depth_gt(h_, projector.handle(), fx, fy, cx, cy, min_depth, max_depth, T_w_c.data(), &n, n_rejected));
        return n;
    }
    // every filtered cell of this map against the nearest centroid of `other` within opts.radius (dsx_map_compare; the
    // arithmetic is stated in dsi_map_eval.h); the distances stay on the device for fetchDistances until this map changes
    MapCompareResult compare(const WorldMap& other, const MapCompareOptions& opts)
    {
        MapCompareResult r;
        r.radius = opts.radius;
        r.hist.assign(opts.n_bins > 0 ? (size_t)opts.n_bins : 0, 0);
        check(dsx_map_compare(h_, other.h_, &opts, r.hist.empty() ? nullptr : r.hist.data(), &r.info));
        return r;
    }
    // (key, dist) of the last compare of this map; sort: by ascending key
    MapDistances fetchDistances(bool sort = true) const
    {
        MapDistances out;  // (the values come before the keys in this entry point and in dsx_map_prune_fetch)
        detail::fetch_rows([&](size_t room, size_t* n) { return dsx_map_compare_fetch(h_, detail::ptr(out.dist), detail::ptr(out.keys), room, n); },
                           [&](size_t n) { out.keys.resize(n), out.dist.resize(n); });
        if (sort) detail::sort_rows_by_key(out.keys, out.dist);
        return out;
    }

    // removes the cells that fail opts and rebuilds the table around the rest (dsx_map_prune; the rule is stated in
    // dsi_map_prune.h); render, compare and classification of the map are invalid afterwards
    MapPruneInfo prune(const MapPruneOptions& opts = MapPruneOptions())
    {
        return detail::info_of<MapPruneInfo>(dsx_map_prune, h_, &opts);
    }
    // prune's dry run (dsx_map_prune_classify): the same counts, the map unchanged; the verdicts stay on the device for
    // fetchPruneReasons until the map changes
    MapPruneInfo classifyPrune(const MapPruneOptions& opts = MapPruneOptions())
    {
        return detail::info_of<MapPruneInfo>(dsx_map_prune_classify, h_, &opts);
    }
    // (key, reason) of every cell from the last classifyPrune of this map; sort: by ascending key
    MapPruneReasons fetchPruneReasons(bool sort = true) const
    {
        MapPruneReasons out;
        detail::fetch_rows([&](size_t room, size_t* n) { return dsx_map_prune_fetch(h_, detail::ptr(out.reason), detail::ptr(out.keys), room, n); },
                           [&](size_t n) { out.keys.resize(n), out.reason.resize(n); });
        if (sort) detail::sort_rows_by_key(out.keys, out.reason);
        return out;
    }

    // labels the map's connected components (dsx_map_components; the rule is stated in dsi_map_components.h); the labelling
    // stays on the device until the map changes, and nothing else of the map changes
    MapComponentsInfo components(const MapComponentsOptions& opts = MapComponentsOptions())
    {
        return detail::info_of<MapComponentsInfo>(dsx_map_components, h_, &opts);
    }
    // (key, label) of every labelled cell from the last components() of this map, and with_reasons -- after a
    // selectComponents on it -- the selection's reason; sort: by ascending key
    MapComponentLabels fetchComponents(bool with_reasons = false, bool sort = true) const
    {
        MapComponentLabels out;
        uint8_t none = 0, *reasons = nullptr;  // (no vector's data(): without a row it may be null, which would not ask for the reasons)
        detail::fetch_rows([&](size_t room, size_t* n) { return dsx_map_components_fetch(h_, detail::ptr(out.keys), detail::ptr(out.labels), reasons, room, n); },
                           [&](size_t n) {
                               out.keys.resize(n), out.labels.resize(n);
                               if (with_reasons) out.reason.resize(n), reasons = n ? out.reason.data() : &none;
                           });
        if (sort) detail::sort_rows_by_key(out.keys, out.labels, out.reason);
        return out;
    }
    // (label, cells, points) of every component from the last components() of this map, by cells descending, then label
    // ascending
    MapComponentList listComponents() const
    {
        MapComponentList out;
        const size_t n = detail::fetch_rows(
            [&](size_t room, size_t* m) { return dsx_map_components_list(h_, detail::ptr(out.labels), detail::ptr(out.cells), detail::ptr(out.points), room, m); },
            [&](size_t m) { out.labels.resize(m), out.cells.resize(m), out.points.resize(m); });
        detail::sort_rows(n, [&](size_t a, size_t b) { return out.cells[a] != out.cells[b] ? out.cells[a] > out.cells[b] : out.labels[a] < out.labels[b]; },
                          out.labels, out.cells, out.points);
        return out;
    }
    // pruneComponents' dry run (dsx_map_components_select): the same counts, the map unchanged; the reasons stay on the
    // device for fetchComponents(true) until the map changes
    MapComponentsSelectInfo selectComponents(const MapComponentsSelection& sel = MapComponentsSelection())
    {
        return detail::info_of<MapComponentsSelectInfo>(dsx_map_components_select, h_, &sel);
    }
    // removes the cells that the selection rejects and rebuilds the table around the rest (dsx_map_prune_components);
    // render, compare, alignment, classification and labelling of the map are invalid afterwards
    MapComponentsSelectInfo pruneComponents(const MapComponentsSelection& sel = MapComponentsSelection())
    {
        return detail::info_of<MapComponentsSelectInfo>(dsx_map_prune_components, h_, &sel);
    }

    // the k nearest cells of n host points, stride 3 or 4 floats (dsx_map_knn_points; the rule is stated in dsi_map_knn.h);
    // reads the map only
    MapNeighbours query(const float* xyz, size_t stride_floats, size_t n, const MapKnnOptions& opts) const
    {
        MapNeighbours out;
        out.k = opts.k;
        const size_t rows = opts.k > 0 ? n * (size_t)opts.k : 0;
        out.keys.assign(rows, 0);
        out.dist.assign(rows, std::numeric_limits<float>::infinity());
        out.found.assign(n, 0);
        check(dsx_map_knn_points(h_, xyz, stride_floats, n, &opts, out.keys.data(), out.dist.data(), out.found.data()));
        return out;
    }
    // the self query (dsx_map_knn): every cell asks for its k nearest other cells; the result stays on the device for
    // pruneOutliers until the map changes, and nothing else of the map changes
    MapKnnInfo knn(const MapKnnOptions& opts)
    {
        return detail::info_of<MapKnnInfo>(dsx_map_knn, h_, &opts);
    }
    // removes the isolated cells and the statistical outliers of the last knn() and rebuilds the table around the rest
    // (dsx_map_prune_knn); everything derived from the map is invalid afterwards
    MapKnnSelectInfo pruneOutliers(const MapKnnSelection& sel = MapKnnSelection())
    {
        return detail::info_of<MapKnnSelectInfo>(dsx_map_prune_knn, h_, &sel);
    }

    // the local shape of every cell (dsx_map_pca; the rule is stated in dsi_map_pca.h): the result stays on the device for
    // fetchPca and pruneShapes until the map changes, and nothing else of the map changes
    MapPcaInfo pca(const MapPcaOptions& opts)
    {
        const MapPcaInfo info = detail::info_of<MapPcaInfo>(dsx_map_pca, h_, &opts);
        pca_moments_ = opts.keep_moments != 0;
        return info;
    }
    // the rows of the last pca() (dsx_map_pca_fetch)
    MapShapes fetchPca() const
    {
        MapShapes out;  // (without a row the second call is left out, which the Python binding makes)
        detail::fetch_rows(
            [&](size_t room, size_t* n) {
                return dsx_map_pca_fetch(h_, detail::ptr(out.keys), detail::ptr(out.normal), detail::ptr(out.tangent), detail::ptr(out.eval),
                                         detail::ptr(out.members), detail::ptr(out.label), detail::ptr(out.flags), detail::ptr(out.moments),
                                         nullptr, room, n);
            },
            [&](size_t n) {
                out.keys.resize(n), out.normal.resize(3 * n), out.tangent.resize(3 * n), out.eval.resize(3 * n);
                out.members.resize(n), out.label.resize(n), out.flags.resize(n);
                if (pca_moments_) out.moments.resize(9 * n);
            },
            false);
        return out;
    }
    // keeps the cells of the last pca() whose label is in the selection and rebuilds the table around them
    // (dsx_map_prune_pca); everything derived from the map is invalid afterwards
    MapPcaSelectInfo pruneShapes(const MapPcaSelection& sel = MapPcaSelection())
    {
        return detail::info_of<MapPcaSelectInfo>(dsx_map_prune_pca, h_, &sel);
    }

    // what one host depth image (height x width, row-major; mask may be nullptr) says about every cell (dsx_map_observe; the
    // rule is stated in dsi_map_visibility.h): the verdicts accumulate per cell until the map changes or clearVisibility(),
    // and nothing else of the map changes
    MapObserveInfo observe(const float* depth, const uint8_t* mask, const MapObservation& obs)
    {
        visibility_selected_ = false;
        return detail::info_of<MapObserveInfo>(dsx_map_observe, h_, depth, mask, &obs);
    }
    // the same of the filtered depth map and mask the mapper left on the device, read where they lie (dsx_map_observe_mapper)
    template <typename MapperT>
    MapObserveInfo observeMapper(MapperT& mapper, const MapObservation& obs)
    {
        visibility_selected_ = false;
        return detail::info_of<MapObserveInfo>(dsx_map_observe_mapper, h_, mapper.handle(), &obs);
    }
    void clearVisibility()
    {
        visibility_selected_ = false;
        check(dsx_map_visibility_clear(h_));
    }
    // the tally of every cell (dsx_map_visibility_fetch); sort: by ascending key
    MapVisibility fetchVisibility(bool sort = true) const
    {
        MapVisibility out;
        detail::fetch_rows(
            [&](size_t room, size_t* n) {
                return dsx_map_visibility_fetch(h_, detail::ptr(out.keys), detail::ptr(out.seen), detail::ptr(out.agree), detail::ptr(out.through),
                                                detail::ptr(out.reason), room, n);
            },
            [&](size_t n) {
                out.keys.resize(n), out.seen.resize(n), out.agree.resize(n), out.through.resize(n);
                if (visibility_selected_) out.reason.resize(n);
            });
        if (sort) detail::sort_rows_by_key(out.keys, out.seen, out.agree, out.through, out.reason);
        return out;
    }
    // pruneCarved()'s dry run (dsx_map_visibility_select): the same counts, the map unchanged
    MapVisibilitySelectInfo selectCarved(const MapVisibilitySelection& sel = MapVisibilitySelection())
    {
        visibility_selected_ = false;
        const MapVisibilitySelectInfo info = detail::info_of<MapVisibilitySelectInfo>(dsx_map_visibility_select, h_, &sel);
        visibility_selected_ = true;
        return info;
    }
    // removes the cells that the observed views look through and rebuilds the table around the rest
    // (dsx_map_prune_visibility); everything derived from the map is invalid afterwards
    MapVisibilitySelectInfo pruneCarved(const MapVisibilitySelection& sel = MapVisibilitySelection())
    {
        visibility_selected_ = false;
        return detail::info_of<MapVisibilitySelectInfo>(dsx_map_prune_visibility, h_, &sel);
    }

    // appends `other` (same context, same leaf) to this map on the device (dsx_map_merge; the rule is stated in
    // dsi_map_merge.h): this map becomes the map that had made its own integrate calls and then other's.  other is
    // unchanged; render, compare and classification of this map are invalid afterwards
    MapMergeInfo merge(const WorldMap& other) { return detail::info_of<MapMergeInfo>(dsx_map_merge, h_, other.h_); }
    // the map's exact state (dsx_map_export); sort: by ascending key.  Changes nothing
    MapState exportState(bool sort = true) const
    {
        MapState out;
        dsx_map_state_t st;
        detail::fetch_rows(
            [&](size_t room, size_t* m) {
                return dsx_map_export(h_, &st, detail::ptr(out.keys), detail::ptr(out.n), detail::ptr(out.S), detail::ptr(out.windows),
                                      detail::ptr(out.stamp), room, m);
            },
            [&](size_t m) { out.keys.resize(m), out.n.resize(m), out.S.resize(3 * m), out.windows.resize(m), out.stamp.resize(m); });
        out.leaf = st.leaf;
        out.calls = st.calls, out.accepted = st.accepted, out.rejected = st.rejected;
        if (sort) detail::sort_rows_by_key(out.keys, out.n, out.S, out.windows, out.stamp);
        return out;
    }
    // appends an exported state as merge appends the map it came from (dsx_map_import): into an empty map without calls
    // it restores that map.  The state is validated on the device; a refused state leaves this map unchanged
    MapMergeInfo importState(const MapState& state)
    {
        const size_t m = state.keys.size();
        if (state.n.size() != m || state.windows.size() != m || state.stamp.size() != m || state.S.size() != 3 * m)
            throw Error(DSI_ERR_INVALID, "MapState: keys, n, windows and stamp need one entry per cell and S three");
        const dsx_map_state_t st{state.leaf, (uint64_t)m, state.calls, state.accepted, state.rejected};
        return detail::info_of<MapMergeInfo>(dsx_map_import, h_, &st, state.keys.data(), state.n.data(), state.S.data(), state.windows.data(),
                                             state.stamp.data());
    }

    // one correspondence pass of ICP (dsx_map_align_step; the arithmetic is stated in dsi_map_align.h): every filtered
    // cell of this map, moved by T (this map's frame in other's), against the nearest filtered centroid of `other` within
    // opts.radius; the exact integer moments of the matched pairs come back, the pairs stay on the device
    MapAlignMoments align_step(const WorldMap& other, const MapAlignOptions& opts, const std::array<double, 12>& T = kIdentityPose)
    {
        return detail::info_of<MapAlignMoments>(dsx_map_align_step, h_, other.h_, &opts, T.data());
    }
    // ICP of this map onto `other` from T_init (dsx_map_align).  A round with too few matched cells or degenerate pairs
    // does not throw: the result then has ok == false, the last good pose and info.stopped; every other error throws
    MapAlignResult align(const WorldMap& other, const MapAlignOptions& opts, const std::array<double, 12>& T_init = kIdentityPose)
    {
        MapAlignResult r;
        const int rc = dsx_map_align(h_, other.h_, &opts, T_init.data(), r.T.data(), &r.info);
        if (rc != DSI_OK && !(rc == DSI_ERR_INVALID && r.info.stopped != 0)) check(rc);
        r.ok = rc == DSI_OK;
        return r;
    }
    // one integrate call of other's filtered cells, each as its float32 centroid, under T (other's frame in this map's) on
    // the device (dsx_map_integrate_map): bit for bit integrate() of other.extract()'s xyz.  Returns the cells integrated
    uint64_t integrate_map(const WorldMap& other, const std::array<double, 12>& T = kIdentityPose, uint32_t min_points = 1,
                           uint32_t min_windows = 1, uint64_t* n_rejected = nullptr)
    {
        uint64_t n = 0;
        check(dsx_map_integrate_map(h_, other.h_, T.data(), min_points, min_windows, &n, n_rejected));
        return n;
    }

private:
    Context& ctx_;
    dsi_map_t* h_ = nullptr;
    int width_ = 0, height_ = 0;  // of the last render
    bool pca_moments_ = false;    // the last pca() kept its moments
    bool visibility_selected_ = false;  // a selectCarved() left reasons beside the tally
};

// 3-D accuracy, completeness and F-score of the map `est` against the map `gt` (the curves of the reference's
// scripts/precision_completeness.py:44,60,76 taken in space): one compare per direction, then, from the integer counts,
// thresholds (i + 1) * radius / n_bins, precision = 100 cumsum(hist_est) / n_cells_est, recall = 100 cumsum(hist_gt) /
// n_cells_gt, f1 = 2 P R / (P + R), 0 where P + R == 0.  opts: the filters with a = est and b = gt, radius, n_bins.
struct MapFScore {
    std::vector<double> thresholds, precision, recall, f1;
    MapCompareResult est, gt;
};
inline MapFScore map_f_score(WorldMap& est, WorldMap& gt, const MapCompareOptions& opts)
{
    MapCompareOptions back = opts;
    back.min_points_a = opts.min_points_b, back.min_windows_a = opts.min_windows_b;
    back.min_points_b = opts.min_points_a, back.min_windows_b = opts.min_windows_a;
    MapFScore f;
    f.est = est.compare(gt, opts);
    f.gt = gt.compare(est, back);
    const double w = opts.radius / (double)opts.n_bins;
    uint64_t ce = 0, cg = 0;
    for (int i = 0; i < opts.n_bins; ++i) {
        ce += f.est.hist[(size_t)i];
        cg += f.gt.hist[(size_t)i];
        const double P = f.est.info.n_cells ? 100.0 * (double)ce / (double)f.est.info.n_cells : 0.0;
        const double R = f.gt.info.n_cells ? 100.0 * (double)cg / (double)f.gt.info.n_cells : 0.0;
        f.thresholds.push_back(((double)i + 1.0) * w);
        f.precision.push_back(P);
        f.recall.push_back(R);
        f.f1.push_back(P + R > 0.0 ? 2.0 * P * R / (P + R) : 0.0);
    }
    return f;
}

}  // namespace dsi

// the reference's spellings (utils.hpp:23-52), on the process-wide default context: main.cpp:249-250 and
// process1.cpp:209-223 compile as they stand
template <typename EventT, typename ImgT>
inline void accumulateEvents(const std::vector<EventT>& events, const bool use_polarity, ImgT& img)
{
    dsi::accumulateEvents(dsi::default_context(), events, use_polarity, img);
}
template <typename DepthImg, typename ConfImg, typename MaskImg>
inline void saveDepthMaps(const DepthImg& depth_map, const ConfImg& confidence_map, const MaskImg& semidense_mask,
                          const float min_depth, const float max_depth, const std::string& suffix, const std::string& out_path)
{
    dsi::saveDepthMaps(dsi::default_context(), depth_map, confidence_map, semidense_mask, min_depth, max_depth, suffix, out_path);
}
// (depth_map_dense is not used by the reference's body either: its block is commented out, utils.cpp:95-103)
template <typename DepthImg, typename ConfImg, typename MaskImg, typename DenseImg>
inline void saveDepthMaps(const DepthImg& depth_map, const ConfImg& confidence_map, const MaskImg& semidense_mask,
                          const DenseImg& /*depth_map_dense*/, const float min_depth, const float max_depth,
                          const std::string& suffix, const std::string& out_path)
{
    dsi::saveDepthMaps(dsi::default_context(), depth_map, confidence_map, semidense_mask, min_depth, max_depth, suffix, out_path);
}
