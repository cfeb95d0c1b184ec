// The run's pictures through the C++ adapter at the reference's call sites: accumulateEvents spelled as main.cpp:246-250
// spells it and saveDepthMaps in both signatures (process1.cpp:209-223, utils.hpp), with a stand-in of cv::Mat (no OpenCV
// here), checked against the C ABI with memcmp.  Run by tests/test_gpu_run_images.py, which compares what this program
// writes with the numpy restatement.
//   test_run_images DIR    events.{x.u16,y.u16,p.u8}, event_image.u8, depth.f32 conf.f32 mask.u8, neg.u8 bgr.u8 and
//                          saveDepthMaps' files with out_path DIR/ and suffixes "a" (7 arguments) and "b" (8 arguments)
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "dsi_engine.hpp"

#define CV_8U 0
#define CV_32F 5
#define CV_8UC1 CV_8U
#define CV_32FC1 CV_32F

namespace cv {  // the members of cv::Mat the reference's call sites and the adapter's customisation points use
struct Size {
    int width = 0, height = 0;
    Size(int w, int h) : width(w), height(h) {}
};
class Mat {
public:
    int rows = 0, cols = 0;
    Mat() = default;
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(Size s, int type) { create(s.height, s.width, type); }
    void create(int r, int c, int type)
    {
        if (type != CV_8U && type != CV_32F) throw std::runtime_error("cv::Mat look-alike: type not CV_8U / CV_32F");
        rows = r;
        cols = c;
        type_ = type;
        buf_ = std::make_shared<std::vector<unsigned char>>((size_t)r * c * (type == CV_32F ? 4 : 1));
    }
    void release()
    {
        buf_.reset();
        rows = cols = 0;
    }
    bool isContinuous() const { return true; }
    template <typename T>
    T* ptr(int row = 0)
    {
        if ((type_ == CV_32F) != (sizeof(T) == 4)) throw std::runtime_error("cv::Mat look-alike: wrong element type");
        return reinterpret_cast<T*>(buf_->data()) + (size_t)row * cols;
    }
    template <typename T>
    T& at(int r, int c)
    {
        return ptr<T>(r)[c];
    }

private:
    int type_ = CV_8U;
    std::shared_ptr<std::vector<unsigned char>> buf_;
};
}  // namespace cv

namespace dvs_msgs {
struct Event {
    uint16_t x, y;
    double ts;
    bool polarity;
};
}  // namespace dvs_msgs

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

bool exists(const std::string& path)
{
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        std::fclose(f);
        return true;
    }
    return false;
}

struct Lcg {
    uint64_t s;
    double uni()
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) / 9007199254740992.0;
    }
};

int run(const std::string& dir)
{
    const int W = 70, H = 9;
    Lcg rng{5};
    // ---- accumulateEvents, main.cpp:246-250
    std::vector<dvs_msgs::Event> interval_events0;
    std::vector<uint16_t> x, y;
    std::vector<uint8_t> p;
    for (int i = 0; i < 5000; ++i) {
        dvs_msgs::Event e;
        e.x = (uint16_t)(rng.uni() * (W + 2));  // a few outside the sensor
        e.y = (uint16_t)(rng.uni() * H);
        e.ts = 1e-4 * i;
        e.polarity = rng.uni() < 0.6;
        interval_events0.push_back(e);
        x.push_back(e.x);
        y.push_back(e.y);
        p.push_back(e.polarity ? 1 : 0);
    }
    cv::Size full_resolution(W, H);
    for (int use_polarity = 0; use_polarity < 2; ++use_polarity) {
        cv::Mat event_image0 = cv::Mat(full_resolution, CV_8UC1);
        accumulateEvents(interval_events0, use_polarity != 0, event_image0);
        std::vector<uint8_t> abi((size_t)W * H);
        size_t dropped = 0;
        dsi::check(dsi_event_image(dsi::default_context().handle(), x.data(), y.data(), p.data(), x.size(), W, H, use_polarity,
                                   abi.data(), &dropped));
        EXPECT(dropped > 0 && dropped < x.size());
        EXPECT(std::memcmp(abi.data(), event_image0.ptr<uint8_t>(0), abi.size()) == 0);
        dsi::Image<uint8_t> own(H, W);
        EXPECT(dsi::accumulateEvents(dsi::default_context(), interval_events0, use_polarity != 0, own) == dropped);
        EXPECT(std::memcmp(abi.data(), own.data.data(), abi.size()) == 0);
        write(dir + (use_polarity ? "/event_image.u8" : "/event_image_nopol.u8"), abi.data(), abi.size());
    }
    // an empty window (ordinary in the main.cpp:245-258 loop): 128 everywhere with polarity, 0 without; the batch form alike
    for (int use_polarity = 0; use_polarity < 2; ++use_polarity) {
        const std::vector<dvs_msgs::Event> none;
        cv::Mat empty_image = cv::Mat(full_resolution, CV_8UC1);
        std::memset(empty_image.ptr<uint8_t>(0), 77, (size_t)W * H);
        accumulateEvents(none, use_polarity != 0, empty_image);
        std::vector<uint8_t> abi((size_t)W * H, 77), of_batch((size_t)W * H, 77);
        size_t dropped = 9;
        dsi::check(dsi_event_image(dsi::default_context().handle(), nullptr, nullptr, nullptr, 0, W, H, use_polarity, abi.data(),
                                   &dropped));
        EXPECT(dropped == 0);
        dsi_batch_t* b = nullptr;
        dsi::check(dsi_batch_create(dsi::default_context().handle(), nullptr, nullptr, 0, nullptr, nullptr, 0, &b));
        dsi::check(dsi_batch_event_image(b, nullptr, W, H, use_polarity, of_batch.data(), &dropped));
        dsi::check(dsi_batch_destroy(b));
        EXPECT(dropped == 0);
        for (size_t i = 0; i < abi.size(); ++i) {
            const uint8_t want = use_polarity ? 128 : 0;
            EXPECT(abi[i] == want && of_batch[i] == want && empty_image.ptr<uint8_t>(0)[i] == want);
            if (abi[i] != want) break;
        }
    }
    write(dir + "/events.x.u16", x.data(), x.size() * 2);
    write(dir + "/events.y.u16", y.data(), y.size() * 2);
    write(dir + "/events.p.u8", p.data(), p.size());

    // ---- saveDepthMaps, process1.cpp:209-223
    const float min_depth = 4.f, max_depth = 200.f;
    cv::Mat depth_map(H, W, CV_32FC1), confidence_map(H, W, CV_32FC1), semidense_mask(H, W, CV_8UC1), depth_map_dense;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            depth_map.at<float>(r, c) = (float)(3.0 + 60.0 * rng.uni());
            confidence_map.at<float>(r, c) = (float)(40.0 * rng.uni());
            semidense_mask.at<uint8_t>(r, c) = rng.uni() < 0.2 ? 1 : 0;
        }
    const std::string out_path = dir + "/";
    saveDepthMaps(depth_map, confidence_map, semidense_mask, min_depth, max_depth, std::string("a"), out_path);
    saveDepthMaps(depth_map, confidence_map, semidense_mask, depth_map_dense, min_depth, max_depth, std::string("b"), out_path);
    for (const char* suffix : {"a", "b"}) {
        EXPECT(exists(out_path + "depth_points_" + suffix + ".txt"));
        EXPECT(exists(out_path + "confidence_map_negated_" + suffix + ".png"));
        EXPECT(exists(out_path + "inv_depth_colored_dilated_" + suffix + ".png"));
    }
    std::vector<uint8_t> neg, bgr, neg_abi((size_t)W * H), bgr_abi((size_t)W * H * 3);
    dsi::saveDepthMaps(dsi::default_context(), depth_map, confidence_map, semidense_mask, min_depth, max_depth, "c", out_path, &neg,
                       &bgr);
    dsi::check(dsi_depth_images(dsi::default_context().handle(), depth_map.ptr<float>(0), confidence_map.ptr<float>(0),
                                semidense_mask.ptr<uint8_t>(0), H, W, min_depth, max_depth, nullptr, neg_abi.data(), bgr_abi.data()));
    EXPECT(neg.size() == neg_abi.size() && std::memcmp(neg.data(), neg_abi.data(), neg.size()) == 0);
    EXPECT(bgr.size() == bgr_abi.size() && std::memcmp(bgr.data(), bgr_abi.data(), bgr.size()) == 0);
    write(dir + "/depth.f32", depth_map.ptr<float>(0), (size_t)W * H * 4);
    write(dir + "/conf.f32", confidence_map.ptr<float>(0), (size_t)W * H * 4);
    write(dir + "/mask.u8", semidense_mask.ptr<uint8_t>(0), (size_t)W * H);
    write(dir + "/neg.u8", neg_abi.data(), neg_abi.size());
    write(dir + "/bgr.u8", bgr_abi.data(), bgr_abi.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
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
