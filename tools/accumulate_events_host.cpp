// The reference's accumulateEvents (utils.cpp:184-216) restated as the plain single-thread loop it is, over
// std::vector<Event>: the host yardstick of tools/run_images_bench.py.  Prints one JSON line per case.
//   accumulate_events_host WIDTH HEIGHT N_EVENTS HOT_PIXELS REPS      (HOT_PIXELS 0: events spread over the sensor)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Event {  // dvs_msgs::Event's fields
    uint16_t x, y;
    double ts;
    bool polarity;
};

static void accumulateEvents(const std::vector<Event>& events, int width, int height, std::vector<float>& imgf, std::vector<uint8_t>& img)
{
    std::fill(imgf.begin(), imgf.end(), 0.f);
    for (auto e : events) imgf[(size_t)e.y * width + e.x] += (e.polarity ? 1 : -1);
    const auto mm = std::minmax_element(imgf.begin(), imgf.end());
    const double half_range = std::max(std::fabs((double)*mm.first), std::fabs((double)*mm.second));
    if (half_range > 0) {
        const float a = (float)(128 / half_range);
        for (size_t i = 0; i < (size_t)width * height; ++i) {
            const float r = std::nearbyint(imgf[i] * a + 128.f);
            img[i] = (uint8_t)(r < 0.f ? 0 : (r > 255.f ? 255 : (int)r));
        }
    } else {
        std::fill(img.begin(), img.end(), (uint8_t)128);
    }
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int width = std::atoi(argv[1]), height = std::atoi(argv[2]);
    const size_t n = (size_t)std::atoll(argv[3]);
    const int hot = std::atoi(argv[4]), reps = std::atoi(argv[5]);
    uint64_t s = 12345;
    auto next = [&s] {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (uint32_t)(s >> 33);
    };
    std::vector<uint32_t> hot_px((size_t)std::max(hot, 1));
    for (auto& p : hot_px) p = next() % (uint32_t)(width * height);
    std::vector<Event> events(n);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t p = hot ? hot_px[next() % (uint32_t)hot] : next() % (uint32_t)(width * height);
        events[i] = Event{(uint16_t)(p % (uint32_t)width), (uint16_t)(p / (uint32_t)width), 1e-6 * (double)i, (next() & 1u) != 0};
    }
    std::vector<float> imgf((size_t)width * height);
    std::vector<uint8_t> img((size_t)width * height);
    accumulateEvents(events, width, height, imgf, img);
    double best = 1e30, total = 0;
    unsigned sum = 0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        accumulateEvents(events, width, height, imgf, img);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        best = std::min(best, ms);
        total += ms;
        sum += img[(size_t)r % img.size()];
    }
    std::printf("{\"op\": \"host_loop\", \"sensor\": \"%dx%d\", \"events\": %zu, \"hot_pixels\": %d, \"ms\": %.4f, \"ms_best\": %.4f, \"check\": %u}\n",
                width, height, n, hot, total / reps, best, sum);
    return 0;
}
