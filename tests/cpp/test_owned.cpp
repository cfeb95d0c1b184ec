// test_owned.cpp -- the owning types of dvs_mcemvs_amd/csrc/dsi_owned.hpp against counting fakes of the eight HIP
// runtime calls the header makes.  Host code only: no HIP runtime is linked and no GPU is needed, so the program runs
// under the address and undefined-behaviour sanitizers (tests/test_owned_cpu.py builds it that way).
//
// Every fake allocation is a malloc'd token kept in a table; giving back a pointer or handle that is not in the table
// (a second free, a free of something never made) counts as an error.  The program exits non-zero unless every check
// held and every token was given back exactly once.
#include "../../dvs_mcemvs_amd/csrc/dsi_owned.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

namespace {

enum Kind { kDevice, kPinned, kEvent, kStream };
const char* const kKindName[] = {"device memory", "pinned memory", "event", "stream"};

std::map<void*, Kind> g_live;
int g_made[4] = {0, 0, 0, 0}, g_freed[4] = {0, 0, 0, 0};
int g_errors = 0;
int g_fail_next = 0;  // > 0: the next creating call fails

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_errors;                                                    \
        }                                                                  \
    } while (0)

hipError_t make(Kind k, void** out, size_t bytes)
{
    if (g_fail_next > 0) {
        --g_fail_next;
        return hipErrorOutOfMemory;
    }
    void* p = std::malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    g_live[p] = k;
    ++g_made[k];
    *out = p;
    return hipSuccess;
}

hipError_t give_back(Kind k, void* p)
{
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != k) {
        std::printf("%s %p given back but not live\n", kKindName[k], p);
        ++g_errors;
        return hipErrorInvalidValue;
    }
    g_live.erase(it);
    ++g_freed[k];
    std::free(p);
    return hipSuccess;
}

int live() { return (int)g_live.size(); }

}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return make(kDevice, ptr, size); }
hipError_t hipFree(void* ptr) { return give_back(kDevice, ptr); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return make(kPinned, ptr, size); }
hipError_t hipHostFree(void* ptr) { return give_back(kPinned, ptr); }
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned) { return make(kEvent, reinterpret_cast<void**>(event), 8); }
hipError_t hipEventDestroy(hipEvent_t event) { return give_back(kEvent, event); }
hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int) { return make(kStream, reinterpret_cast<void**>(stream), 8); }
hipError_t hipStreamDestroy(hipStream_t stream) { return give_back(kStream, stream); }
}

namespace {

using dsi::DevBuf;
using dsi::Event;
using dsi::HostPinned;
using dsi::Stream;

// `x = std::move(x)` without the compiler's self-move warning
template <typename T>
void self_move(T& x)
{
    T* alias = &x;
    x = std::move(*alias);
}

void test_devbuf_moves()
{
    {
        DevBuf<float> a;
        CHECK(a.p == nullptr && a.cap == 0);
        CHECK(a.reserve(10) == hipSuccess && a.p && a.cap == 10);
        a.p[9] = 1.f;  // (the fake really holds 10 floats: the sanitizer checks the size arithmetic)
        float* const pa = a.p;
        DevBuf<float> b(std::move(a));  // move construction
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 10);
        DevBuf<float> c;
        c = std::move(b);  // move assignment onto an empty target
        CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 10);
        self_move(c);
        CHECK(c.p == pa && c.cap == 10 && live() == 1);
        DevBuf<float> d;
        CHECK(d.reserve(3) == hipSuccess && live() == 2);
        d = std::move(c);  // onto a non-empty target: its buffer goes first
        CHECK(live() == 1 && d.p == pa && d.cap == 10 && c.p == nullptr);
        a = std::move(c);  // empty onto empty
        CHECK(a.p == nullptr && live() == 1);
    }
    CHECK(live() == 0);
}

void test_devbuf_reserve()
{
    {
        DevBuf<double> a;
        CHECK(a.reserve(0) == hipSuccess && a.p == nullptr && live() == 0);
        CHECK(a.reserve(4) == hipSuccess && a.cap == 4);
        double* const p4 = a.p;
        CHECK(a.reserve(3) == hipSuccess && a.p == p4 && a.cap == 4);  // grow-only: a smaller request keeps the buffer
        CHECK(a.reserve(4) == hipSuccess && a.p == p4);
        const int freed = g_freed[kDevice];
        CHECK(a.reserve(100) == hipSuccess && a.cap == 100 && live() == 1);  // growth frees first
        CHECK(g_freed[kDevice] == freed + 1);
        a.p[99] = 2.0;
        // a failing growth leaves the buffer empty (the old block is gone, as the engine expects) and reusable
        g_fail_next = 1;
        CHECK(a.reserve(1000) == hipErrorOutOfMemory);
        CHECK(a.p == nullptr && a.cap == 0 && live() == 0);
        CHECK(a.reserve(1000) == hipSuccess && a.cap == 1000 && live() == 1);
        a.release();
        CHECK(a.p == nullptr && a.cap == 0 && live() == 0);
        a.release();  // twice is fine
        g_fail_next = 1;
        CHECK(a.reserve(1) == hipErrorOutOfMemory && a.p == nullptr && a.cap == 0);  // a failing first allocation
        CHECK(a.reserve(2) == hipSuccess && live() == 1);
    }
    CHECK(live() == 0);
}

// what dsi_mapper::BatchTables is: several buffers in a struct, the structs in a vector that reallocates
struct Tables {
    DevBuf<float> centers;
    DevBuf<unsigned> nvalid, cuts;
    DevBuf<unsigned short> rowstart;
};

void test_vector_of_structs()
{
    {
        std::vector<Tables> v;
        v.resize(1);
        CHECK(v[0].centers.reserve(5) == hipSuccess && v[0].cuts.reserve(7) == hipSuccess);
        float* const p0 = v[0].centers.p;
        for (size_t n = 2; n <= 40; ++n) {  // past the capacity several times: the elements are relocated by move
            v.resize(n);
            CHECK(v[n - 1].centers.p == nullptr);
            CHECK(v[n - 1].centers.reserve(n) == hipSuccess && v[n - 1].rowstart.reserve(n) == hipSuccess);
        }
        CHECK(v[0].centers.p == p0 && v[0].centers.cap == 5 && v[0].cuts.cap == 7);
        CHECK(live() == 2 + 2 * 39);
        v.resize(3);  // shrinking destroys the tail
        CHECK(live() == 2 + 2 * 2);
        v.erase(v.begin());  // move-assigns the rest down
        CHECK(live() == 2 * 2 && v[0].centers.cap == 2 && v[1].centers.cap == 3);
        std::vector<Tables> w(std::move(v));
        CHECK(live() == 2 * 2 && w.size() == 2);
    }
    CHECK(live() == 0);
}

void test_c_array()
{
    {
        struct Scratch {
            DevBuf<unsigned> votes[8];  // TieScratch::votes
        } s;
        for (int c = 0; c < 8; c += 2) CHECK(s.votes[c].reserve(16 + c) == hipSuccess);
        CHECK(live() == 4);
        Scratch t(std::move(s));
        CHECK(live() == 4 && s.votes[0].p == nullptr && t.votes[2].cap == 18 && t.votes[1].p == nullptr);
    }
    CHECK(live() == 0);
}

template <typename H, typename Create>
void test_handle(Kind k, Create create)
{
    {
        H a;
        CHECK(!a && a.h == nullptr);
        CHECK(create(a) == hipSuccess && a && live() == 1);
        const auto ha = a.h;
        H b(std::move(a));
        CHECK(!a && b.h == ha);
        H c;
        c = std::move(b);
        CHECK(!b && c.h == ha);
        self_move(c);
        CHECK(c.h == ha && live() == 1);
        H d;
        CHECK(create(d) == hipSuccess && live() == 2);
        d = std::move(c);  // onto a non-empty target
        CHECK(live() == 1 && d.h == ha && !c);
        CHECK(create(d) == hipSuccess && live() == 1 && d.h);  // creating again gives the first back
        g_fail_next = 1;
        CHECK(create(d) != hipSuccess && !d && live() == 0);  // a failed creation leaves it empty ...
        CHECK(create(d) == hipSuccess && live() == 1);        // ... and reusable
        d.release();
        CHECK(!d && live() == 0);
        d.release();
        // in a vector that reallocates, then shrinks (dsi_context::marks, dsi_mapper::timing_pool)
        std::vector<H> v;
        for (int i = 0; i < 20; ++i) {
            H e;
            CHECK(create(e) == hipSuccess);
            v.push_back(std::move(e));
        }
        CHECK(live() == 20);
        H back = std::move(v.back());
        v.pop_back();
        CHECK(live() == 20 && back);
        v.resize(5);
        CHECK(live() == 6);
        H arr[3];
        CHECK(create(arr[1]) == hipSuccess && live() == 7);
    }
    CHECK(live() == 0);
    CHECK(g_made[k] == g_freed[k] && g_made[k] > 0);
}

}  // namespace

int main()
{
    test_devbuf_moves();
    test_devbuf_reserve();
    test_vector_of_structs();
    test_c_array();
    test_handle<Event>(kEvent, [](Event& e) { return e.create(hipEventDisableTiming); });
    test_handle<Stream>(kStream, [](Stream& s) { return s.create(hipStreamNonBlocking); });
    test_handle<HostPinned<unsigned>>(kPinned, [](HostPinned<unsigned>& h) {
        const hipError_t e = h.alloc(64, hipHostMallocDefault);
        if (e == hipSuccess) h.h[63] = 7u;
        return e;
    });
    for (int k = 0; k < 4; ++k) {
        std::printf("%-14s made %3d  given back %3d\n", kKindName[k], g_made[k], g_freed[k]);
        CHECK(g_made[k] == g_freed[k] && g_made[k] > 0);
    }
    CHECK(g_live.empty());
    if (g_errors) {
        std::printf("FAILED: %d error(s)\n", g_errors);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
