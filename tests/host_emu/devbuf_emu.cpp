// The owners of plan-owned memory (zafx_devbuf.hpp) over a counting allocator: malloc / free / memcpy, a count of live blocks, a log of the
// calls and a switch that makes the next allocation fail.  Prints "ok" and returns 0, or says which property broke.
//   g++ -std=c++17 -fsanitize=address,undefined -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/devbuf_emu.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "zafx_devbuf.hpp"

static long long g_live = 0, g_pinned_live = 0;
static bool g_fail_next = false;
static std::string g_log;   // 'a' device allocation, 'f' device free, 'c' copy, 'A' / 'F' the page-locked ones

namespace zafx {
hipError_t dev_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    ++g_live;
    g_log += 'a';
    return hipSuccess;
}
hipError_t dev_free(void* p) {
    std::free(p);
    --g_live;
    g_log += 'f';
    return hipSuccess;
}
hipError_t dev_copy_h2d(void* dst, const void* src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    g_log += 'c';
    return hipSuccess;
}
hipError_t pinned_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    ++g_pinned_live;
    g_log += 'A';
    return hipSuccess;
}
hipError_t pinned_free(void* p) {
    std::free(p);
    --g_pinned_live;
    g_log += 'F';
    return hipSuccess;
}
}  // namespace zafx

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s  (log %s)\n", __LINE__, #cond, g_log.c_str()); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

using zafx::DevBuf;
using zafx::PinnedBuf;

struct Five {
    DevBuf<float> a, b;
    DevBuf<int> c;
    DevBuf<void> d;
    PinnedBuf e;
};

// reserve / reset / move / destruction, the same for both owners
template <class B>
static int grow_only(long long& live, char alloc, char release) {
    const std::string al(1, alloc), fr(1, release);
    {
        B b;
        CHECK(b.get() == nullptr && b.bytes() == 0);
        g_log.clear();
        CHECK(b.reserve(0) == hipSuccess && b.get() == nullptr && g_log.empty());
        CHECK(b.reserve(100) == hipSuccess && b.get() && b.bytes() == 100 && live == 1);
        void* const first = b.get();
        CHECK(b.reserve(40) == hipSuccess && b.get() == first && b.bytes() == 100);    // never shrinks, keeps the pointer
        CHECK(b.reserve(100) == hipSuccess && b.get() == first && g_log == al);
        CHECK(b.reserve(101) == hipSuccess && b.bytes() == 101 && live == 1 && g_log == al + fr + al);   // the old block goes first
        g_fail_next = true;
        CHECK(b.reserve(500) == hipErrorOutOfMemory && b.get() == nullptr && b.bytes() == 0 && live == 0);
        CHECK(b.reserve(8) == hipSuccess && live == 1);
        g_log.clear();
        B moved(std::move(b));
        CHECK(b.get() == nullptr && b.bytes() == 0 && moved.bytes() == 8 && live == 1);
        b = std::move(moved);
        CHECK(moved.get() == nullptr && b.bytes() == 8 && live == 1 && g_log.empty());
        {
            B gone(std::move(moved));   // a moved-from buffer, moved again and destroyed: frees nothing
        }
        CHECK(live == 1 && g_log.empty());
        {
            B view;
            view.borrow(b);
            CHECK(view.get() == b.get() && view.bytes() == 8);
        }
        CHECK(live == 1 && g_log.empty());   // a view frees nothing
        CHECK(b.reset() == hipSuccess && b.get() == nullptr && b.bytes() == 0 && live == 0 && g_log == fr);
        CHECK(b.reset() == hipSuccess && g_log == fr);
        CHECK(b.reserve(16) == hipSuccess);
    }
    CHECK(live == 0);   // the destructor frees
    return 0;
}

int main() {
    const float one[4] = {1.f, 2.f, 3.f, 4.f}, two[2] = {5.f, 6.f};
    {
        DevBuf<float> b;
        CHECK(b.upload(one, sizeof(one)) == hipSuccess && g_log == "ac" && g_live == 1 && b.bytes() == sizeof(one));
        CHECK(std::memcmp(b.get(), one, sizeof(one)) == 0);
        const float* as_argument = b;   // the implicit conversion a kernel launch relies on
        CHECK(as_argument == b.get());
        g_log.clear();
        CHECK(b.upload(two, sizeof(two)) == hipSuccess && g_log == "fac");   // the first block is freed BEFORE the second allocation
        CHECK(g_live == 1 && b.bytes() == sizeof(two) && std::memcmp(b.get(), two, sizeof(two)) == 0);
        g_log.clear();
        CHECK(b.upload(two, sizeof(two)) == hipSuccess && g_log == "fac");   // also at the same size: upload always replaces
        g_log.clear();
        CHECK(b.upload(one, 0) == hipSuccess && b.get() == nullptr && b.bytes() == 0 && g_live == 0 && g_log == "f");
        CHECK(b.upload(nullptr, 0) == hipSuccess && b.get() == nullptr && g_live == 0 && g_log == "f");   // zero bytes on a null buffer: nothing
        CHECK(b.upload(one, sizeof(one)) == hipSuccess && g_live == 1);
        g_log.clear();
        g_fail_next = true;
        CHECK(b.upload(two, sizeof(two)) == hipErrorOutOfMemory);
        CHECK(b.get() == nullptr && b.bytes() == 0 && g_live == 0 && g_log == "f");   // the old block is gone, nothing was copied
        CHECK(b.upload(one, sizeof(one)) == hipSuccess && g_live == 1);
    }
    CHECK(g_live == 0);
    if (int rc = grow_only<DevBuf<unsigned char>>(g_live, 'a', 'f')) return rc;
    if (int rc = grow_only<DevBuf<void>>(g_live, 'a', 'f')) return rc;
    if (int rc = grow_only<PinnedBuf>(g_pinned_live, 'A', 'F')) return rc;
    {
        Five s;
        CHECK(s.a.upload(one, sizeof(one)) == hipSuccess && s.b.upload(two, sizeof(two)) == hipSuccess && s.c.reserve(64) == hipSuccess);
        CHECK(s.d.reserve(1) == hipSuccess && s.e.reserve(256) == hipSuccess);
        CHECK(g_live == 4 && g_pinned_live == 1);
        Five t(std::move(s));   // the struct moves as a whole; the source then holds nothing
        CHECK(s.a.get() == nullptr && s.e.get() == nullptr && t.c.bytes() == 64 && g_live == 4 && g_pinned_live == 1);
    }
    CHECK(g_live == 0 && g_pinned_live == 0);
    std::printf("ok\n");
    return 0;
}
