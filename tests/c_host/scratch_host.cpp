// ns3d_scratch (navierstokes3d_amd/csrc/ns3d_scratch.h) on the host, without a HIP runtime: this file supplies hipMalloc, hipFree,
// hipGetLastError, hipGetErrorString and ns3d_fail itself — malloc and free behind counters and one log of events — and is built
// with -fsanitize=address,undefined (tests/test_scratch_host.py), so a double free, a leak or a use after free ends the run.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ns3d_scratch.h"

static int n_malloc = 0, n_free = 0, n_fail = 0, n_drain = 0;
static bool fail_next_malloc = false;
static std::string events;             // 'm' hipMalloc, 'f' hipFree, 'd' drain: the order they came in

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes)
{
    events += 'm';
    if (fail_next_malloc) {
        fail_next_malloc = false;
        *p = (void *)0x1;               // the owner must not keep whatever a failed call left here
        return hipErrorOutOfMemory;
    }
    ++n_malloc;
    *p = std::malloc(bytes ? bytes : 1);
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    events += 'f';
    ++n_free;
    std::free(p);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
}
int ns3d_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    char msg[256];
    std::vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    ++n_fail;
    return code;
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed (events \"%s\")\n", __FILE__, __LINE__, #cond, events.c_str()); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

static_assert(!std::is_copy_constructible<ns3d_scratch>::value && !std::is_copy_assignable<ns3d_scratch>::value, "ns3d_scratch copies");

struct Rank { int id = 0; ns3d_scratch a, b[2]; };     // an owner as std::vector<MRank> holds them

int main()
{
    auto drain_ok = [] { events += 'd'; ++n_drain; return 0; };
    auto drain_refuses = [] { events += 'd'; ++n_drain; return 7; };
    {
        ns3d_scratch s;
        CHECK(s.ptr == nullptr && s.bytes == 0);
        // the first reserve allocates and does not drain
        CHECK(s.reserve(100, drain_ok) == 0);
        CHECK(events == "m" && s.ptr && s.bytes == 100 && n_drain == 0);
        ((char *)s.ptr)[99] = 1;
        // enough room: no call at all
        void *p0 = s.ptr;
        CHECK(s.reserve(100, drain_ok) == 0 && s.reserve(1, drain_ok) == 0 && s.reserve(0, drain_ok) == 0);
        CHECK(events == "m" && s.ptr == p0 && s.bytes == 100);
        // growth: the drain exactly once, before the free, the allocation last
        CHECK(s.reserve(101, drain_ok) == 0);
        CHECK(events == "mdfm" && n_drain == 1 && s.bytes == 101 && s.as<char>() == (char *)s.ptr);
        ((char *)s.ptr)[100] = 1;
        // a drain that refuses: its value comes back, buffer and size stay, nothing is freed or allocated
        void *p1 = s.ptr;
        CHECK(s.reserve(500, drain_refuses) == 7);
        CHECK(events == "mdfmd" && s.ptr == p1 && s.bytes == 101 && n_fail == 0);
        // a failing allocation (the old buffer has gone by then) leaves {nullptr, 0}; a later reserve succeeds without a drain
        fail_next_malloc = true;
        CHECK(s.reserve(500, drain_ok) == NS3D_ERR_HIP);
        CHECK(events == "mdfmddfm" && s.ptr == nullptr && s.bytes == 0 && n_fail == 1);
        CHECK(s.reserve(500, drain_ok) == 0);
        CHECK(events == "mdfmddfmm" && s.ptr && s.bytes == 500 && n_drain == 3);
        // … and on an empty owner likewise
        ns3d_scratch t;
        fail_next_malloc = true;
        CHECK(t.reserve(8, drain_ok) == NS3D_ERR_HIP && t.ptr == nullptr && t.bytes == 0 && n_fail == 2);
        CHECK(t.reserve(8, drain_ok) == 0 && t.bytes == 8);
        // release twice frees once; what the destructor then finds is empty
        const int f0 = n_free;
        s.release();
        s.release();
        CHECK(n_free == f0 + 1 && s.ptr == nullptr && s.bytes == 0);
        // a move leaves the source empty
        ns3d_scratch u(std::move(t));
        CHECK(t.ptr == nullptr && t.bytes == 0 && u.ptr && u.bytes == 8);
    }
    CHECK(n_malloc == n_free);          // s was released by hand, u by its destructor
    {
        // a vector of owners grows (its elements move) and is destroyed: every buffer is freed once — ASan is the judge
        std::vector<Rank> ranks;
        for (int i = 0; i < 37; ++i) {
            ranks.emplace_back();
            ranks.back().id = i;
            CHECK(ranks.back().a.reserve(16 + i, drain_ok) == 0);
            if (i % 3 == 0) CHECK(ranks.back().b[1].reserve(8, drain_ok) == 0);
        }
        ranks.resize(64);
        for (int i = 0; i < 37; ++i) {
            CHECK(ranks[i].id == i && ranks[i].a.bytes == (size_t)(16 + i));
            ((char *)ranks[i].a.ptr)[15 + i] = 1;
        }
        Rank gone(std::move(ranks[5]));     // how ns3d_mgpu_destroy ends a rank: the buffers go with `gone`, the element stays empty
        CHECK(ranks[5].a.ptr == nullptr && gone.a.bytes == 21);
    }
    CHECK(n_malloc == n_free);
    std::printf("scratch OK: %d allocations, %d frees, %d drains\n", n_malloc, n_free, n_drain);
    return 0;
}
