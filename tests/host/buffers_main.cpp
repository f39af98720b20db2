/* Walks the owning buffer types of rgbd_odometry_amd/csrc/dvo_buffers.h over counting fakes of the four HIP allocation calls (plain
 * malloc underneath, the n-th allocation can be told to fail).  Stand-alone: built with the address and undefined-behaviour
 * sanitizers by tests/test_buffers_cpu.py, linked without the HIP runtime. */
#include "dvo_buffers.h"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {
std::set<void *> g_live_dev, g_live_host;
int g_allocs = 0, g_frees = 0, g_peak = 0, g_fail_at = 0;      /* g_fail_at: the n-th allocation from now fails (0: none) */

int live() { return (int)(g_live_dev.size() + g_live_host.size()); }
hipError_t fake_alloc(std::set<void *> &pool, void **p, size_t bytes) {
    *p = nullptr;
    if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    pool.insert(*p);
    g_allocs++;
    if (live() > g_peak) g_peak = live();
    return hipSuccess;
}
hipError_t fake_free(std::set<void *> &pool, void *p) {
    if (!p) return hipSuccess;
    if (!pool.erase(p)) { std::fprintf(stderr, "free of a block that is not live (double free, or the wrong kind)\n"); std::abort(); }
    std::free(p);
    g_frees++;
    return hipSuccess;
}
void start() { g_allocs = g_frees = g_peak = g_fail_at = 0; }

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(g_live_dev, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(g_live_dev, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) {
    CHECK(flags == hipHostMallocDefault);
    return fake_alloc(g_live_host, p, bytes);
}
hipError_t hipHostFree(void *p) { return fake_free(g_live_host, p); }
}

using dvo_host::DevBuf;
using dvo_host::PinnedBuf;

template <template <class> class Buf>
void walk() {
    {   /* an empty buffer frees nothing */
        start();
        { Buf<float> b; CHECK(b.get() == nullptr && b.size() == 0 && !b); b.reset(); }
        CHECK(g_allocs == 0 && g_frees == 0);
    }
    {   /* alloc, destroy */
        start();
        {
            Buf<double> b;
            CHECK(b.alloc(7) == hipSuccess && b.get() && b.size() == 7 && live() == 1);
            double *raw = b;                       /* the implicit conversion, indexing and pointer arithmetic through it */
            raw[6] = 1.0;
            CHECK(b[6] == 1.0 && b + 6 == raw + 6);
        }
        CHECK(live() == 0 && g_allocs == 1 && g_frees == 1);
    }
    {   /* move construction leaves the source empty */
        start();
        {
            Buf<int> a;
            CHECK(a.alloc(3) == hipSuccess);
            int *raw = a.get();
            Buf<int> b(std::move(a));
            CHECK(a.get() == nullptr && a.size() == 0 && b.get() == raw && b.size() == 3 && live() == 1 && g_frees == 0);
        }
        CHECK(live() == 0 && g_frees == 1);
    }
    {   /* move assignment frees the destination's old block exactly once; self-move-assignment is harmless */
        start();
        {
            Buf<int> a, b;
            CHECK(a.alloc(3) == hipSuccess && b.alloc(5) == hipSuccess && live() == 2);
            int *raw = a.get();
            b = std::move(a);
            CHECK(g_frees == 1 && live() == 1 && a.get() == nullptr && a.size() == 0 && b.get() == raw && b.size() == 3);
            Buf<int> &self = b;
            b = std::move(self);
            CHECK(g_frees == 1 && live() == 1 && b.get() == raw && b.size() == 3);
            b = Buf<int>();                       /* an empty one over a full one: how a release is written */
            CHECK(g_frees == 2 && live() == 0 && b.get() == nullptr && b.size() == 0);
        }
        CHECK(live() == 0 && g_frees == 2);
    }
    {   /* a failed alloc leaves {nullptr, 0}, on an empty and on a full buffer; a later alloc works */
        start();
        Buf<float> b;
        g_fail_at = 1;
        CHECK(b.alloc(4) == hipErrorOutOfMemory && b.get() == nullptr && b.size() == 0 && live() == 0);
        CHECK(b.alloc(4) == hipSuccess && b.size() == 4 && live() == 1);
        g_fail_at = 1;
        CHECK(b.alloc(8) == hipErrorOutOfMemory && b.get() == nullptr && b.size() == 0 && live() == 0);
        CHECK(b.alloc(8) == hipSuccess && b.get() && b.size() == 8 && live() == 1);
    }
    CHECK(live() == 0);
    {   /* alloc on a full buffer frees first: never two blocks at once */
        start();
        Buf<char> b;
        CHECK(b.alloc(16) == hipSuccess && b.alloc(32) == hipSuccess && b.size() == 32);
        CHECK(g_peak == 1 && g_allocs == 2 && g_frees == 1);
    }
    CHECK(live() == 0);
}

/* ensure_points: five locals are filled, and only then move-assigned over the old five */
struct Five { DevBuf<float> pts; DevBuf<unsigned> cpts, cidx, cpt4, chdr; };
hipError_t grow_five(Five &L, size_t n) {
    Five N;
    hipError_t e;
    if ((e = N.pts.alloc(3 * n)) != hipSuccess) return e;
    if ((e = N.cpts.alloc(n)) != hipSuccess) return e;
    if ((e = N.cidx.alloc(n)) != hipSuccess) return e;
    if ((e = N.cpt4.alloc(n)) != hipSuccess) return e;
    if ((e = N.chdr.alloc(n / 64)) != hipSuccess) return e;
    L.pts = std::move(N.pts); L.cpts = std::move(N.cpts); L.cidx = std::move(N.cidx); L.cpt4 = std::move(N.cpt4); L.chdr = std::move(N.chdr);
    return hipSuccess;
}
void walk_five() {
    start();
    {
        Five L;
        CHECK(grow_five(L, 256) == hipSuccess && live() == 5);
        void *old[5] = {L.pts.get(), L.cpts.get(), L.cidx.get(), L.cpt4.get(), L.chdr.get()};
        g_fail_at = 4;
        CHECK(grow_five(L, 512) == hipErrorOutOfMemory);
        CHECK(live() == 5);                                   /* the three new blocks are gone ... */
        CHECK(L.pts.get() == old[0] && L.cpts.get() == old[1] && L.cidx.get() == old[2] && L.cpt4.get() == old[3] && L.chdr.get() == old[4]);
        CHECK(L.pts.size() == 768 && L.chdr.size() == 4);     /* ... and the old five untouched */
        CHECK(grow_five(L, 512) == hipSuccess && live() == 5 && L.pts.size() == 1536 && L.pts.get() != nullptr);
    }
    CHECK(live() == 0);
    start();
    {   /* the first growth: nothing to keep */
        Five L;
        g_fail_at = 4;
        CHECK(grow_five(L, 256) == hipErrorOutOfMemory && live() == 0 && !L.pts && !L.chdr);
    }
}

/* a release: a default-constructed struct of several buffers assigned over a full one */
struct Several {
    int n = 0;
    DevBuf<float> a;
    PinnedBuf<float> b;
    struct Inner { DevBuf<int> c[2]; PinnedBuf<double> d; } in;
};
void walk_release() {
    start();
    Several S;
    S.n = 5;
    CHECK(S.a.alloc(1) == hipSuccess && S.b.alloc(2) == hipSuccess && S.in.c[0].alloc(3) == hipSuccess && S.in.c[1].alloc(4) == hipSuccess &&
          S.in.d.alloc(5) == hipSuccess && live() == 5);
    S = Several();
    CHECK(live() == 0 && g_frees == 5 && S.n == 0 && !S.a && !S.b && !S.in.c[0] && !S.in.c[1] && !S.in.d && S.in.d.size() == 0);
    S = Several();
    CHECK(g_frees == 5);
}

int main() {
    walk<DevBuf>();
    walk<PinnedBuf>();
    walk_five();
    walk_release();
    CHECK(live() == 0);
    std::puts("ok");
    return 0;
}
