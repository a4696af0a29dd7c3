// Host check of csrc/sm_devmem.h (tests/test_devmem_cpu.py builds it with the address and undefined-behaviour sanitizers):
// grow() over a three-buffer group and a DevList of five buffers, with the raw device operations replaced by host ones that
// count live allocations, log every free and can fail the k-th allocation.  Freed blocks go back to the heap only between
// scenarios, so inside one scenario an address names one allocation and a second free of it shows in the log.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

static std::set<void *> g_live;
static std::vector<void *> g_freed;
static long g_mallocs = 0, g_fail_at = 0, g_raw_calls = 0, g_bad_frees = 0;

#define SM_DEVMEM_STUB
namespace {
hipError_t dm_malloc(void **p, size_t bytes) {
    ++g_raw_calls;
    if (++g_mallocs == g_fail_at) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xCD, bytes);             // device memory is not zero unless asked for
    g_live.insert(*p);
    return hipSuccess;
}
hipError_t dm_free(void *p) {
    ++g_raw_calls;
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) ++g_bad_frees;      // never allocated, or freed before
    g_freed.push_back(p);
    return hipSuccess;
}
hipError_t dm_zero(void *p, size_t bytes) { ++g_raw_calls; std::memset(p, 0, bytes); return hipSuccess; }
hipError_t dm_sync() { ++g_raw_calls; return hipSuccess; }
}  // namespace
#include "../shapemol_amd/csrc/sm_devmem.h"

static long g_checks = 0;
#define CHECK(cond)                                                                               \
    do {                                                                                          \
        ++g_checks;                                                                               \
        if (!(cond)) { std::printf("FAILED %s:%d (%s, k = %ld): %s\n", __FILE__, __LINE__, g_what, g_k, #cond); std::exit(1); } \
    } while (0)
static const char *g_what = "";
static long g_k = 0;

static void new_scenario(long fail_at) {
    for (void *p : g_freed) std::free(p);
    g_freed.clear();
    g_mallocs = 0; g_fail_at = fail_at;
}
static long times_freed(void *p) { return (long)std::count(g_freed.begin(), g_freed.end(), p); }
static bool freed_at_most_once() {
    std::vector<void *> f = g_freed;
    std::sort(f.begin(), f.end());
    return std::adjacent_find(f.begin(), f.end()) == f.end() && g_bad_frees == 0;
}

// A group of buffers with one capacity, grown either by grow() (three buffers) or by hand on a DevList (five, padded)
struct Group {
    virtual ~Group() {}
    virtual int n() const = 0;
    virtual hipError_t to(int64_t need) = 0;           // the growth protocol
    virtual void release() = 0;
    virtual void **slot(int i) = 0;
    virtual size_t bytes(int i, int64_t need) const = 0;      // usable bytes, padding included
    virtual bool zero(int i) const = 0;
    int64_t cap = 0;
};

struct GrowGroup : Group {
    DevList mem;
    float *a = nullptr; int *b = nullptr; double *c = nullptr;
    int n() const override { return 3; }
    hipError_t to(int64_t need) override {
        return grow(mem, {dev_buf(&a, (size_t)need * 4), dev_buf(&b, (size_t)need * 3 * 4, true), dev_buf(&c, (size_t)need * 8)}, cap, need);
    }
    void release() override { mem.release(); cap = 0; }
    void **slot(int i) override { return i == 0 ? (void **)&a : i == 1 ? (void **)&b : (void **)&c; }
    size_t bytes(int i, int64_t need) const override { return (size_t)need * (i == 0 ? 4 : i == 1 ? 12 : 8); }
    bool zero(int i) const override { return i == 1; }
};

struct ListGroup : Group {
    DevList mem{256};
    char *p[5] = {};
    int n() const override { return 5; }
    hipError_t to(int64_t need) override {              // as a workspace is rebuilt: released first, capacity set last
        if (need <= cap) return hipSuccess;
        mem.release(); cap = 0;
        for (int i = 0; i < 5; ++i) {
            const hipError_t e = mem.alloc(&p[i], (size_t)need * (i + 1), zero(i));
            if (e != hipSuccess) return e;
        }
        cap = need;
        return hipSuccess;
    }
    void release() override { mem.release(); cap = 0; }
    void **slot(int i) override { return (void **)&p[i]; }
    size_t bytes(int i, int64_t need) const override { return (size_t)need * (i + 1) + 256; }
    bool zero(int i) const override { return i != 2; }
};

static void expect_empty(Group &g) {
    CHECK(g.cap == 0);
    for (int i = 0; i < g.n(); ++i) CHECK(*g.slot(i) == nullptr);
    CHECK(g_live.empty());
    CHECK(freed_at_most_once());
}

// step 3: grows without a failure, buffers distinct, zero where asked, writable over their full size; then steps 4 and 5
static void expect_grows_and_releases(Group &g, int64_t need) {
    g_fail_at = 0;
    CHECK(g.to(need) == hipSuccess);
    CHECK(g.cap == need);
    CHECK((long)g_live.size() == g.n());
    std::vector<void *> ptrs;
    for (int i = 0; i < g.n(); ++i) {
        unsigned char *q = static_cast<unsigned char *>(*g.slot(i));
        CHECK(q != nullptr && g_live.count(q) == 1);
        CHECK(std::find(ptrs.begin(), ptrs.end(), (void *)q) == ptrs.end());
        ptrs.push_back(q);
        const size_t nb = g.bytes(i, need);
        if (g.zero(i)) CHECK(std::all_of(q, q + nb, [](unsigned char v) { return v == 0; }));
        else CHECK(q[0] == 0xCD && q[nb - 1] == 0xCD);
        std::memset(q, 0xAB, nb);
    }
    // 4. nothing to grow: no raw call at all (no synchronise either), pointers unchanged
    const long calls = g_raw_calls;
    CHECK(g.to(need) == hipSuccess && g.to(need - 1) == hipSuccess);
    CHECK(g_raw_calls == calls && g.cap == need);
    for (int i = 0; i < g.n(); ++i) CHECK(*g.slot(i) == ptrs[i]);
    // 5. release, twice
    g.release();
    expect_empty(g);
    for (void *q : ptrs) CHECK(times_freed(q) == 1);
    g.release();
    expect_empty(g);
}

template <typename G>
static void run(const char *what) {
    g_what = what;
    const int64_t need = 37;
    const int n = G().n();
    for (g_k = 1; g_k <= n; ++g_k) {
        {   // 1. from empty, the k-th allocation fails
            G g;
            new_scenario(g_k);
            CHECK(g.to(need) != hipSuccess);
            expect_empty(g);
            expect_grows_and_releases(g, need);
        }
        {   // 2. from `need` to 2 * need, the k-th allocation of the growth fails: the old buffers are freed exactly once
            G g;
            new_scenario(0);
            CHECK(g.to(need) == hipSuccess && g.cap == need);
            std::vector<void *> old;
            for (int i = 0; i < n; ++i) old.push_back(*g.slot(i));
            g_fail_at = g_mallocs + g_k;
            CHECK(g.to(2 * need) != hipSuccess);
            expect_empty(g);
            for (void *q : old) CHECK(times_freed(q) == 1);
            expect_grows_and_releases(g, need);
        }
    }
    {   // a list that goes out of scope releases what it owns
        new_scenario(0);
        { G g; CHECK(g.to(need) == hipSuccess); }
        CHECK(g_live.empty() && freed_at_most_once());
    }
    new_scenario(0);
}

int main() {
    run<GrowGroup>("grow over three buffers");
    run<ListGroup>("DevList of five buffers");
    std::printf("ok %ld checks\n", g_checks);
    return 0;
}
