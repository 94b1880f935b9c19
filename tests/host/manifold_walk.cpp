// manifold_walk.cpp -- the host half of ddk_knn_radii / ddk_manifold_members (csrc/manifold.hip) under ASan + UBSan on a machine
// without a GPU (`make manifold_walk_asan`, csrc/host_sanitize.h; run by tests/test_sample_metrics_host.py).  Nothing runs on a device:
// every launch's geometry and pointer arguments are checked against arenas of exactly the sizes the library's own size queries
// returned, base + extent of every tensor included, and every argument error must come back before the first launch.
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>

#include "ddk.h"

extern "C" void ddk_san_register(const void* base, size_t bytes, const char* name);
extern "C" void ddk_san_unregister(const void* base);
extern "C" void ddk_san_clear(void);
extern "C" void ddk_san_stats(long* launches, long* errors);
extern "C" const char* ddk_san_first_error(void);

struct Arena {
    void* p = nullptr;
    size_t bytes = 0;
    Arena(size_t n, const char* name) : bytes(n ? n : 16) {
        p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { std::perror("mmap"); std::exit(2); }
        ddk_san_register(p, bytes, name);
    }
    ~Arena() { ddk_san_unregister(p); munmap(p, bytes); }
    float* f() const { return static_cast<float*>(p); }
    uint8_t* b() const { return static_cast<uint8_t*>(p); }
};

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

static long launches_now() {
    long l, e;
    ddk_san_stats(&l, &e);
    return l;
}

static void radii(int N, int D, int k) {
    const size_t wb = ddk_knn_radii_workspace_bytes(N);
    CHECK(wb >= (size_t)N * 9 * 4 && wb % ((size_t)N * 4) == 0, "radii N=%d: workspace %zu", N, wb);
    Arena x((size_t)N * D * 4, "x"), r((size_t)N * 4, "radii"), ws(wb, "workspace");
    long l0 = launches_now();
    CHECK(ddk_knn_radii(x.f(), N, D, k, r.f(), ws.p, wb, nullptr) == DDK_OK, "radii N=%d D=%d k=%d: %s", N, D, k, ddk_last_error());
    CHECK(launches_now() - l0 == 3, "radii N=%d: %ld launches", N, launches_now() - l0);
    // every argument error comes back before any launch
    l0 = launches_now();
    CHECK(ddk_knn_radii(x.f(), N, D, k, r.f(), ws.p, wb - 1, nullptr) == DDK_ERR_ARG, "radii N=%d: short workspace accepted", N);
    CHECK(ddk_knn_radii(x.f(), N, D, 0, r.f(), ws.p, wb, nullptr) == DDK_ERR_ARG, "k = 0 accepted");
    CHECK(ddk_knn_radii(x.f(), N, D, 8, r.f(), ws.p, wb, nullptr) == DDK_ERR_ARG, "k = 8 accepted");
    CHECK(ddk_knn_radii(x.f(), k, D, k, r.f(), ws.p, wb, nullptr) == DDK_ERR_ARG, "N = k accepted");
    CHECK(ddk_knn_radii(x.f(), N, D + 2, k, r.f(), ws.p, wb, nullptr) == DDK_ERR_ARG, "D %% 4 != 0 accepted");
    CHECK(ddk_knn_radii(x.f() + 1, N, D, k, r.f(), ws.p, wb, nullptr) == DDK_ERR_ARG, "misaligned x accepted");
    CHECK(ddk_knn_radii(nullptr, N, D, k, r.f(), ws.p, wb, nullptr) == DDK_ERR_ARG, "null x accepted");
    CHECK(ddk_knn_radii(x.f(), N, D, k, r.f(), nullptr, wb, nullptr) == DDK_ERR_ARG, "null workspace accepted");
    CHECK(launches_now() == l0, "radii N=%d: %ld launches after a rejected call", N, launches_now() - l0);
}

static void members(int Na, int Nb, int D, bool with_ra, bool with_rb) {
    const size_t wb = ddk_manifold_members_workspace_bytes(Na, Nb);
    CHECK(wb == ((size_t)Na + Nb) * 4, "members %d x %d: workspace %zu", Na, Nb, wb);
    Arena a((size_t)Na * D * 4, "a"), b((size_t)Nb * D * 4, "b"), ra((size_t)Na * 4, "ra"), rb((size_t)Nb * 4, "rb"), ain(Na, "a_in"),
        bin(Nb, "b_in"), ws(wb, "workspace");
    const float* pra = with_ra ? ra.f() : nullptr;
    const float* prb = with_rb ? rb.f() : nullptr;
    long l0 = launches_now();
    CHECK(ddk_manifold_members(a.f(), pra, Na, b.f(), prb, Nb, D, with_rb ? ain.b() : nullptr, with_ra ? bin.b() : nullptr, ws.p, wb, nullptr) ==
              DDK_OK, "members %d x %d x %d: %s", Na, Nb, D, ddk_last_error());
    CHECK(launches_now() - l0 == 3, "members: %ld launches", launches_now() - l0);
    l0 = launches_now();
    CHECK(ddk_manifold_members(a.f(), pra, Na, b.f(), prb, Nb, D, ain.b(), bin.b(), ws.p, wb - 1, nullptr) == DDK_ERR_ARG, "short workspace accepted");
    CHECK(ddk_manifold_members(a.f(), nullptr, Na, b.f(), nullptr, Nb, D, ain.b(), bin.b(), ws.p, wb, nullptr) == DDK_ERR_ARG, "no radii accepted");
    CHECK(ddk_manifold_members(a.f(), ra.f(), Na, b.f(), rb.f(), Nb, D, nullptr, bin.b(), ws.p, wb, nullptr) == DDK_ERR_ARG, "rb without a_in accepted");
    CHECK(ddk_manifold_members(a.f(), ra.f(), Na, b.f(), rb.f(), Nb, D, ain.b(), nullptr, ws.p, wb, nullptr) == DDK_ERR_ARG, "ra without b_in accepted");
    CHECK(ddk_manifold_members(a.f(), ra.f(), 0, b.f(), rb.f(), Nb, D, ain.b(), bin.b(), ws.p, wb, nullptr) == DDK_ERR_ARG, "Na = 0 accepted");
    CHECK(ddk_manifold_members(a.f(), ra.f(), Na, b.f(), rb.f(), Nb, D + 1, ain.b(), bin.b(), ws.p, wb, nullptr) == DDK_ERR_ARG, "odd D accepted");
    CHECK(launches_now() == l0, "members: %ld launches after a rejected call", launches_now() - l0);
}

int main() {
    ddk_san_clear();
    // less than a tile, ragged tiles, one and several column ranges, several tiles per range, the sizes of a real evaluation
    const int ns[] = {4, 5, 128, 137, 257, 1100, 10000, 50000};
    for (int n : ns) {
        radii(n, n >= 10000 ? 2048 : 64, 3);
        members(n, n / 2 + 3, n >= 10000 ? 2048 : 64, true, true);
        members(n / 2 + 3, n, 64, true, false);
        members(n, n, 4, false, true);
    }
    radii(8, 4, 7);
    radii(2, 2024, 1);
    CHECK(ddk_knn_radii_workspace_bytes(0) == 0 && ddk_manifold_members_workspace_bytes(0, 5) == 0, "size queries of empty sets");
    long launches, errors;
    ddk_san_stats(&launches, &errors);
    std::printf("manifold walk: %ld launches, %ld pointer/geometry errors, %d failed expectations%s%s\n", launches, errors, failures,
                errors ? "; first: " : "", errors ? ddk_san_first_error() : "");
    return (errors || failures) ? 1 : 0;
}
