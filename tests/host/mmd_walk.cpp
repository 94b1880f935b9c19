// mmd_walk.cpp -- the host half of ddk_poly_mmd_sums / ddk_manifold_ball_counts (csrc/manifold.hip) under ASan + UBSan on a machine
// without a GPU (`make mmd_walk_asan`, csrc/host_sanitize.h; run by tests/test_sample_metrics_ext_host.py).  Nothing runs on a device:
// every launch's geometry and pointer arguments are checked against arenas of exactly the sizes the library's own size queries
// returned, base + extent of every tensor included, and every argument error must come back before the first launch.
#include <sys/mman.h>

#include <cmath>
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
    double* d() const { return static_cast<double*>(p); }
    int* i() const { return static_cast<int*>(p); }
};

static int failures = 0;
static int accepted = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

static long launches_now() {
    long l, e;
    ddk_san_stats(&l, &e);
    return l;
}

static size_t tiles(int ma, int mb) {
    const size_t ta = ((size_t)ma + 127) / 128, tb = ((size_t)mb + 127) / 128;
    return ta * (ta + 1) / 2 + tb * (tb + 1) / 2 + ta * tb;
}

static void mmd(int S, int ma, int mb, int D) {
    const size_t wb = ddk_poly_mmd_workspace_bytes(S, ma, mb);
    CHECK(wb == (size_t)S * tiles(ma, mb) * 8, "mmd %d x (%d, %d): workspace %zu", S, ma, mb, wb);
    Arena a((size_t)S * ma * D * 4, "a"), b((size_t)S * mb * D * 4, "b"), sums((size_t)S * 3 * 8, "sums"), ws(wb, "workspace");
    const float g = 1.0f / D;
    long l0 = launches_now();
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_OK, "mmd %d x (%d, %d) x %d: %s", S, ma,
          mb, D, ddk_last_error());
    CHECK(launches_now() - l0 == 2, "mmd: %ld launches", launches_now() - l0);
    ++accepted;
    // every argument error comes back before any launch
    l0 = launches_now();
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb - 1, nullptr) == DDK_ERR_ARG, "short workspace accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, g, 1.0f, sums.d(), nullptr, wb, nullptr) == DDK_ERR_ARG, "null workspace accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, g, 1.0f, sums.d(), static_cast<char*>(ws.p) + 8, wb, nullptr) == DDK_ERR_ARG,
          "misaligned workspace accepted");
    CHECK(ddk_poly_mmd_sums(nullptr, b.f(), S, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "null a accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), nullptr, S, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "null b accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, g, 1.0f, nullptr, ws.p, wb, nullptr) == DDK_ERR_ARG, "null sums accepted");
    CHECK(ddk_poly_mmd_sums(a.f() + 1, b.f(), S, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "misaligned a accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f() + 2, S, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "misaligned b accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, g, 1.0f, reinterpret_cast<double*>(sums.f() + 1), ws.p, wb, nullptr) == DDK_ERR_ARG,
          "misaligned sums accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D + 2, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "D %% 4 != 0 accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, 0, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "D = 0 accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, 1, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "ma = 1 accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, 1, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "mb = 1 accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), 0, ma, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "S = 0 accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, (1 << 24) / S + 1, mb, D, g, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG,
          "S ma > 2^24 accepted");
    CHECK(ddk_poly_mmd_sums(a.f(), b.f(), S, ma, mb, D, INFINITY, 1.0f, sums.d(), ws.p, wb, nullptr) == DDK_ERR_ARG, "gamma = inf accepted");
    CHECK(launches_now() == l0, "mmd: %ld launches after a rejected call", launches_now() - l0);
}

static void balls(int Na, int Nb, int D) {
    const size_t wb = ddk_manifold_ball_counts_workspace_bytes(Na, Nb);
    CHECK(wb == ((size_t)Na + Nb) * 4, "balls %d x %d: workspace %zu", Na, Nb, wb);
    Arena a((size_t)Na * D * 4, "a"), b((size_t)Nb * D * 4, "b"), ra((size_t)Na * 4, "ra"), counts((size_t)Na * 4, "counts"), ws(wb, "workspace");
    long l0 = launches_now();
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f(), Nb, D, counts.i(), ws.p, wb, nullptr) == DDK_OK, "balls %d x %d x %d: %s", Na, Nb, D,
          ddk_last_error());
    CHECK(launches_now() - l0 == 3, "balls: %ld launches", launches_now() - l0);
    ++accepted;
    l0 = launches_now();
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f(), Nb, D, counts.i(), ws.p, wb - 1, nullptr) == DDK_ERR_ARG, "short workspace accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f(), Nb, D, counts.i(), nullptr, wb, nullptr) == DDK_ERR_ARG, "null workspace accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), nullptr, Na, b.f(), Nb, D, counts.i(), ws.p, wb, nullptr) == DDK_ERR_ARG, "null ra accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f(), Nb, D, nullptr, ws.p, wb, nullptr) == DDK_ERR_ARG, "null counts accepted");
    CHECK(ddk_manifold_ball_counts(nullptr, ra.f(), Na, b.f(), Nb, D, counts.i(), ws.p, wb, nullptr) == DDK_ERR_ARG, "null a accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f() + 1, Nb, D, counts.i(), ws.p, wb, nullptr) == DDK_ERR_ARG, "misaligned b accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), 0, b.f(), Nb, D, counts.i(), ws.p, wb, nullptr) == DDK_ERR_ARG, "Na = 0 accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f(), 0, D, counts.i(), ws.p, wb, nullptr) == DDK_ERR_ARG, "Nb = 0 accepted");
    CHECK(ddk_manifold_ball_counts(a.f(), ra.f(), Na, b.f(), Nb, D + 1, counts.i(), ws.p, wb, nullptr) == DDK_ERR_ARG, "odd D accepted");
    CHECK(launches_now() == l0, "balls: %ld launches after a rejected call", launches_now() - l0);
}

int main() {
    ddk_san_clear();
    // the shapes of tests/test_sample_metrics_ext_gpu.py, then the sizes of a real evaluation: one segment of 10 000 and of 50 000 rows
    // a side, and the conventional hundred subsets of a thousand
    const int shapes[][4] = {{1, 2, 2, 4},         {1, 130, 90, 40},       {3, 130, 130, 32},       {1, 300, 257, 72},      {100, 8, 8, 32},
                             {1, 1000, 1000, 2048}, {1, 10000, 10000, 2048}, {1, 50000, 30000, 2048}, {100, 1000, 1000, 2048}, {1 << 16, 2, 3, 4}};
    for (const auto& s : shapes) mmd(s[0], s[1], s[2], s[3]);
    const int pairs[][3] = {{150, 90, 32}, {130, 300, 40}, {8, 1, 4}, {300, 257, 72}, {1, 1, 4}, {10000, 10000, 2048}, {50000, 30000, 2048}};
    for (const auto& p : pairs) balls(p[0], p[1], p[2]);
    CHECK(ddk_poly_mmd_workspace_bytes(0, 8, 8) == 0 && ddk_poly_mmd_workspace_bytes(1, 1, 8) == 0 && ddk_poly_mmd_workspace_bytes(1, 8, 1) == 0 &&
              ddk_poly_mmd_workspace_bytes(2, (1 << 23) + 1, 8) == 0 && ddk_manifold_ball_counts_workspace_bytes(0, 5) == 0,
          "size queries of refused shapes");
    long launches, errors;
    ddk_san_stats(&launches, &errors);
    std::printf("mmd walk: %ld launches in %d accepted calls, %ld pointer/geometry errors, %d failed expectations%s%s\n", launches, accepted, errors,
                failures, errors ? "; first: " : "", errors ? ddk_san_first_error() : "");
    return (errors || failures) ? 1 : 0;
}
