// data_walk.cpp -- the host half of the image-batch entry (csrc/image_batch.hip) under ASan + UBSan on a machine without a GPU
// (`make data_walk_asan`, csrc/host_sanitize.h; run by tests/test_native_data_host.py).  Nothing runs on a device: for every shape of the
// test list the band query and the entry are called with arenas of exactly the tensors' sizes, the launch's geometry and pointers are
// checked, and every argument error must come back before a launch.
#include <sys/mman.h>

#include <algorithm>
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
    int32_t* i() const { return static_cast<int32_t*>(p); }
    int64_t* l() const { return static_cast<int64_t*>(p); }
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

// the longest row of taps with a weight above zero among rows off .. off+S-1 of the antialiased bilinear resize n_in -> n_out
static int taps_of(int n_in, int n_out, int off, int S) {
    const double scale = (double)n_in / n_out, support = std::max(scale, 1.0), inv = std::min(1.0 / scale, 1.0);
    int taps = 0;
    for (int i = off; i < off + S; ++i) {
        const double c = scale * (i + 0.5);
        const int lo = std::max((int)(c - support + 0.5), 0), hi = std::min((int)(c + support + 0.5), n_in);
        int first = hi, last = lo - 1;
        for (int j = lo; j < hi; ++j)
            if (1.0 - std::fabs((j - c + 0.5) * inv) > 0.0) { first = std::min(first, j); last = j; }
        taps = std::max(taps, last - first + 1);
    }
    return taps;
}

static void shape(int Hs, int Ws, int S, int C, int B, int want_row_taps, int want_col_taps) {
    const int Ho = Hs <= Ws ? S : (int)((double)S * Hs / Ws), Wo = Hs <= Ws ? (int)((double)S * Ws / Hs) : S;
    const int top = (int)std::nearbyint((Ho - S) / 2.0), left = (int)std::nearbyint((Wo - S) / 2.0);      // half to even, as Python's round
    const int rt = taps_of(Hs, Ho, top, S), ct = taps_of(Ws, Wo, left, S);
    CHECK(rt == want_row_taps && ct == want_col_taps, "%dx%d -> %d: taps %d, %d", Hs, Ws, S, rt, ct);
    const long long N = 6;
    Arena images((size_t)N * Hs * Ws * C, "images"), index((size_t)B * 8, "index"), rs((size_t)S * 4, "row_start"), rw((size_t)S * rt * 4, "row_w"),
        cs((size_t)S * 4, "col_start"), cw((size_t)S * ct * 4, "col_w"), out((size_t)B * C * S * S * 4, "out");
    const int r = ddk_image_batch_rows_per_group(Hs, Ws, C, S, rt, ct);
    CHECK(r >= 1 && r <= S, "%dx%dx%d -> %d: rows per group %d", Hs, Ws, C, S, r);
    long l0 = launches_now();
    CHECK(ddk_image_batch(images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 1, 7, 0, out.f(), nullptr) == DDK_OK,
          "%dx%dx%d -> %d: %s", Hs, Ws, C, S, ddk_last_error());
    CHECK(launches_now() - l0 == 1, "%dx%dx%d -> %d: %ld launches", Hs, Ws, C, S, launches_now() - l0);
    // every argument error comes back before any launch
    l0 = launches_now();
#define REJECT(what, ...) CHECK(ddk_image_batch(__VA_ARGS__) == DDK_ERR_ARG, "%dx%dx%d -> %d: %s accepted", Hs, Ws, C, S, what)
    REJECT("null images", nullptr, N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("null index", images.b(), N, Hs, Ws, C, nullptr, B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("null row_start", images.b(), N, Hs, Ws, C, index.l(), B, nullptr, rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("null row_w", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), nullptr, rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("null col_start", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, nullptr, cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("null col_w", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), nullptr, ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("null out", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, nullptr, nullptr);
    REJECT("C = 0", images.b(), N, Hs, Ws, 0, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("C = 5", images.b(), N, Hs, Ws, 5, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("S no multiple of 4", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S + 2, 0, 7, 0, out.f(), nullptr);
    REJECT("S = 0", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, 0, 0, 7, 0, out.f(), nullptr);
    REJECT("S = 1028", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, 1028, 0, 7, 0, out.f(), nullptr);
    REJECT("row_taps = 0", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), 0, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("row_taps = 33", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), 33, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("col_taps = 0", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), 0, S, 0, 7, 0, out.f(), nullptr);
    REJECT("col_taps = 33", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), 33, S, 0, 7, 0, out.f(), nullptr);
    REJECT("more taps than source rows", images.b(), N, rt - 1, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("B = 0", images.b(), N, Hs, Ws, C, index.l(), 0, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("n_images = 0", images.b(), 0, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f(), nullptr);
    REJECT("misaligned out", images.b(), N, Hs, Ws, C, index.l(), B, rs.i(), rw.f(), rt, cs.i(), cw.f(), ct, S, 0, 7, 0, out.f() + 1, nullptr);
#undef REJECT
    CHECK(launches_now() == l0, "%dx%dx%d -> %d: %ld launches after rejected calls", Hs, Ws, C, S, launches_now() - l0);
    std::printf("%4d x %4d x %d -> %4d  taps %2d, %2d  %3d rows per group, %3d bands\n", Hs, Ws, C, S, rt, ct, r, (S + r - 1) / r);
}

int main() {
    ddk_san_clear();
    // (Hs, Ws, S) of tests/image_batch_ref.py SHAPES with the taps utils/image_batch.py finds for them, each with C = 1 and C = 3, B = 5
    static const int shapes[][5] = {{218, 178, 64, 6, 6}, {21, 13, 8, 4, 4}, {13, 21, 8, 4, 4}, {9, 9, 16, 2, 2}, {40, 24, 32, 2, 2},
                                    {16, 16, 16, 1, 1},   {33, 47, 16, 5, 5}, {12, 20, 24, 2, 2}, {64, 64, 16, 8, 8}, {7, 5, 4, 3, 2}};
    for (const auto& s : shapes)
        for (int C : {1, 3}) shape(s[0], s[1], s[2], C, 5, s[3], s[4]);
    // the larger shapes the kernel must take: S = 256 from 256 and from 1024 (four times the side), S = 32 unchanged, a partial last band
    shape(256, 256, 256, 3, 16, 1, 1);
    shape(1024, 1024, 256, 3, 16, 8, 8);
    shape(32, 32, 32, 3, 128, 1, 1);
    shape(128, 128, 32, 1, 2, 8, 8);
    shape(512, 512, 128, 3, 2, 8, 8);
    // a shape whose single output row does not fit the LDS budget: the query says 0 and the entry refuses it before a launch
    {
        Arena images(16, "images"), index(8, "index"), t(1024 * 8 * 4, "tables"), out(16, "out");
        const long l0 = launches_now();
        CHECK(ddk_image_batch_rows_per_group(4096, 4096, 4, 1024, 8, 8) == 0, "4096^2 x 4 -> 1024 taken");
        CHECK(ddk_image_batch(images.b(), 1, 4096, 4096, 4, index.l(), 1, t.i(), t.f(), 8, t.i(), t.f(), 8, 1024, 0, 7, 0, out.f(), nullptr) == DDK_ERR_ARG,
              "4096^2 x 4 -> 1024 accepted");
        CHECK(ddk_image_batch_rows_per_group(218, 178, 0, 64, 7, 7) == 0 && ddk_image_batch_rows_per_group(218, 178, 3, 62, 7, 7) == 0 &&
                  ddk_image_batch_rows_per_group(218, 178, 3, 64, 33, 7) == 0, "the query takes a bad shape");
        CHECK(launches_now() == l0, "%ld launches after rejected calls", launches_now() - l0);
    }
    long launches, errors;
    ddk_san_stats(&launches, &errors);
    std::printf("data walk: %ld launches, %ld pointer/geometry errors, %d failed expectations%s%s\n", launches, errors, failures,
                errors ? "; first: " : "", errors ? ddk_san_first_error() : "");
    return (errors || failures) ? 1 : 0;
}
