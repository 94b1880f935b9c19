// fft_noisy_walk.cpp -- the host half of the noisy deconvolution entries (csrc/fft_conv.hip, ddk_sampler_run_restore_fft_noisy in
// csrc/unet_plan.hip) under ASan + UBSan on a machine without a GPU (`make fft_noisy_walk_asan`, csrc/host_sanitize.h; run by
// tests/test_restore_fft_noisy_host.py).  Nothing runs on a device: every launch's geometry and pointer arguments are checked against
// arenas of exactly the sizes the library's own size queries returned, in the plane form and in the multi-launch form, and every
// argument error must come back before the first launch.
#include <sys/mman.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

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
    int64_t* l() const { return static_cast<int64_t*>(p); }
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
static size_t al4(size_t v) { return (v + 3) / 4 * 4; }

// the spectrum of A+ y and the lone step: one launch each in the plane form; two and three through the scratch (T, and T and T2)
static void lone(int B, int C, int H, int W) {
    const size_t N = (size_t)H * W, xb = (size_t)B * C * N * 4;
    const bool multi = N > 16384;
    Arena x(xb, "x"), eps(xb, "eps_hat"), y(xb, "y"), yhat(2 * xb, "Yhat"), mask(N * 4, "mask"), gain(N * 4, "gain"), nsc(4 * 4, "nsc"),
        mul(N * 8, "multiplier"), tw((size_t)std::max(H, W) * 4, "twiddles"), tmp(multi ? 4 * xb : 16, "scratch"), t((size_t)B * 8, "t"),
        tab(5 * 4 * 4, "tables");
    float* sc = multi ? tmp.f() : nullptr;
    const float *cr = tab.f(), *crm1 = tab.f() + 4, *c1 = tab.f() + 8, *c2 = tab.f() + 12, *sg = tab.f() + 16;
    auto step = [&](const float* m, const float* g, const float* ns, const float* twd, const float* yh, float* scratch, const float* sigma, int h) {
        return ddk_p_sample_update_restore_fft_noisy(x.f(), eps.f(), m, g, ns, twd, yh, scratch, t.l(), cr, crm1, c1, c2, sigma, B, h, W, C, 1, 0,
                                                     nullptr);
    };
    long l0 = launches_now();
    CHECK(ddk_circular_spectrum(y.f(), mul.f(), tw.f(), yhat.f(), sc, B, H, W, C, nullptr) == DDK_OK, "spectrum %dx%dx%d: %s", C, H, W, ddk_last_error());
    CHECK(launches_now() - l0 == (multi ? 2 : 1), "spectrum %dx%d: %ld launches", H, W, launches_now() - l0);
    l0 = launches_now();
    CHECK(step(mask.f(), gain.f(), nsc.f(), tw.f(), yhat.f(), sc, sg, H) == DDK_OK, "step %dx%dx%d: %s", C, H, W, ddk_last_error());
    CHECK(launches_now() - l0 == (multi ? 3 : 1), "step %dx%d: %ld launches", H, W, launches_now() - l0);
    // every argument error comes back before any launch
    l0 = launches_now();
    CHECK(ddk_circular_spectrum(y.f(), mul.f(), tw.f(), yhat.f(), sc, B, H + 8, W, C, nullptr) == DDK_ERR_ARG, "spectrum: H no power of two accepted");
    CHECK(ddk_circular_spectrum(y.f(), nullptr, tw.f(), yhat.f(), sc, B, H, W, C, nullptr) == DDK_ERR_ARG, "spectrum: null multiplier accepted");
    CHECK(ddk_circular_spectrum(y.f() + 1, mul.f(), tw.f(), yhat.f(), sc, B, H, W, C, nullptr) == DDK_ERR_ARG, "spectrum: misaligned y accepted");
    CHECK(step(mask.f(), gain.f(), nsc.f(), tw.f(), yhat.f(), sc, sg, H + 8) == DDK_ERR_ARG, "step: H no power of two accepted");
    CHECK(step(nullptr, gain.f(), nsc.f(), tw.f(), yhat.f(), sc, sg, H) == DDK_ERR_ARG, "null mask accepted");
    CHECK(step(mask.f(), nullptr, nsc.f(), tw.f(), yhat.f(), sc, sg, H) == DDK_ERR_ARG, "null gain accepted");
    CHECK(step(mask.f(), gain.f(), nullptr, tw.f(), yhat.f(), sc, sg, H) == DDK_ERR_ARG, "null nsc accepted");
    CHECK(step(mask.f(), gain.f(), nsc.f(), nullptr, yhat.f(), sc, sg, H) == DDK_ERR_ARG, "null twiddles accepted");
    CHECK(step(mask.f(), gain.f(), nsc.f(), tw.f(), nullptr, sc, sg, H) == DDK_ERR_ARG, "null Yhat accepted");
    CHECK(step(mask.f(), gain.f(), nsc.f(), tw.f(), yhat.f(), sc, nullptr, H) == DDK_ERR_ARG, "null sigma accepted");
    CHECK(step(mask.f(), gain.f() + 1, nsc.f(), tw.f(), yhat.f(), sc, sg, H) == DDK_ERR_ARG, "misaligned gain accepted");
    CHECK(step(mask.f(), gain.f(), nsc.f() + 1, tw.f(), yhat.f(), sc, sg, H) == DDK_ERR_ARG, "misaligned nsc accepted");
    CHECK(step(mask.f(), gain.f(), nsc.f(), tw.f(), yhat.f() + 1, sc, sg, H) == DDK_ERR_ARG, "misaligned Yhat accepted");
    if (multi) {
        CHECK(ddk_circular_spectrum(y.f(), mul.f(), tw.f(), yhat.f(), nullptr, B, H, W, C, nullptr) == DDK_ERR_ARG, "multi-launch spectrum without a scratch accepted");
        CHECK(step(mask.f(), gain.f(), nsc.f(), tw.f(), yhat.f(), nullptr, sg, H) == DDK_ERR_ARG, "multi-launch step without a scratch accepted");
    }
    CHECK(launches_now() == l0, "lone %dx%d: %ld launches after rejected calls", H, W, launches_now() - l0);
}

// a three-step eager chain of the new kind on a workspace of exactly the queried size
static void chain(const char* name, int in_ch, int chan, std::vector<int> mults, int B, int H, int W) {
    ddk_unet_config cfg{};
    cfg.in_ch = in_ch; cfg.chan = chan; cfg.n_levels = (int)mults.size();
    for (size_t i = 0; i < mults.size(); ++i) cfg.mults[i] = mults[i];
    ddk_unet* u = ddk_unet_create(&cfg);
    CHECK(u != nullptr, "%s: ddk_unet_create: %s", name, ddk_last_error());
    if (!u) return;
    const int T = 100;
    const size_t packed_bytes = ddk_unet_packed_bytes(u), N = (size_t)H * W, xb = (size_t)B * N * in_ch * 4;
    const size_t fft_bytes = ddk_sampler_restore_fft_workspace_bytes(u, B, H, W, 2), bytes = ddk_sampler_restore_fft_noisy_workspace_bytes(u, B, H, W, 2);
    CHECK(fft_bytes > 0 && bytes == fft_bytes + N * 4 + al4(3) * 4 + 2 * xb + (N > 16384 ? 2 * xb : 0),
          "%s: workspace query %zu against the deconvolution sampler's %zu", name, bytes, fft_bytes);
    CHECK(ddk_sampler_restore_fft_noisy_tail_parts(u, B, H, W) == 0, "%s: tail parts", name);
    CHECK(ddk_sampler_restore_fft_noisy_workspace_bytes(u, B, H + 8, W, 2) == 0, "%s: off-grid workspace query", name);
    Arena packed(packed_bytes, "packed");
    long long max_slot = 0;
    const int n_slots = ddk_unet_num_slots(u);
    for (int i = 0; i < n_slots; ++i) max_slot = std::max(max_slot, ddk_unet_slot_numel(u, i));
    Arena canonical((size_t)max_slot * 4, "canonical weight");
    for (int i = 0; i < n_slots; ++i)
        CHECK(ddk_unet_pack_slot(u, i, canonical.f(), packed.p, nullptr) == DDK_OK, "%s: pack slot %d: %s", name, i, ddk_last_error());
    CHECK(ddk_unet_finalize_pack(u, packed.p, nullptr) == DDK_OK, "%s: finalize_pack: %s", name, ddk_last_error());
    Arena x(xb, "x"), y(xb, "y"), mask(N * 4, "mask"), P(N * 8, "P"), gain(N * 4, "gain"), nsc(3 * 4, "nsc"), tw((size_t)std::max(H, W) * 4, "twiddles"),
        tables((size_t)5 * T * 4, "schedule tables"), ws(bytes, "noisy deconvolution sampler workspace");
    const int64_t map[3] = {0, T / 2, T - 1};
    ddk_sampler_args a{};
    a.unet = u; a.packed = packed.p; a.x = x.f(); a.noise = nullptr;
    a.c_recip = tables.f(); a.c_recipm1 = tables.f() + T; a.c1 = tables.f() + 2 * T; a.c2 = tables.f() + 3 * T; a.sigma = tables.f() + 4 * T;
    a.B = B; a.H = H; a.W = W; a.t_start = 2; a.t_end = 0; a.seed = 1; a.stream_id = 0; a.use_graph = 0;
    a.workspace = ws.p; a.workspace_bytes = bytes;
    auto run = [&](const float* m, const float* p, const float* g, const float* ns, const float* twd, const float* yy) {
        return ddk_sampler_run_restore_fft_noisy(&a, map, m, p, g, ns, twd, yy, nullptr);
    };
    long l0 = launches_now();
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), tw.f(), y.f()) == DDK_OK, "%s: sampler_run_restore_fft_noisy: %s", name, ddk_last_error());
    const long per_chain = launches_now() - l0;
    CHECK(per_chain > 3, "%s: %ld launches in a three-step chain", name, per_chain);
    l0 = launches_now();
    a.workspace_bytes = bytes - 4;
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), tw.f(), y.f()) == DDK_ERR_WORKSPACE, "%s: short workspace accepted", name);
    a.workspace_bytes = fft_bytes;      // the deconvolution sampler's size is not enough either
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), tw.f(), y.f()) == DDK_ERR_WORKSPACE, "%s: the deconvolution sampler's workspace accepted", name);
    a.workspace_bytes = bytes;
    CHECK(run(nullptr, P.f(), gain.f(), nsc.f(), tw.f(), y.f()) == DDK_ERR_ARG, "%s: null mask accepted", name);
    CHECK(run(mask.f(), nullptr, gain.f(), nsc.f(), tw.f(), y.f()) == DDK_ERR_ARG, "%s: null P accepted", name);
    CHECK(run(mask.f(), P.f(), nullptr, nsc.f(), tw.f(), y.f()) == DDK_ERR_ARG, "%s: null gain accepted", name);
    CHECK(run(mask.f(), P.f(), gain.f(), nullptr, tw.f(), y.f()) == DDK_ERR_ARG, "%s: null nsc accepted", name);
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), nullptr, y.f()) == DDK_ERR_ARG, "%s: null twiddles accepted", name);
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), tw.f(), nullptr) == DDK_ERR_ARG, "%s: null y accepted", name);
    CHECK(run(mask.f(), P.f(), gain.f() + 1, nsc.f(), tw.f(), y.f()) == DDK_ERR_ARG, "%s: misaligned gain accepted", name);
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), tw.f(), y.f() + 1) == DDK_ERR_ARG, "%s: misaligned y accepted", name);
    a.noise = x.f();
    CHECK(run(mask.f(), P.f(), gain.f(), nsc.f(), tw.f(), y.f()) == DDK_ERR_ARG, "%s: injected noise accepted", name);
    a.noise = nullptr;
    CHECK(launches_now() == l0, "%s: %ld launches after rejected calls", name, launches_now() - l0);
    ddk_unet_destroy(u);
    std::printf("%-38s workspace %zu B (deconvolution %zu B), %ld launches per three-step chain\n", name, bytes, fft_bytes, per_chain);
}

int main() {
    ddk_san_clear();
    lone(3, 3, 16, 16);                 // the smallest plane: 64 threads
    lone(2, 1, 32, 16);                 // N = 512, H > W
    lone(2, 8, 16, 64);
    lone(1, 3, 128, 128);               // the largest plane form: 128 KB of LDS
    lone(1, 3, 128, 256);               // the multi-launch form
    lone(1, 2, 256, 128);
    lone(3, 1, 256, 256);
    chain("plane form, 3x16x16 b2, width 32", 3, 32, {1, 2, 2, 2}, 2, 16, 16);
    chain("plane form, 1x32x32 b3, width 32", 1, 32, {1, 2}, 3, 32, 32);
    chain("multi-launch form, 3x256x256 b1, width 32", 3, 32, {1, 2, 2, 2}, 1, 256, 256);
    long launches, errors;
    ddk_san_stats(&launches, &errors);
    std::printf("fft noisy walk: %ld launches, %ld pointer/geometry errors, %d failed expectations%s%s\n", launches, errors, failures,
                errors ? "; first: " : "", errors ? ddk_san_first_error() : "");
    return (errors || failures) ? 1 : 0;
}
