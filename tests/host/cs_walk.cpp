// cs_walk.cpp -- the host half of the compressed-sensing entries (csrc/hadamard.hip, ddk_sampler_run_restore_cs in csrc/unet_plan.hip)
// under ASan + UBSan on a machine without a GPU (`make cs_walk_asan`, csrc/host_sanitize.h; run by tests/test_restore_cs_host.py).
// Nothing runs on a device: every launch's geometry and pointer arguments are checked against arenas of exactly the sizes the
// library's own size queries returned, in the plane form and in the scratch form, and every argument error must come back before
// the first launch.
#include <sys/mman.h>

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
    int32_t* i() const { return static_cast<int32_t*>(p); }
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

// the lone transforms and the lone step: one launch in the plane form; two (transforms) or three (step) through the scratch
static void lone(int B, int C, int H, int W, int m) {
    const size_t N = (size_t)H * W, xb = (size_t)B * C * N * 4;
    const bool scratch_form = N > 32768;
    Arena x(xb, "x"), eps(xb, "eps_hat"), y((size_t)B * C * m * 4, "y"), perm(N * 4, "perm"), tmp(scratch_form ? xb : 16, "scratch"),
        t((size_t)B * 8, "t"), tab(5 * 4 * 4, "tables");
    float* sc = scratch_form ? tmp.f() : nullptr;
    const float *cr = tab.f(), *crm1 = tab.f() + 4, *c1 = tab.f() + 8, *c2 = tab.f() + 12, *sg = tab.f() + 16;
    long l0 = launches_now();
    CHECK(ddk_hadamard_measure(x.f(), perm.i(), y.f(), sc, B, H, W, C, m, nullptr) == DDK_OK, "measure %dx%dx%d m=%d: %s", C, H, W, m, ddk_last_error());
    CHECK(launches_now() - l0 == (scratch_form ? 2 : 1), "measure %dx%d: %ld launches", H, W, launches_now() - l0);
    l0 = launches_now();
    CHECK(ddk_hadamard_adjoint(y.f(), perm.i(), x.f(), sc, B, H, W, C, m, nullptr) == DDK_OK, "adjoint %dx%dx%d m=%d: %s", C, H, W, m, ddk_last_error());
    CHECK(launches_now() - l0 == (scratch_form ? 2 : 1), "adjoint %dx%d: %ld launches", H, W, launches_now() - l0);
    l0 = launches_now();
    CHECK(ddk_p_sample_update_restore_cs(x.f(), eps.f(), y.f(), perm.i(), sc, t.l(), cr, crm1, c1, c2, sg, B, H, W, C, m, 1, 0, nullptr) == DDK_OK,
          "step %dx%dx%d m=%d: %s", C, H, W, m, ddk_last_error());
    CHECK(launches_now() - l0 == (scratch_form ? 3 : 1), "step %dx%d: %ld launches", H, W, launches_now() - l0);
    // every argument error comes back before any launch
    l0 = launches_now();
    CHECK(ddk_hadamard_measure(x.f(), perm.i(), y.f(), sc, B, H, W, C, m + 2, nullptr) == DDK_ERR_ARG, "m %% 4 != 0 accepted");
    CHECK(ddk_hadamard_measure(x.f(), perm.i(), y.f(), sc, B, H, W, C, (int)N + 4, nullptr) == DDK_ERR_ARG, "m > N accepted");
    CHECK(ddk_hadamard_measure(x.f(), perm.i(), y.f(), sc, B, H + 8, W, C, m, nullptr) == DDK_ERR_ARG, "H no power of two accepted");
    CHECK(ddk_hadamard_measure(x.f(), perm.i(), y.f(), sc, B, H, W, 9, m, nullptr) == DDK_ERR_ARG, "nine channels accepted");
    CHECK(ddk_hadamard_measure(x.f() + 1, perm.i(), y.f(), sc, B, H, W, C, m, nullptr) == DDK_ERR_ARG, "misaligned x accepted");
    CHECK(ddk_hadamard_measure(x.f(), nullptr, y.f(), sc, B, H, W, C, m, nullptr) == DDK_ERR_ARG, "null perm accepted");
    CHECK(ddk_hadamard_adjoint(nullptr, perm.i(), x.f(), sc, B, H, W, C, m, nullptr) == DDK_ERR_ARG, "null y accepted");
    CHECK(ddk_hadamard_adjoint(y.f(), perm.i(), x.f(), sc, 0, H, W, C, m, nullptr) == DDK_ERR_ARG, "B = 0 accepted");
    CHECK(ddk_p_sample_update_restore_cs(x.f(), eps.f(), y.f(), perm.i(), sc, t.l(), cr, crm1, c1, c2, nullptr, B, H, W, C, m, 1, 0, nullptr) == DDK_ERR_ARG,
          "null sigma accepted");
    CHECK(ddk_p_sample_update_restore_cs(x.f(), eps.f(), y.f(), perm.i(), sc, t.l(), cr, crm1, c1, c2, sg, B, H, W, C, 0, 1, 0, nullptr) == DDK_ERR_ARG,
          "m = 0 accepted");
    if (scratch_form) {
        CHECK(ddk_hadamard_measure(x.f(), perm.i(), y.f(), nullptr, B, H, W, C, m, nullptr) == DDK_ERR_ARG, "scratch form without a scratch accepted");
        CHECK(ddk_p_sample_update_restore_cs(x.f(), eps.f(), y.f(), perm.i(), nullptr, t.l(), cr, crm1, c1, c2, sg, B, H, W, C, m, 1, 0, nullptr) ==
                  DDK_ERR_ARG, "scratch form step without a scratch accepted");
    }
    CHECK(launches_now() == l0, "lone %dx%d: %ld launches after rejected calls", H, W, launches_now() - l0);
}

// a three-step eager chain of the new kind on a workspace of exactly the queried size
static void chain(const char* name, int in_ch, int chan, std::vector<int> mults, int B, int H, int W, int m) {
    ddk_unet_config cfg{};
    cfg.in_ch = in_ch; cfg.chan = chan; cfg.n_levels = (int)mults.size();
    for (size_t i = 0; i < mults.size(); ++i) cfg.mults[i] = mults[i];
    ddk_unet* u = ddk_unet_create(&cfg);
    CHECK(u != nullptr, "%s: ddk_unet_create: %s", name, ddk_last_error());
    if (!u) return;
    const int T = 100;
    const size_t packed_bytes = ddk_unet_packed_bytes(u), N = (size_t)H * W, xb = (size_t)B * N * in_ch * 4;
    const size_t plain = ddk_sampler_workspace_bytes(u, B, H, W, 2), cs_bytes = ddk_sampler_restore_cs_workspace_bytes(u, B, H, W, 2);
    CHECK(plain > 0 && cs_bytes == plain + N * 4 + 2 * xb, "%s: workspace query %zu against the plain sampler's %zu", name, cs_bytes, plain);
    CHECK(ddk_sampler_restore_cs_tail_parts(u, B, H, W) == 0, "%s: tail parts", name);
    CHECK(ddk_sampler_restore_cs_workspace_bytes(u, B, H + 8, W, 2) == 0, "%s: off-grid workspace query", name);
    Arena packed(packed_bytes, "packed");
    long long max_slot = 0;
    const int n_slots = ddk_unet_num_slots(u);
    for (int i = 0; i < n_slots; ++i) max_slot = std::max(max_slot, ddk_unet_slot_numel(u, i));
    Arena canonical((size_t)max_slot * 4, "canonical weight");
    for (int i = 0; i < n_slots; ++i)
        CHECK(ddk_unet_pack_slot(u, i, canonical.f(), packed.p, nullptr) == DDK_OK, "%s: pack slot %d: %s", name, i, ddk_last_error());
    CHECK(ddk_unet_finalize_pack(u, packed.p, nullptr) == DDK_OK, "%s: finalize_pack: %s", name, ddk_last_error());
    Arena x(xb, "x"), y((size_t)B * in_ch * m * 4, "y"), perm(N * 4, "perm"), tables((size_t)5 * T * 4, "schedule tables"), ws(cs_bytes, "cs sampler workspace");
    const int64_t map[3] = {0, T / 2, T - 1};
    ddk_sampler_args a{};
    a.unet = u; a.packed = packed.p; a.x = x.f(); a.noise = nullptr;
    a.c_recip = tables.f(); a.c_recipm1 = tables.f() + T; a.c1 = tables.f() + 2 * T; a.c2 = tables.f() + 3 * T; a.sigma = tables.f() + 4 * T;
    a.B = B; a.H = H; a.W = W; a.t_start = 2; a.t_end = 0; a.seed = 1; a.stream_id = 0; a.use_graph = 0;
    a.workspace = ws.p; a.workspace_bytes = cs_bytes;
    long l0 = launches_now();
    CHECK(ddk_sampler_run_restore_cs(&a, map, y.f(), perm.i(), m, nullptr) == DDK_OK, "%s: sampler_run_restore_cs: %s", name, ddk_last_error());
    const long per_chain = launches_now() - l0;
    CHECK(per_chain > 3, "%s: %ld launches in a three-step chain", name, per_chain);
    l0 = launches_now();
    a.workspace_bytes = cs_bytes - 4;
    CHECK(ddk_sampler_run_restore_cs(&a, map, y.f(), perm.i(), m, nullptr) == DDK_ERR_WORKSPACE, "%s: short workspace accepted", name);
    a.workspace_bytes = plain;          // the plain sampler's size is not enough either
    CHECK(ddk_sampler_run_restore_cs(&a, map, y.f(), perm.i(), m, nullptr) == DDK_ERR_WORKSPACE, "%s: the plain sampler's workspace accepted", name);
    a.workspace_bytes = cs_bytes;
    CHECK(ddk_sampler_run_restore_cs(&a, map, y.f(), perm.i(), m + 1, nullptr) == DDK_ERR_ARG, "%s: m %% 4 != 0 accepted", name);
    CHECK(ddk_sampler_run_restore_cs(&a, map, nullptr, perm.i(), m, nullptr) == DDK_ERR_ARG, "%s: null y accepted", name);
    CHECK(ddk_sampler_run_restore_cs(&a, map, y.f(), nullptr, m, nullptr) == DDK_ERR_ARG, "%s: null perm accepted", name);
    a.noise = x.f();
    CHECK(ddk_sampler_run_restore_cs(&a, map, y.f(), perm.i(), m, nullptr) == DDK_ERR_ARG, "%s: injected noise accepted", name);
    a.noise = nullptr;
    CHECK(launches_now() == l0, "%s: %ld launches after rejected calls", name, launches_now() - l0);
    ddk_unet_destroy(u);
    std::printf("%-34s workspace %zu B (plain %zu B), %ld launches per three-step chain\n", name, cs_bytes, plain, per_chain);
}

int main() {
    ddk_san_clear();
    lone(3, 3, 16, 16, 100);            // the smallest plane: 64 threads
    lone(2, 1, 16, 32, 4);              // N = 512
    lone(2, 8, 32, 32, 1024);           // every coefficient measured
    lone(1, 3, 128, 256, 8192);         // the largest plane form: 128 KB of LDS
    lone(1, 3, 256, 256, 16384);        // the scratch form
    lone(3, 1, 256, 256, 65536);
    chain("plane form, 3x16x16 b2, width 32", 3, 32, {1, 2, 2, 2}, 2, 16, 16, 100);
    chain("plane form, 1x32x32 b3, width 32", 1, 32, {1, 2}, 3, 32, 32, 256);
    chain("scratch form, 3x256x256 b1, width 32", 3, 32, {1, 2, 2, 2}, 1, 256, 256, 16384);
    long launches, errors;
    ddk_san_stats(&launches, &errors);
    std::printf("cs walk: %ld launches, %ld pointer/geometry errors, %d failed expectations%s%s\n", launches, errors, failures,
                errors ? "; first: " : "", errors ? ddk_san_first_error() : "");
    return (errors || failures) ? 1 : 0;
}
