// restore_walk.cpp -- the host half of the block restore entries (ddk_sampler_run_restore, _masked, _multistep, _noisy, _gray) and of
// the separable ones (ddk_sampler_run_restore_blur, _sep; csrc/unet_plan.hip) under ASan + UBSan on a machine without a GPU
// (`make restore_walk_asan`, csrc/host_sanitize.h; run by tests/test_restore_walk_host.py).  Nothing runs on a device: every entry
// walks a three-step eager chain whose arenas have exactly the sizes the library's own queries returned, a workspace 16 bytes short
// and the plain sampler's are refused, and every argument error must come back before the first launch.  The walk also prints what
// every sampler size query returns for its shapes, one "size" line each, which the test holds against a recorded table.
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <utility>
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

constexpr int T = 100, T_START = 2;
static const int64_t MAP[3] = {0, T / 2, T - 1};

// a 32-wide model of `mults` on in_ch channels, packed from a zero canonical weight
struct Model {
    ddk_unet* u = nullptr;
    std::unique_ptr<Arena> packed;
    Model(int in_ch, std::vector<int> mults) {
        ddk_unet_config cfg{};
        cfg.in_ch = in_ch; cfg.chan = 32; cfg.n_levels = (int)mults.size();
        for (size_t i = 0; i < mults.size(); ++i) cfg.mults[i] = mults[i];
        u = ddk_unet_create(&cfg);
        CHECK(u != nullptr, "ddk_unet_create: %s", ddk_last_error());
        if (!u) std::exit(1);
        packed = std::make_unique<Arena>(ddk_unet_packed_bytes(u), "packed");
        long long max_slot = 0;
        const int n_slots = ddk_unet_num_slots(u);
        for (int i = 0; i < n_slots; ++i) max_slot = std::max(max_slot, ddk_unet_slot_numel(u, i));
        Arena canonical((size_t)max_slot * 4, "canonical weight");
        for (int i = 0; i < n_slots; ++i)
            CHECK(ddk_unet_pack_slot(u, i, canonical.f(), packed->p, nullptr) == DDK_OK, "pack slot %d: %s", i, ddk_last_error());
        CHECK(ddk_unet_finalize_pack(u, packed->p, nullptr) == DDK_OK, "finalize_pack: %s", ddk_last_error());
    }
    ~Model() { ddk_unet_destroy(u); }
};

using Run = std::function<int(const ddk_sampler_args&)>;
using Faults = std::vector<std::pair<const char*, Run>>;

// one entry: the chain on a workspace of exactly `bytes`, the short workspaces, then the faults, each of which must be DDK_ERR_ARG
// before any launch (injected noise is one of every entry's)
static void walk(const std::string& name, const Model& m, int B, int H, int W, size_t bytes, const Run& run, const Faults& faults) {
    const int C = 3;
    const size_t xb = (size_t)B * H * W * C * 4, plain = ddk_sampler_workspace_bytes(m.u, B, H, W, T_START);
    CHECK(plain > 0 && bytes > plain && bytes % 16 == 0, "%s: workspace query %zu against the plain sampler's %zu", name.c_str(), bytes, plain);
    if (!(plain > 0 && bytes > plain)) return;
    Arena x(xb, "x"), tables((size_t)5 * T * 4, "schedule tables"), ws(bytes, "restore sampler workspace");
    ddk_sampler_args a{};
    a.unet = m.u; a.packed = m.packed->p; a.x = x.f(); a.noise = nullptr;
    a.c_recip = tables.f(); a.c_recipm1 = tables.f() + T; a.c1 = tables.f() + 2 * T; a.c2 = tables.f() + 3 * T; a.sigma = tables.f() + 4 * T;
    a.B = B; a.H = H; a.W = W; a.t_start = T_START; a.t_end = 0; a.seed = 1; a.stream_id = 0; a.use_graph = 0;
    a.workspace = ws.p; a.workspace_bytes = bytes;
    long l0 = launches_now();
    CHECK(run(a) == DDK_OK, "%s: %s", name.c_str(), ddk_last_error());
    const long per_chain = launches_now() - l0;
    CHECK(per_chain > 3, "%s: %ld launches in a three-step chain", name.c_str(), per_chain);
    l0 = launches_now();
    ddk_sampler_args b = a;
    b.workspace_bytes = bytes - 16;
    CHECK(run(b) == DDK_ERR_WORKSPACE, "%s: a workspace 16 bytes short accepted", name.c_str());
    b.workspace_bytes = plain;
    CHECK(run(b) == DDK_ERR_WORKSPACE, "%s: the plain sampler's workspace accepted", name.c_str());
    for (const auto& f : faults) CHECK(f.second(a) == DDK_ERR_ARG, "%s: %s accepted", name.c_str(), f.first);
    b = a; b.noise = x.f();
    CHECK(run(b) == DDK_ERR_ARG, "%s: injected noise accepted", name.c_str());
    b = a; b.sigma = nullptr; b.c1 = nullptr;
    CHECK(run(b) == DDK_ERR_ARG, "%s: null schedule tables accepted", name.c_str());
    b = a; b.t_end = 3;
    CHECK(run(b) == DDK_ERR_ARG, "%s: t_end > t_start accepted", name.c_str());
    b = a; b.x = nullptr;
    CHECK(run(b) == DDK_ERR_ARG, "%s: null x accepted", name.c_str());
    CHECK(launches_now() == l0, "%s: %ld launches after rejected calls", name.c_str(), launches_now() - l0);
    std::printf("%-46s workspace %zu B (plain %zu B), %ld launches per three-step chain\n", name.c_str(), bytes, plain, per_chain);
}

// the five block entries at block n: y [B][H/n][W/n][3] (the grey one's a third of it), the mask [B][H/n][W/n] at n = 1 and none at n = 2
static void block_entries(const Model& m, int B, int H, int W, int n) {
    const size_t blocks = (size_t)B * (H / n) * (W / n);
    Arena y(blocks * 3 * 4, "y"), yg(blocks * 4, "grey y"), mask(blocks * 4, "mask"), rows((size_t)3 * T * 4, "c3, lam, sgm");
    const float *c3 = rows.f(), *lam = rows.f() + T, *sgm = rows.f() + 2 * T, *mk = n == 1 ? mask.f() : nullptr;
    const std::string at = ", 3x" + std::to_string(H) + "x" + std::to_string(W) + " b" + std::to_string(B) + " n=" + std::to_string(n) +
                           (mk ? " masked" : "");
    const int64_t down[3] = {0, 60, 50};
    if (n > 1)
        walk("restore" + at, m, B, H, W, ddk_sampler_restore_workspace_bytes(m.u, B, H, W, T_START),
             [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore(&a, MAP, y.f(), n, nullptr); },
             {{"null y", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore(&a, MAP, nullptr, n, nullptr); }},
              {"n = 1", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore(&a, MAP, y.f(), 1, nullptr); }},
              {"n = 3", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore(&a, MAP, y.f(), 3, nullptr); }},
              {"a falling timestep map", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore(&a, down, y.f(), n, nullptr); }}});
    walk("restore_masked" + at, m, B, H, W, ddk_sampler_restore_masked_workspace_bytes(m.u, B, H, W, T_START, n),
         [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_masked(&a, MAP, y.f(), mk, n, nullptr); },
         {{"null y", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_masked(&a, MAP, nullptr, mk, n, nullptr); }},
          {"n = 1 without a mask", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_masked(&a, MAP, y.f(), nullptr, 1, nullptr); }},
          {"n = 16", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_masked(&a, MAP, y.f(), mk, 16, nullptr); }},
          {"a falling timestep map", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_masked(&a, down, y.f(), mk, n, nullptr); }}});
    walk("restore_multistep" + at, m, B, H, W, ddk_sampler_restore_multistep_workspace_bytes(m.u, B, H, W, T_START, n),
         [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_multistep(&a, MAP, c3, y.f(), mk, n, nullptr); },
         {{"null y", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_multistep(&a, MAP, c3, nullptr, mk, n, nullptr); }},
          {"null c3", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_multistep(&a, MAP, nullptr, y.f(), mk, n, nullptr); }},
          {"n = 1 without a mask", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_multistep(&a, MAP, c3, y.f(), nullptr, 1, nullptr); }},
          {"n = 0", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_multistep(&a, MAP, c3, y.f(), mk, 0, nullptr); }}});
    walk("restore_noisy" + at, m, B, H, W, ddk_sampler_restore_noisy_workspace_bytes(m.u, B, H, W, T_START, n),
         [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_noisy(&a, MAP, lam, sgm, y.f(), mk, n, nullptr); },
         {{"null y", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_noisy(&a, MAP, lam, sgm, nullptr, mk, n, nullptr); }},
          {"null lam", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_noisy(&a, MAP, nullptr, sgm, y.f(), mk, n, nullptr); }},
          {"null sgm", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_noisy(&a, MAP, lam, nullptr, y.f(), mk, n, nullptr); }},
          {"n = 1 without a mask", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_noisy(&a, MAP, lam, sgm, y.f(), nullptr, 1, nullptr); }},
          {"n = 5", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_noisy(&a, MAP, lam, sgm, y.f(), mk, 5, nullptr); }}});
    walk("restore_gray" + at, m, B, H, W, ddk_sampler_restore_gray_workspace_bytes(m.u, B, H, W, T_START, n),
         [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_gray(&a, MAP, lam, sgm, yg.f(), mk, n, 1 + (n > 1), nullptr); },
         {{"null y", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_gray(&a, MAP, lam, sgm, nullptr, mk, n, 1, nullptr); }},
          {"null lam", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_gray(&a, MAP, nullptr, sgm, yg.f(), mk, n, 1, nullptr); }},
          {"weights = 0", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_gray(&a, MAP, lam, sgm, yg.f(), mk, n, 0, nullptr); }},
          {"weights = 3", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_gray(&a, MAP, lam, sgm, yg.f(), mk, n, 3, nullptr); }},
          {"n = 3", [&](const ddk_sampler_args& a) { return ddk_sampler_run_restore_gray(&a, MAP, lam, sgm, yg.f(), mk, 3, 1, nullptr); }}});
}

// the deblurring entry on the plane's own y, and the size-changing one on y [B][h][w][3] with Q_h [H][h], Q_w [W][w]
static void separable_entries(const Model& m, int B, int H, int W, int h, int w) {
    const std::string at = ", 3x" + std::to_string(H) + "x" + std::to_string(W) + " b" + std::to_string(B);
    const size_t bytes = ddk_sampler_restore_blur_workspace_bytes(m.u, B, H, W, T_START);
    Arena ph((size_t)H * H * 4, "P_h"), pw((size_t)W * W * 4, "P_w");
    const int64_t down[3] = {0, 60, 50};
    {
        Arena qh((size_t)H * H * 4, "Q_h"), qw((size_t)W * W * 4, "Q_w"), y((size_t)B * H * W * 3 * 4, "y");
        auto run = [&](const ddk_sampler_args& a, const float* p0, const float* p1, const float* q0, const float* q1, const float* yy) {
            return ddk_sampler_run_restore_blur(&a, MAP, p0, p1, q0, q1, yy, nullptr);
        };
        walk("restore_blur" + at, m, B, H, W, bytes, [&](const ddk_sampler_args& a) { return run(a, ph.f(), pw.f(), qh.f(), qw.f(), y.f()); },
             {{"null P_h", [&](const ddk_sampler_args& a) { return run(a, nullptr, pw.f(), qh.f(), qw.f(), y.f()); }},
              {"null P_w", [&](const ddk_sampler_args& a) { return run(a, ph.f(), nullptr, qh.f(), qw.f(), y.f()); }},
              {"null Q_h", [&](const ddk_sampler_args& a) { return run(a, ph.f(), pw.f(), nullptr, qw.f(), y.f()); }},
              {"null Q_w", [&](const ddk_sampler_args& a) { return run(a, ph.f(), pw.f(), qh.f(), nullptr, y.f()); }},
              {"null y", [&](const ddk_sampler_args& a) { return run(a, ph.f(), pw.f(), qh.f(), qw.f(), nullptr); }},
              {"misaligned P_w", [&](const ddk_sampler_args& a) { return run(a, ph.f(), pw.f() + 1, qh.f(), qw.f(), y.f()); }},
              {"misaligned y", [&](const ddk_sampler_args& a) { return run(a, ph.f(), pw.f(), qh.f(), qw.f(), y.f() + 2); }},
              {"H off the grid", [&](ddk_sampler_args a) { a.H += 8; return run(a, ph.f(), pw.f(), qh.f(), qw.f(), y.f()); }},
              {"a falling timestep map", [&](const ddk_sampler_args& a) {
                   return ddk_sampler_run_restore_blur(&a, down, ph.f(), pw.f(), qh.f(), qw.f(), y.f(), nullptr); }}});
    }
    if (h) {
        Arena qh((size_t)H * h * 4, "Q_h"), qw((size_t)W * w * 4, "Q_w"), y((size_t)B * h * w * 3 * 4, "y");
        auto run = [&](const ddk_sampler_args& a, const float* p0, const float* q1, const float* yy, int hh, int ww) {
            return ddk_sampler_run_restore_sep(&a, MAP, p0, pw.f(), qh.f(), q1, yy, hh, ww, nullptr);
        };
        walk("restore_sep" + at + " from " + std::to_string(h) + "x" + std::to_string(w), m, B, H, W, bytes,
             [&](const ddk_sampler_args& a) { return run(a, ph.f(), qw.f(), y.f(), h, w); },
             {{"null P_h", [&](const ddk_sampler_args& a) { return run(a, nullptr, qw.f(), y.f(), h, w); }},
              {"null Q_w", [&](const ddk_sampler_args& a) { return run(a, ph.f(), nullptr, y.f(), h, w); }},
              {"null y", [&](const ddk_sampler_args& a) { return run(a, ph.f(), qw.f(), nullptr, h, w); }},
              {"misaligned Q_w", [&](const ddk_sampler_args& a) { return run(a, ph.f(), qw.f() + 1, y.f(), h, w); }},
              {"h = 0", [&](const ddk_sampler_args& a) { return run(a, ph.f(), qw.f(), y.f(), 0, w); }},
              {"h = 6", [&](const ddk_sampler_args& a) { return run(a, ph.f(), qw.f(), y.f(), 6, w); }},
              {"w above W", [&](const ddk_sampler_args& a) { return run(a, ph.f(), qw.f(), y.f(), h, W + 4); }},
              {"W off the grid", [&](ddk_sampler_args a) { a.W += 8; return run(a, ph.f(), qw.f(), y.f(), h, w); }}});
    }
}

// what every sampler size query returns for one shape: a line per query, the block kinds' with one value per n of NS
static const int NS[4] = {1, 2, 4, 3};
static void sizes(const Model& m, int B, int H, int W, int t) {
    char at[64];
    std::snprintf(at, sizeof at, "3x%dx%d b%d", H, W, B);
    const ddk_unet* u = m.u;
    auto line = [&](const char* q, size_t v) { std::printf("size %s_workspace_bytes %s t_start=%d: %zu\n", q, at, t, v); };
    auto line_n = [&](const char* q, size_t (*f)(const ddk_unet*, int, int, int, int, int)) {
        std::printf("size %s_workspace_bytes %s t_start=%d n=1,2,4,3:", q, at, t);
        for (int n : NS) std::printf(" %zu", f(u, B, H, W, t, n));
        std::printf("\n");
    };
    line("sampler", ddk_sampler_workspace_bytes(u, B, H, W, t));
    line("sampler_multistep", ddk_sampler_multistep_workspace_bytes(u, B, H, W, t));
    line("sampler_inpaint", ddk_sampler_inpaint_workspace_bytes(u, B, H, W, t + 1));
    line("sampler_restore", ddk_sampler_restore_workspace_bytes(u, B, H, W, t));
    line_n("sampler_restore_masked", ddk_sampler_restore_masked_workspace_bytes);
    line_n("sampler_restore_multistep", ddk_sampler_restore_multistep_workspace_bytes);
    line_n("sampler_restore_noisy", ddk_sampler_restore_noisy_workspace_bytes);
    line_n("sampler_restore_gray", ddk_sampler_restore_gray_workspace_bytes);
    line("sampler_restore_blur", ddk_sampler_restore_blur_workspace_bytes(u, B, H, W, t));
    line("sampler_restore_cs", ddk_sampler_restore_cs_workspace_bytes(u, B, H, W, t));
    line("sampler_restore_fft", ddk_sampler_restore_fft_workspace_bytes(u, B, H, W, t));
    line("sampler_restore_fft_noisy", ddk_sampler_restore_fft_noisy_workspace_bytes(u, B, H, W, t));
    if (t != T_START) return;                            // the tail parts do not depend on the chain's length
    auto parts_n = [&](const char* q, int (*f)(const ddk_unet*, int, int, int, int)) {
        std::printf("size %s_tail_parts %s n=1,2,4,3:", q, at);
        for (int n : NS) std::printf(" %d", f(u, B, H, W, n));
        std::printf("\n");
    };
    auto parts = [&](const char* q, int v) { std::printf("size %s_tail_parts %s: %d\n", q, at, v); };
    parts_n("sampler_restore", ddk_sampler_restore_tail_parts);
    parts_n("sampler_restore_masked", ddk_sampler_restore_masked_tail_parts);
    parts_n("sampler_restore_multistep", ddk_sampler_restore_multistep_tail_parts);
    parts_n("sampler_restore_noisy", ddk_sampler_restore_noisy_tail_parts);
    parts_n("sampler_restore_gray", ddk_sampler_restore_gray_tail_parts);
    parts("sampler_restore_blur", ddk_sampler_restore_blur_tail_parts(u, B, H, W));
    parts("sampler_restore_cs", ddk_sampler_restore_cs_tail_parts(u, B, H, W));
    parts("sampler_restore_fft", ddk_sampler_restore_fft_tail_parts(u, B, H, W));
    parts("sampler_restore_fft_noisy", ddk_sampler_restore_fft_noisy_tail_parts(u, B, H, W));
}

int main() {
    ddk_san_clear();
    {
        Model m(3, {1, 2, 2, 2});
        block_entries(m, 2, 16, 16, 1);
        block_entries(m, 2, 16, 16, 2);
        separable_entries(m, 2, 16, 16, 8, 12);
        separable_entries(m, 2, 80, 80, 0, 0);           // above 64 KB an image: the two-launch form through blr.tmp
        sizes(m, 2, 16, 16, T_START);
        sizes(m, 2, 16, 16, 999);
        sizes(m, 2, 80, 80, T_START);
        sizes(m, 1, 256, 256, T_START);                  // the cs / fft kinds' scratch and multi-launch forms
        sizes(m, 2, 16, 48, T_START);                    // off the cs / fft grid, on the blur's
    }
    long launches, errors;
    ddk_san_stats(&launches, &errors);
    std::printf("restore walk: %ld launches, %ld pointer/geometry errors, %d failed expectations%s%s\n", launches, errors, failures,
                errors ? "; first: " : "", errors ? ddk_san_first_error() : "");
    return (errors || failures) ? 1 : 0;
}
