// Internal helpers shared by the libddk.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "ddk.h"

#ifdef DDK_HOST_SANITIZE      // `make asan`: the host half checked on a GPU-less machine (host_sanitize.h); never part of libddk.so
#include "host_sanitize.h"
#endif

namespace ddk {

void set_error(const char* fmt, ...);

inline int fail_arg(const char* what) {
    set_error("bad argument: %s", what);
    return DDK_ERR_ARG;
}

// Checks the launch that was just enqueued (no sync: only catches configuration errors).
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return DDK_ERR_HIP;
    }
    return DDK_OK;
}

#define DDK_REQUIRE(cond, msg)              \
    do {                                    \
        if (!(cond)) return ddk::fail_arg(msg); \
    } while (0)

#define DDK_HIP(call)                                                    \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) {                                          \
            ddk::set_error("%s: %s", #call, hipGetErrorString(e_));      \
            return DDK_ERR_HIP;                                          \
        }                                                                \
    } while (0)

#define DDK_TRY(expr)              \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != DDK_OK) return rc_; \
    } while (0)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline hipStream_t as_stream(ddk_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// ---- device helpers -------------------------------------------------------------------------
// Mish(x) = x * tanh(softplus(x)).  With n = e^x (e^x + 2): tanh(ln(1+e^x)) = n / (n + 2), which has
// no cancellation for x << 0 and one exp + one divide.  For x > 20 softplus(x) == x in torch
// (threshold 20) and tanh(x) rounds to 1 in fp32, so Mish(x) == x.
// exp and the divide use the hardware transcendental units (v_exp_f32 / v_rcp_f32, ~1 ulp each): ~8 instructions per
// element instead of ~30 with the IEEE-exact library versions -- in the GroupNorm kernels the exact form was a third
// of the kernel's time.  Relative error of the result <= ~4e-7 (tests hold elementwise ops to 5e-6).
__device__ __forceinline__ float mish_f(float x) {
    if (x > 20.0f) return x;
    const float e = __expf(x);
    const float n = e * (e + 2.0f);
    return x * (n * __frcp_rn(n + 2.0f));
}

// d/du [u * tanh(softplus(u))]: with e = exp(u), n = e(e+2), t = n/(n+2):  t + u * 4 e (e+1) / (n+2)^2
// (hardware exp / reciprocal as in mish_f: one v_exp_f32 + one v_rcp_f32 instead of a library exp and two IEEE divides -- this
// runs per element in conv epilogues (ddk_conv_args.dmish_src) and in the GroupNorm backward)
__device__ __forceinline__ float mish_grad_f(float u) {
    if (u > 20.0f) return (u - u) + 1.0f;       // 1, and NaN at +Inf as torch's mish backward gives (x * 0 there): a non-finite stays visible
    const float e = __expf(u);
    const float n = e * (e + 2.0f);
    const float r = __frcp_rn(n + 2.0f);
    return n * r + u * (4.0f * e * (e + 1.0f)) * (r * r);
}

// u / upr for the float4-units-per-pixel count of a GroupNorm group (1, 2, 4 or 8 in every reference configuration): a
// shift when upr is a power of two -- the integer divide is ~30 VALU ops and these kernels do it per element, per pass.
__device__ __forceinline__ int div_upr(int u, int upr) {
    return (upr & (upr - 1)) == 0 ? u >> (31 - __builtin_clz(upr)) : u / upr;
}
__device__ __forceinline__ long long div_upr(long long u, int upr) {
    return (upr & (upr - 1)) == 0 ? u >> (31 - __builtin_clz(upr)) : u / upr;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Sum over the whole workgroup (blockDim.x a multiple of 64, <= 1024); result valid in every thread.
// `red` is at least 17 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();  // protect `red` from a previous use
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = (lane < nw) ? red[lane] : 0.0f;
    t = wave_sum(t);
    return t;
}

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = (lane < nw) ? red[lane] : -INFINITY;
    t = wave_max(t);
    return t;
}

// core.hip: per-device one-time setup; conv_igemm.hip / conv_wgrad.hip provide the per-file parts
int ensure_device_init();
int conv_init_device();
int wgrad_init_device();

// ---- internal launchers used by the UNet plan (same arithmetic as the public entry points) ----
// conv_igemm.hip
size_t conv_workspace_bytes(int kind, int B, int H, int W, int cin, int N);
// Channel LayerNorm folded into a 1x1 conv: a.weight must hold W o g (per input channel), c1 = W g, c2 = W b per output
// channel.  Only valid when conv_ln_fold_ok() says so for the shape.
struct ConvLnFold {
    const float* c1;
    const float* c2;
    float eps;
};
// GroupNorm + Mish (+ time shift, + residual = ddk_conv_args.resid) finished inside the Winograd conv's launch: the workgroups
// of one image exchange their per-tile statistics through `records` / `counters` (conv_wino_cluster_ws_floats() floats, the
// counters zero before the first launch; they re-arm themselves)
struct WinoGnFuse {
    const float* gamma;
    const float* beta;
    const float* temb;
    const long long* temb_rows;
    int temb_stride;
    float eps;
    int groups;
    float* records;
    unsigned* counters;
    unsigned* fail;         // sticky count of workgroups that gave up waiting (may be null)
    unsigned* pairs = nullptr;   // shapes whose channel chunks are split (conv_wino_cluster_split_np): conv_wino_cluster_pair_words() zeroed
                                 // words; the partial tiles go through ddk_conv_args::workspace ((splits - 1) slabs)
    // optional: the addend is a 1x1 conv of a narrow tensor, evaluated in the epilogue (the first ResnetBlock's res_conv of the
    // <= 8-channel input, blocks.py:103,115): res_x [B*H*W][res_cin], res_w [N][res_ld] (first res_cin entries of a row), res_b [N] or null
    const float* res_x = nullptr;
    const float* res_w = nullptr;
    const float* res_b = nullptr;
    int res_cin = 0, res_ld = 0;
};
bool conv_ln_fold_ok(int B, int H, int W, int cin, int N);
int conv_forward(const ddk_conv_args& a, hipStream_t st, const ConvLnFold* ln = nullptr, const WinoGnFuse* fuse = nullptr);
int conv_splits(int kind, int B, int H, int W, int cin, int N);
// conv_wino.hip
bool conv_wino_ok(int kind, int H, int W, int cin, int N);
int conv_wino_splits(int B, int H, int W, int cin, int N);
bool conv_wino_skip_ok(int B, int H, int W, int cin, int N);   // the conv can carry a 1x1 skip conv of its input (ddk_conv_args.skip_out)
int conv_wino_forward(const ddk_conv_args& a, int splits, hipStream_t st, const WinoGnFuse* fuse = nullptr);
int conv_wino_cluster_np(int B, int H, int W, int cin, int N, int groups);    // m tiles per image when eligible, else 0
int conv_wino_cluster_split_np(int B, int H, int W, int cin, int N, int groups, int* splits_out);   // the same for k-split shapes
size_t conv_wino_cluster_pair_words(int B, int H, int W, int N);
bool conv_wino_variant_new(int B, int H, int W, int N);   // the shape runs on the 8-matrix-wave kernels (they carry the 1x1 addend)
bool conv_wino_cluster_device_ok();     // a whole MI355X (256 CUs, 8 XCDs, no CU mask): the only place a cluster is co-resident
size_t conv_wino_cluster_ws_floats(int B, int H, int W, int N);
// workgroups of each code object's in-launch exchanges that gave up waiting (cluster_sync.h; ~0u: unreadable)
unsigned conv_wino_cluster_timeouts();
unsigned conv_first_cluster_timeouts();
unsigned level_chain_cluster_timeouts();
unsigned attention_cluster_timeouts();
// The cluster counter area `cl` of a plan's workspace (unet_plan.hip), in 4-byte words and in this order: [B][8 * 16] counters of the
// in-launch GroupNorm (16 per (image, n tile), N <= 512: every layer re-arms the same words); one line for the workspace's sticky give-up
// count (ddk_unet_cluster_check); [B][64] the level chain's arrival and departure counters, a 128-byte line per image each; CL_PAIR_WORDS
// pair counters of the channel-chunk-split in-launch GroupNorm (<= 128 (m tile, n tile) pairs: 256 workgroups, >= 2 splits); [B][4] lines of
// 32 words, the (image, head) pair counters of the pixel-split attention launch (attn_split_kernel); the records.
// A ddk_conv3x3_gn_mish_cluster workspace has the first two only: its records start at cl_front_floats().
constexpr size_t CL_PAIR_WORDS = 128 * 16;
inline size_t cl_fail_offset(int B) { return (size_t)B * 8 * 16; }
inline size_t cl_front_floats(int B) { return cl_fail_offset(B) + 16; }
inline size_t cl_chain_offset(int B) { return cl_front_floats(B); }
inline size_t cl_pair_offset(int B) { return cl_chain_offset(B) + (size_t)B * 64; }
inline size_t cl_attn_offset(int B) { return cl_pair_offset(B) + CL_PAIR_WORDS; }
inline size_t cl_counter_floats(int B) { return cl_attn_offset(B) + (size_t)B * 4 * 32; }   // everything in front of a plan's records
struct ClWords { unsigned* counters; unsigned* fail; };
inline ClWords cl_words(float* cl, int B) { return {reinterpret_cast<unsigned*>(cl), reinterpret_cast<unsigned*>(cl + cl_fail_offset(B))}; }
// waits for `st`, then reads and clears a workspace's sticky give-up word: DDK_OK, or DDK_ERR_CLUSTER with the error
// "<who>: <n> workgroup(s) gave up waiting for their cluster<tail>"
int cluster_fail_check(unsigned* word, hipStream_t st, const char* who, const char* tail);
// transpose conv 4x4 stride 2 as Winograd F(2x2, 2x2) per output phase (weight_wino = ddk_pack_convT_weight_wino)
bool convT_wino_ok(int H, int W, int cin, int N);
int convT_wino_splits(int B, int H, int W, int cin, int N);
int convT_wino_forward(const ddk_conv_args& a, int splits, hipStream_t st);
int conv_wino_init_device();
int conv_wino_stats_parts(int B, int H, int W, int cin, int N, int groups);   // tiles per image, or 0
// conv_first.hip: Conv2d(C_in <= 8, N, 3, padding=1) on the unpadded input, GroupNorm partials in the epilogue; with
// counter / t_cur it also does the sampler's per-step bookkeeping (t_cur[b] <- counter; counter -= 1)
bool conv_first_ok(int cin, int N, int H, int W, int groups);
int conv_first(const float* x, const float* wp, const float* bias, float* out, float* gn_partials, int B, int H, int W, int cin, int N,
               int groups, int64_t* counter, int64_t* t_cur, hipStream_t st);
int conv_first_init_device();
// ... with the Block's GroupNorm + Mish + time shift finished in the same launch (the image's tiles exchange their statistics):
// records = conv_first_gn_ws_floats() floats, counters = [B][8 * 16] zeroed words that re-arm themselves, fail = sticky give-up count
bool conv_first_gn_ok(int cin, int N, int H, int W, int groups);
size_t conv_first_gn_ws_floats(int B, int H, int W);
int conv_first_gn(const float* x, const float* wp, const float* bias, const float* gamma, const float* beta, const float* temb,
                  int temb_stride, const long long* temb_rows, float eps, float* out, int B, int H, int W, int cin, int N, int groups,
                  float* records, unsigned* counters, unsigned* fail, int64_t* counter, int64_t* t_cur, hipStream_t st);
// (in the sampler this kernel reads the step counter in EVERY workgroup -- the time shift's row -- so it must not decrement it: the
//  step's last kernel does, final_tail / p_update with ChainHooks::dec_counter)
// conv1x1_ws.hip: 1x1 conv with 128 input channels on a large map as a weights-stationary, pixel-streaming GEMM
// (w = the packed 1x1 weight [N][128]; ln as in conv_forward)
// conv1x1_sm.hip: 1x1 conv + bias + residual on small maps (32x32 tiles, the four waves split K, no ring)
bool conv1x1_sm_ok(long long M, int c0, int c1, int N);
int conv1x1_sm(const float* src0, int c0, const float* src1, int c1, const float* w, const float* bias, const float* resid, float* out,
               long long M, int N, const ConvLnFold* ln, hipStream_t st);
int conv1x1_sm_init_device();
// conv1x1_stream.hip: 1x1 conv between 32 / 64-channel tensors on large maps as a memory stream (weights in registers, no LDS)
bool conv1x1_stream_ok(long long M, int cin, int N);
int conv1x1_stream(const float* x, int cin, const float* w, const float* bias, const float* dmish_src, const float* resid, float* out,
                   float* mish_out, long long M, int N, int pre_mish, int post_mish, hipStream_t st);
bool conv1x1_ws_ok(long long M, int K, int N);
// images > 0: PER-IMAGE weights -- w is [images][128][128], the LayerNorm vectors [images][128], N == 128, M / images pixels per image
int conv1x1_ws(const float* x, const float* w, const float* bias, const float* resid, float* out, long long M, int N, const ConvLnFold* ln,
               hipStream_t st, int images = 0);
int conv1x1_ws_init_device();
// conv_local.hip: conv3x3 + GroupNorm + Mish (+shift, +residual) in one launch for 4x4 / 8x8 maps
// the addend of the image-local kernels may still be in split-K form (the 1x1 skip conv's slabs): n slabs `stride` floats apart,
// summed in order, plus bias[c] -- the skip conv's reduce launch folded into the consumer's load
struct AddendSlabs {
    int n = 1;
    long long stride = 0;
    const float* bias = nullptr;
};
bool conv_gn_local_ok(int H, int W, int cin, int c0, int N, int groups);
int conv_gn_local(const float* src0, int c0, const float* src1, int c1, const float* w, const float* bias, const float* gamma,
                  const float* beta, const float* temb, int temb_stride, const long long* temb_rows, const float* addend, float* out,
                  int B, int H, int W, int N, int groups, float eps, hipStream_t st, const AddendSlabs& as = AddendSlabs(),
                  const AddendSlabs& src_slabs = AddendSlabs());      // src_slabs.n > 1: src0 is in split-K form (summed while staged)
int conv_gn_local_init_device();
bool conv_gn_wlocal_ok(int H, int W, int cin, int c0, int N, int groups);     // 64-pixel maps: the same in Winograd form
int conv_gn_wlocal(const float* src0, int c0, const float* src1, int c1, const float* w, const float* bias, const float* gamma,
                   const float* beta, const float* temb, int temb_stride, const long long* temb_rows, const float* addend, float* out,
                   int B, int H, int W, int N, int groups, float eps, hipStream_t st, const AddendSlabs& as = AddendSlabs(),
                   const AddendSlabs& src_slabs = AddendSlabs());
double conv_flops(int kind, int B, int H, int W, int cin, int N);
// norm_act.hip
size_t groupnorm_workspace_bytes(int B, int HW, int C, int groups);
int gn_train_nsplit(int HW, int cpg);
int gn_stats_partials(const float* x, float* part, int B, int HW, int C, int groups, int ns, hipStream_t st);
int groupnorm_mish(const float* x, const float* gamma, const float* beta, const float* temb, int temb_stride,
                   const float* addend, float* out, int B, int HW, int C, int groups, float eps, void* ws, size_t ws_bytes,
                   hipStream_t st, const long long* temb_rows = nullptr);
int groupnorm_mish_ex(const float* x, int nslab, long long slab_stride, const float* cbias, const float* gamma,
                      const float* beta, const float* temb, int temb_stride, const float* addend, float* out, int B, int HW, int C,
                      int groups, float eps, void* ws, size_t ws_bytes, hipStream_t st, const long long* temb_rows = nullptr);
// rc_*: optional on-the-fly 1x1 addend  rc_b[c] + sum_k rc_x[pix][k] rc_w[c*rc_ld + k]  (k < rc_cin <= 8), instead of `addend`
int groupnorm_mish_parts(const float* x, const float* part, int np, const float* gamma, const float* beta, const float* temb,
                         int temb_stride, const float* addend, float* out, int B, int HW, int C, int groups, float eps, hipStream_t st,
                         const long long* temb_rows = nullptr, const float* rc_x = nullptr, const float* rc_w = nullptr,
                         const float* rc_b = nullptr, int rc_cin = 0, int rc_ld = 0);
int chan_layernorm(const float* x, const float* g, const float* b, float* out, long long M, int C, float eps, hipStream_t st);
// widths that are not multiples of 32: C real channels in rows of pitch CP = pad32(C), padding kept zero
int groupnorm_mish_generic(const float* x, const float* gamma, const float* beta, const float* temb, int temb_stride, const float* addend,
                           float* out, int B, int HW, int CP, int C, int groups, float eps, hipStream_t st, const long long* temb_rows = nullptr);
int chan_layernorm_generic(const float* x, const float* g, const float* b, float* out, long long M, int CP, int C, float eps, hipStream_t st);
int unary(int op, const float* x, float* out, long long n, hipStream_t st);
int add(const float* a, const float* b, float* out, long long n, hipStream_t st);
int avgpool2(const float* x, float* out, int B, int H, int W, int C, hipStream_t st);
int upsample_nearest2(const float* x, float* out, int B, int H, int W, int C, hipStream_t st);
// attention.hip
size_t linattn_context_workspace_bytes(int B, int HW, int heads);
int linattn_context(const float* qkv, float* ctx, int B, int HW, int heads, void* workspace, size_t workspace_bytes, hipStream_t st,
                    bool kv_only = false);
// folded attention output (attention.hip): per-image C x C matrix A and fold vectors from the context
bool attn_fold_ok(int C, int heads);
bool attn_kvctx_ok(int B, int HW, int C, int heads);     // k, v projection + context in one launch (attention.hip, attn_kvctx_kernel)
size_t attn_kvctx_workspace_bytes(int B, int HW);
int attn_kvctx(const float* x, const float* w_kv, const float* c1, const float* c2, float ln_eps, float* ctx, int B, int HW, void* workspace,
               size_t workspace_bytes, hipStream_t st);
// ... leaving the split records in the workspace (no merge, no ctx) for attn_fold_parts, which folds A, a1, a2 straight from them
int attn_kvctx_splits(int B, int HW);
int attn_kvctx_parts(const float* x, const float* w_kv, const float* c1, const float* c2, float ln_eps, int B, int HW, void* workspace,
                     size_t workspace_bytes, hipStream_t st);
bool attn_fold_parts_ok(int C, int heads, int splits);
int attn_fold_parts(const float* part, int splits, const float* wqg, const float* c1q, const float* c2q, const float* wout, const float* bout,
                    float* A, float* a1, float* a2, int B, int C, int heads, hipStream_t st);
size_t attn_fold_out_floats(int B);
int attn_fold(const float* ctx, const float* wqg, const float* c1q, const float* c2q, const float* wout, const float* bout, float* A,
              float* a1, float* a2, int B, int C, int heads, hipStream_t st);
int linattn_apply(const float* qkv, const float* ctx, float* out, int B, int HW, int heads, hipStream_t st);
int linattn_fused_small(const float* qkv, float* ctx, float* out, int B, int HW, int heads, hipStream_t st);
// to_qkv + core of one (image, head, half of the pixels) per workgroup on 16x16 / 8x8 maps (attention.hip, attn_split_kernel)
bool attn_split_ok(int B, int HW, int C, int heads);
size_t attn_split_counter_words(int B);     // == B * 4 * 32: the plan keeps them at cl_attn_offset()
size_t attn_split_record_floats(int B);
int attn_split(const float* x, const float* w, const float* c1, const float* c2, float ln_eps, float* ctx, float* out, int B, int HW, int C,
               unsigned* counters, float* records, unsigned* fail, hipStream_t st);
bool linattn_small_qkv_ok(int HW, int C);
int linattn_small_qkv_init_device();
int qkv_operand_pack(const float* lnw, float* wop, int heads, int cp, hipStream_t st);
int linattn_small_qkv(const float* x, const float* wop, const float* c1, const float* c2, float ln_eps, float* ctx, float* out, int B, int HW,
                      int C, int heads, hipStream_t st);
// time_embed.hip
int time_mlp(const int64_t* t, const float* freqs, const float* w1t, const float* b1, const float* w2t, const float* b2,
             float* act, float* raw, int B, int dim, hipStream_t st);
int time_proj(const float* act, const float* wt, const float* bias, float* out, int B, int dim, int n_out, hipStream_t st);
// layout_pack.hip
int conv1x1_small_n(const float* x, const float* w, const float* bias, float* out, long long M, int C, int n_out, hipStream_t st);
// diffusion.hip
// RePaint inpainting: the known latent, its mask and the per-row tables of one reverse op
struct InpaintOps {
    const float* known;           // x0 of the known image, same layout as x
    const float* mask;            // same layout as x: nonzero = known
    const float *ka, *kb;         // per row: x_kn = ka x0 + kb z2 (sqrt(abar_{tau-1}), sqrt(1 - abar_{tau-1}))
    const float *ja, *jb;         // per row: the forward jump after the op, x = ja x + jb z3 (jb == 0: no jump)
};
// DDNM+ for a noisy measurement, per row t[b]: the correction's scale and the draw's scale on measured elements
struct NoisyTables {
    const float *lam, *sgm;
};
// DDNM deblurring: the symmetric projections of the two axes and the two-launch form's scratch
struct BlurOps {
    const float* ph;              // [H][H] row-major, P_h = A_h+ A_h
    const float* pw;              // [W][W] row-major
    float* tmp;                   // T = P_h X0, x's layout; read and written only when an image is too large for the one-launch form
    const float *qh, *qw;         // host side only: A+ of the two axes, from which the chain entry forms Yp = Q_h y Q_w^T before the first step
};
static_assert(sizeof(BlurOps) <= sizeof(InpaintOps), "BlurOps shares the Inpaint operands' storage: StepRule must not grow");
// DDNM compressed sensing: the pixel permutation, the scratch form's T and the number of measured coefficients
struct HadamardOps {
    const int32_t* perm;          // [H W]: a[j] = X[perm[j]], shared by channels and batch; read as perm[j] & (H W - 1)
    float* tmp;                   // T [B][C][H W]; read and written only when a plane is too large for the plane form (256 x 256)
    int m;                        // coefficients 0 .. m - 1 of every plane are measured: rst.y is [B][C][m]
};
static_assert(sizeof(HadamardOps) <= sizeof(InpaintOps), "HadamardOps shares the Inpaint operands' storage: StepRule must not grow");
// DDNM deconvolution of a 2-D point-spread function with periodic boundary: the kept frequencies, the FFT's
// twiddles and the multi-launch form's T
struct FftOps {
    const float* mask;            // [H][W], natural frequency order: nonzero where the frequency is kept (zeroed in x0's spectrum)
    const float* tw;              // [max(H, W) / 2] complex (re, im): exp(-2 pi i j / max(H, W)), float64 on the host rounded to fp32
    float* tmp;                   // T [B][C][H W] complex; read and written only when a plane is too large for the plane form (above 16384 pixels)
    const float* pinv;            // host side only: P^ [H][W] complex, from which the chain entry forms Yp = A+ y before the first step
};
static_assert(sizeof(FftOps) <= sizeof(InpaintOps), "FftOps shares the Inpaint operands' storage: StepRule must not grow");
// DDNM+ deconvolution of a noisy blurred image: FftOps, then the per-frequency gain and the per-row noise scale.
// The spectrum of A+ y rides in rst.y.
struct FftNoisyOps {
    const float* mask;            // as FftOps
    const float* tw;              // as FftOps
    float* tmp;                   // T, and behind it T2 of the same size ([2][B][C][H W] complex); multi-launch form only
    const float* gain;            // [H][W], natural frequency order: 1 / |K^| where kept, 0 elsewhere
    const float* nsc;             // per row t[b]: |c1| sigma_y
    const float* pinv;            // host side only: P^ [H][W] complex, from which the chain entry forms the spectrum of A+ y before the first step
};
static_assert(sizeof(FftNoisyOps) <= sizeof(InpaintOps), "FftNoisyOps shares the Inpaint operands' storage: StepRule must not grow");
constexpr uint32_t INPAINT_Z2_BIT = 0x40000000u;   // Philox stream of the known region's draw: stream_id | this
constexpr uint32_t INPAINT_Z3_BIT = 0x20000000u;   // ... and of the jump's: stream_id | this (so stream_id < 2^29)
// zero-shot super-resolution (DDNM for A = n x n average pooling): the low-resolution image and the block
struct RestoreOps {
    const float* y;               // NHWC [B][H/n][W/n][n_out]: what the n x n block means of x0 are set to
    int n;                        // 2, 4 or 8, dividing H and W
    int H, W;                     // the map the blocks lie in (filled by the chain entry / the lone op; the other kinds need only `per`)
    int gray;                     // StepKind::RestoreGray: the channel weights, GRAY_MEAN or GRAY_LUMA; 0 in every other kind.  y is then
                                  // [B][H/n][W/n] (one channel).  In the four bytes that were padding in front of `mask`
    const float* mask;            // StepKind::RestoreMasked, RestoreMultistep, RestoreNoisy, RestoreGray: [B][H/n][W/n], nonzero = measured, shared by the
                                  // channels; n may be 1 (RestoreMultistep, RestoreNoisy at n >= 2, RestoreGray at every n: may be null, all measured)
};
// the kernels take RestoreOps by value inside StepRule / TailParams: neither its size nor the place of `mask` may move
static_assert(sizeof(RestoreOps) == 32 && offsetof(RestoreOps, mask) == 24, "RestoreOps: gray fills the padding, nothing moves");
constexpr int GRAY_MEAN = 1;      // w = (1/3, 1/3, 1/3): DDNM's colourisation operator
constexpr int GRAY_LUMA = 2;      // w = (0.299, 0.587, 0.114): BT.601 luma
// likelihood sweep (ddk_vlb_sweep_run): one step's operands besides the UNet's
struct VlbStep {
    const float* x;               // clean sample, NHWC [B][H][W][n_out]
    float* xt;                    // q_sample(x, t, eps), the forward's input
    const float* noise;           // [T][B][H][W][n_out] (draw k at t = t_first - k) or null: Philox on the chain state's key
    long long noise_step_stride;
    int t_first;
    const float *c_recip, *c_recipm1, *c1, *c2, *logvar;
    float* partials;              // float2 [T][B][nslot]
    int nslot;                    // tiles of the fused tail, or vlb_sweep_slots_unfused()
};
constexpr uint32_t VLB_STREAM_BIT = 0x80000000u;   // Philox stream ids of the sweep: stream_id | this (never the sampler's)

// How a forward ends.  The kind is the one thing a chain entry hands forward_core, and forward_core hands the fused tail
// (final_tail) or the unfused update (p_update); each kind reads the members listed with it and no others.
enum class StepKind {
    Eps,          // plain forward: eps_hat to eps_out, no update
    Ancestral,    // x <- p_step(x, eps_hat, z): tables c_recip .. sigma; z = injected noise or Philox; eps_out optional
    Multistep,    // DPM-Solver++(2M): x <- (c1 x0 + c2 x) + c3 x0_hist, x0_hist <- x0: c_recip .. c2, c3, x0_hist; no draw
    Inpaint,      // RePaint: Ancestral's op, then x = mask ? x_kn : x, then the optional jump: c_recip .. sigma, inp; Philox only
    Restore,      // DDNM super-resolution: Ancestral's x0 shifted so its n x n block means equal y, then the update: c_recip .. sigma, rst; Philox only
    RestoreMasked,  // DDNM for A = mask o pool_n, n in {1, 2, 4, 8}: Restore's step where the block's rst.mask is nonzero,
                  // Ancestral's where it is zero (a select; n = 1: x0' = y, no arithmetic): c_recip .. sigma, rst with mask; Philox only
    Vlb,          // likelihood sweep: no update, the step's VLB terms to vlb->partials (vlb_rule() fills the rest from *vlb)
    RestoreMultistep,  // DDNM on the DPM-Solver++(2M) chain, n in {1, 2, 4, 8}: RestoreMasked's x0' (rst.mask null at n >= 2:
                  // every block measured), then Multistep's update on it, x0_hist <- x0': c_recip .. c2, c3, x0_hist, rst; no draw
    RestoreNoisy,  // DDNM+ for a measurement with noise of standard deviation sigma_y, n in {1, 2, 4, 8}: RestoreMasked's
                  // step with the correction scaled by lam and the draw of measured elements by sgm instead of sigma (rst.mask null at
                  // n >= 2: every block measured): c_recip .. sigma, lam, sgm, rst; Philox only
    RestoreGray,  // DDNM / DDNM+ for A = mask o pool_n o grey_w on a 3-channel map, n in {1, 2, 4, 8}: RestoreNoisy's step
                  // with the block mean replaced by the weighted mean of the n x n x 3 group and the correction spread by A+'s per-channel
                  // factor (rst.gray names w; rst.mask may be null at every n): c_recip .. sigma, nsy, rst; Philox only
    RestoreBlur,  // DDNM for a separable blur A(X) = A_h X A_w^T per channel: x0' = (x0 - P_h x0 P_w^T) + Yp with the
                  // projections P = A+ A of the two axes and Yp = A+ y, then Restore's update.  The only plane-wide kind: separable.hip's
                  // kernels, never the fused tail: c_recip .. sigma, blr, rst.y = Yp (x's layout), rst.H, rst.W; Philox only
    RestoreHadamard, // DDNM compressed sensing, A = the first m rows of the orthonormal Walsh-Hadamard transform of the permuted plane
                  // (DESIGN.md section 3.17): x0' = A^T y + (I - A^T A) x0, a select between two transforms, then Restore's update.
                  // Plane-wide: hadamard.hip's kernels, never the fused tail: c_recip .. sigma, had, rst.y = y [B][C][m], rst.H, rst.W;
                  // Philox only
    RestoreFFT,   // DDNM deconvolution, A = circular convolution with a 2-D point-spread function:
                  // x0' = Re F2^-1(M ? 0 : F2 x0) / N + Yp, a select between two complex FFTs in LDS, then Restore's update.  Plane-wide:
                  // fft_conv.hip's kernels, never the fused tail: c_recip .. sigma, fft, rst.y = Yp (x's layout), rst.H, rst.W; Philox only
                  // (behind every older kind, so that the kinds above keep their values and their kernels' names)
    RestoreFFTNoisy  // DDNM+ for RestoreFFT's operator and a blurred image with noise of standard deviation sigma_y (DESIGN.md section
                  // 3.19): per frequency, the correction scaled by lam and the draw shaped by phi between the same two FFTs.  Plane-wide:
                  // fft_conv.hip's kernels, never the fused tail: c_recip .. sigma, fnz, rst.y = the spectrum of A+ y ([B][C][H W]
                  // complex, the transform's order), rst.H, rst.W; Philox only (last, for the same reason)
};
// the restore kinds whose operator couples a whole plane: no n x n block, never the fused tail.  The one list of them (RestoreTraits,
// restore_rule_fault, final_tail_ok and the chain's staging in unet_plan.hip read it)
constexpr bool plane_kind(StepKind k) {
    return k == StepKind::RestoreBlur || k == StepKind::RestoreHadamard || k == StepKind::RestoreFFT || k == StepKind::RestoreFFTNoisy;
}
constexpr bool restore_kind(StepKind k) {    // the kinds whose step carries a DDNM constraint (RestoreOps)
    return k == StepKind::Restore || k == StepKind::RestoreMasked || k == StepKind::RestoreMultistep || k == StepKind::RestoreNoisy ||
           k == StepKind::RestoreGray || plane_kind(k);
}
struct StepRule {
    StepKind kind;
    float* eps_out;               // [B][HW][n_out] or null (fused tail only; the unfused tail's eps_hat is its input)
    float* x;                     // [B][HW][n_out] chain state, updated in place (Vlb: the clean sample, read only)
    const float* noise;           // injected draws: draw k = t_first - t of a [n_steps][...] array (stride 0: a single tensor), or null
    long long noise_step_stride;
    int t_first;
    const float *c_recip, *c_recipm1, *c1, *c2, *sigma;     // per row t[b]
    float* x0_hist;               // Multistep: the previous step's clipped x0 (RestoreMultistep: its x0'), same layout as x, read and rewritten
    const float* c3;
    // A rule has one kind, so the Inpaint kind's operands and the RestoreNoisy kind's tables share their storage: the unfused kernels
    // take a StepRule by value, and a larger one would move every argument behind it and with that the instructions of the older kernels.
    union {
        InpaintOps inp;
        NoisyTables nsy;          // RestoreNoisy, RestoreGray
        BlurOps blr;              // RestoreBlur
        HadamardOps had;          // RestoreHadamard
        FftOps fft;               // RestoreFFT
        FftNoisyOps fnz;          // RestoreFFTNoisy
    };
    const VlbStep* vlb;           // host side only
    RestoreOps rst;
};
static_assert(sizeof(StepRule) == 192, "StepRule is a kernel argument: its layout stays byte for byte (see the union's comment)");
inline StepRule vlb_rule(const VlbStep& v) {
    StepRule r{};
    r.kind = StepKind::Vlb;
    r.x = const_cast<float*>(v.x); r.noise = v.noise; r.noise_step_stride = v.noise_step_stride; r.t_first = v.t_first;
    r.c_recip = v.c_recip; r.c_recipm1 = v.c_recipm1; r.c1 = v.c1; r.c2 = v.c2;
    r.vlb = &v;
    return r;
}
// What a step's last kernel does for its chain besides the rule (all optional: a lone call has a host seed / stream id)
struct ChainHooks {
    const int64_t* chain_state;   // {counter, Philox seed, stream id} in device memory: one captured graph serves every seed
    int64_t* dec_counter;         // the step counter, decremented by this (last) kernel of the step when the first kernel left it alone
    uint64_t seed;                // without chain_state
    uint32_t stream_id;
};
// the unfused tail's last kernel, given eps_hat in memory: the rule's update of x (Ancestral, Multistep, Inpaint, Restore, RestoreMasked,
// RestoreMultistep, RestoreNoisy, RestoreGray, RestoreBlur, RestoreHadamard, RestoreFFT, RestoreFFTNoisy) or the sweep's
// reduction of the step's terms (Vlb); `who` names the caller in messages
int p_update(const StepRule& r, const float* eps_hat, const int64_t* t, int B, long long per, const ChainHooks& h, hipStream_t st,
             const char* who = "p_update");
// separable.hip: the RestoreBlur kind's step (p_update hands it over once restore_rule_fault has passed the rule), and whether an
// image of this shape takes the one-launch form (else the rule needs blr.tmp)
int p_update_restore_blur(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st);
bool restore_blur_shape_ok(int H, int W, int channels);
bool restore_blur_one_launch(int H, int W, int channels);
int separable_init_device();
// hadamard.hip: the RestoreHadamard kind's step, the shapes it takes (H, W powers of two in [16, 256], 1..8 channels; m a multiple of
// 4 in [4, H W]) and whether a plane takes the one-launch plane form (else the rule needs had.tmp)
int p_update_restore_cs(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st);
bool restore_cs_shape_ok(int H, int W, int channels);
bool restore_cs_rows_ok(int H, int W, int m);
bool restore_cs_plane_form(int H, int W);
int hadamard_init_device();
// fft_conv.hip: the RestoreFFT kind's step, the shapes it takes (H, W powers of two in [16, 256], 1..8 channels), whether a plane takes
// the one-launch plane form (else the rule needs fft.tmp), and the circular convolution behind ddk_circular_conv (out = Re F2^-1(mul .
// F2 in) / N), which the chain entry forms Yp with; circular_conv_fault is null for sound arguments
int p_update_restore_fft(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st);
bool restore_fft_shape_ok(int H, int W, int channels);
bool restore_fft_plane_form(int H, int W);
const char* circular_conv_fault(const void* in, const void* mul, const void* tw, const void* out, const void* scratch, int B, int H, int W, int C);
int circular_conv(const float* in, const float* mul, const float* tw, float* out, float* scratch, int B, int H, int W, int C, hipStream_t st);
int fft_conv_init_device();
// ... the RestoreFFTNoisy kind's step (the same shapes; a plane above the plane form needs fnz.tmp of twice T's size), and the forward
// half of circular_conv that forms the spectrum of A+ y: out [B][C][H W] complex = mul . F2(in) in the transform's order
int p_update_restore_fft_noisy(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st);
int circular_spectrum(const float* in, const float* mul, const float* tw, float* out, float* scratch, int B, int H, int W, int C, hipStream_t st);
int randn(float* out, long long n, uint64_t seed, uint32_t step, uint32_t stream_id, hipStream_t st);
int vlb_sweep_slots_unfused(int B, long long per);
int vlb_step_input(const VlbStep& v, const float* sqrt_acp, const float* sqrt_1m_acp, const int64_t* chain_state, int B, long long per,
                   hipStream_t st);
int vlb_sweep_finalize(const float* partials, int nslot, float* vlb_t, float* l_simple_t, int T, int B, long long per, hipStream_t st);
// GroupNorm (from conv partials) + Mish + 1x1 projection to n_out <= 8 channels, then the rule, in one launch (final_tail_kernel)
struct TailIn {
    const float* raw;             // [B][HW][C] output of the final Block's conv
    const float* part;            // [B*np][G] {mean, M2} per (128-pixel tile, group)
    int np;
    const float *gamma, *beta;
    float eps;
    const float* w;               // [n_out][C]
    const float* bias;            // [n_out] or null
    int n_out, B, HW, C, groups;
};
// the shapes the fused tail takes: C in {32,64,128,256}; the Multistep, Inpaint, Restore and Vlb instantiations stop at C = 128 (at
// 256 the plain one spills already, and theirs hold more in the prologue).  Restore also needs every 128-pixel tile to hold whole
// rows of blocks, 128 % (W n) == 0 with W, n = restore_w, restore_n (W = 32: n <= 4; W = 16: n <= 8; W = 64: n = 2); the other
// kinds ignore the two.  RestoreMasked: as Restore for n >= 2; n = 1 is pointwise and needs no whole blocks, so every shape of the
// Multistep / Inpaint kinds is taken.  RestoreMultistep, RestoreNoisy: as RestoreMasked.  RestoreGray: n_out == 3, and as RestoreMasked
// (its n = 1 sums the pixel's three channels, which lie in the tile whatever W is).  The one predicate of fused_tail_parts
// (unet_plan.hip) and final_tail.
bool final_tail_ok(int HW, int C, int groups, int n_out, int np, StepKind kind, int restore_w = 0, int restore_n = 0);
int final_tail(const TailIn& in, const StepRule& r, const int64_t* t, const ChainHooks& h, hipStream_t st);

}  // namespace ddk
