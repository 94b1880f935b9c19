// separable.hip -- out = L . in . R^T per channel of an NHWC tensor, and the DDNM deblurring step built on it.
//
// A separable blur A(X) = A_h X A_w^T is not block-local: its range-space projection P_h X P_w^T couples every pixel of a plane, so the
// RestoreBlur kind's x0' needs two small dense products per plane where the other restore kinds need a block mean.  Both products are
// the same 16 x 16 tile on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain per result, no atomics, a fixed summation order: results
// are bit-identical run to run and between eager launches and graph replay):
//
//   D[m][n] = sum_k M[m0 + m][k] S[k][n]        M: rows of L, R, P_h or P_w in global memory (L2-resident: at most 256 KB)
//                                               S: [K][16] in LDS at pitch SP = 20
//
// The image is read as the matrix [H][N], N = W C.  Rows:  T = M X with S a 16-column strip of X, so D is T[16 rows][the strip].
// Columns: per (16 rows h0.., channel c), S[k][n] = T[h0 + n][k][c], so D[m][n] = out[h0 + n][m0 + m][c] -- the transposed tile, which
// lets both products take their matrix operand as float4s along k from row-major storage.  A lane (i = lane & 15, g = lane >> 4) loads
// M[m0 + i][16 s + 4 g .. + 3] and feeds component q to the q-th MFMA of super-step s, whose S operand is S[16 s + 4 g + q][i]: the
// sum runs over every k once, in an order that is the same for every tile.  LDS address (16 s + 4 g + q) SP + i: SP = 20 puts the four
// g at banks 16 g + i (80 g = 16 g mod 64), all 64 distinct; a pitch of 16 would put them on the same 16.
// Two accumulators alternate (the MFMA's dependent latency is 40 cycles against a 32-cycle issue) and are added at the end.
//
// Compiled with -ffp-contract=off (Makefile): the step's elementwise arithmetic rounds every operation like diffusion.hip's.
#include "ddk_internal.h"
#include "diffusion_step.h"

namespace ddk {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SP = 20;            // LDS pitch of a [K][16] operand
constexpr int SEP_MAX = 256;      // H, W <= 256: a strip is at most [256][SP] floats of LDS

__device__ __forceinline__ f32x4 sep_tile(const float* __restrict__ Mrows, int K, const float* S, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const float4* __restrict__ a = reinterpret_cast<const float4*>(Mrows + (size_t)i * K) + g;
    const float* b = S + 4 * g * SP + i;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < K / 16; ++s) {
        const float4 av = a[4 * s];
        const float* bs = b + 16 * s * SP;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bs[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bs[SP], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bs[2 * SP], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bs[3 * SP], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// one deblurring step's operands (by value into the kernels; the chain's StepRule never grows for them)
struct BlurStep {
    float* x;                     // [B][H][W][C], updated in place
    const float* eps;             // eps_hat, same layout
    const float *ph, *pw;         // [H][H], [W][W]
    const float* yp;              // A+ y, x's layout
    float* tmp;                   // T = P_h X0, x's layout (two-launch form only)
    const int64_t* t;
    const float *c_recip, *c_recipm1, *c1, *c2, *sigma;
    int H, W, C;
};

// the element's update once its projection pr = (P_h x0 P_w^T)[e] is known: x0 again from x and eps_hat (it never goes through memory),
// x0' = (x0 - pr) + Yp, not clamped again, then the Restore kind's finish with the Ancestral kind's Philox keying
__device__ __forceinline__ void blur_finish(const BlurStep& p, long long e, float pr, int64_t tb, float cr, float crm1, float a1, float a2,
                                            float sg, uint64_t seed, uint32_t stream) {
    const float xv = p.x[e];
    const float x0 = rst_x0(xv, p.eps[e], cr, crm1);
    const float x0p = __fadd_rn(__fsub_rn(x0, pr), p.yp[e]);
    float z = comp4(philox_normal4((unsigned long long)(e >> 2), (uint32_t)tb, stream, seed), (int)(e & 3));
    p.x[e] = rst_finish<StepKind::RestoreBlur>(xv, x0p, 1.0f, z, a1, a2, sg, 0.0f);
}

// Rows: dst[b][:, strip] = M . src[b][:, strip] for one 16-column strip of the [H][N] matrix per workgroup (grid: N / 16, B).  X0: src is
// the clipped x0 of (p.x, p.eps) and dst is p.tmp; else src -> dst, which may be the same tensor (the strip is in LDS before any write).
template <bool X0>
__global__ __launch_bounds__(256) void sep_rows_kernel(const BlurStep p, const float* __restrict__ src, const float* __restrict__ M,
                                                       float* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float S[SEP_MAX * SP];
    const int H = p.H, N = p.W * p.C, n0 = blockIdx.x * 16, b = blockIdx.y;
    const long long base = (long long)b * H * N + n0;
    float cr = 0.f, crm1 = 0.f;
    if constexpr (X0) {
        const int64_t tb = p.t[b];
        cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb];
    }
    for (int idx = threadIdx.x; idx < H * 16; idx += 256) {
        const int h = idx >> 4, j = idx & 15;
        const long long e = base + (long long)h * N + j;
        float v;
        if constexpr (X0) v = rst_x0(p.x[e], p.eps[e], cr, crm1);
        else v = src[e];
        S[h * SP + j] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    float* __restrict__ out = X0 ? p.tmp : dst;
    for (int m = wave; m < H / 16; m += 4) {
        const f32x4 acc = sep_tile(M + (size_t)m * 16 * H, H, S, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[base + (long long)(16 * m + 4 * g + r) * N + i] = acc[r];
    }
}

// Columns: 16 rows of one image per workgroup (grid: H / 16, B), channel by channel: S[k][n] = T[h0 + n][k][c], the tile is
// out[h0 + n][16 j + m][c].  FINISH: T = p.tmp and the tile goes into blur_finish (this is the step's last kernel: the counter and the
// chain's Philox key as rst_prologue); else buf is read and rewritten in place -- a channel's elements are all staged before any is
// written, and the other channels' are not touched.
template <bool FINISH>
__global__ __launch_bounds__(256) void sep_cols_kernel(const BlurStep p, float* __restrict__ buf, const float* __restrict__ M, uint64_t seed,
                                                       uint32_t stream, const int64_t* __restrict__ chain_state, int64_t* dec_counter) {
    __shared__ __attribute__((aligned(16))) float S[SEP_MAX * SP];
    if constexpr (FINISH) {
        if (dec_counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *dec_counter -= 1;
        if (chain_state) {
            seed = (uint64_t)chain_state[1];
            stream = (uint32_t)chain_state[2];
        }
    }
    const int H = p.H, W = p.W, C = p.C, h0 = blockIdx.x * 16, b = blockIdx.y;
    const float* __restrict__ T = FINISH ? p.tmp : buf;
    const long long base = ((long long)b * H + h0) * W * C;      // element (b, h0, 0, 0)
    int64_t tb = 0;
    float cr = 0.f, crm1 = 0.f, a1 = 0.f, a2 = 0.f, sg = 0.f;
    if constexpr (FINISH) {
        tb = p.t[b];
        cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb]; a1 = p.c1[tb]; a2 = p.c2[tb];
        sg = tb > 0 ? p.sigma[tb] : 0.0f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    for (int c = 0; c < C; ++c) {
        __syncthreads();          // the previous channel's tiles are done with S
        for (int idx = threadIdx.x; idx < 16 * W; idx += 256) {
            const int n = idx / W, k = idx - n * W;
            S[k * SP + n] = T[base + ((long long)n * W + k) * C + c];
        }
        __syncthreads();
        for (int j = wave; j < W / 16; j += 4) {
            const f32x4 acc = sep_tile(M + (size_t)j * 16 * W, W, S, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long e = base + ((long long)i * W + 16 * j + 4 * g + r) * C + c;
                if constexpr (FINISH) blur_finish(p, e, acc[r], tb, cr, crm1, a1, a2, sg, seed, stream);
                else buf[e] = acc[r];
            }
        }
    }
}

// The one-launch form: one workgroup per image (grid: B; 1024 threads) keeps X0 and T in LDS, both as [K][16] operands at pitch SP:
//   Xs[strip s][h][SP]                 the strips of X0, s < N / 16
//   Ts[row group m, channel c][w][SP]  T[16 m + n][w][c] at [w][n]
// 2 (H N / 16) SP floats = 10 H N bytes, the whole 160 KB at H N 4 = 64 KB.  P_h and P_w stream through sep_tile from L2.
__global__ __launch_bounds__(1024) void restore_blur_image_kernel(const BlurStep p, uint64_t seed, uint32_t stream,
                                                                  const int64_t* __restrict__ chain_state, int64_t* dec_counter) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    rst_prologue(dec_counter, chain_state, seed, stream);
    const int H = p.H, W = p.W, C = p.C, N = W * C, b = blockIdx.x;
    float* Xs = lds;
    float* Ts = lds + (size_t)(N / 16) * H * SP;
    const long long base = (long long)b * H * N;
    const int64_t tb = p.t[b];
    const float cr = p.c_recip[tb], crm1 = p.c_recipm1[tb], a1 = p.c1[tb], a2 = p.c2[tb], sg = tb > 0 ? p.sigma[tb] : 0.0f;
    for (int idx = threadIdx.x; idx < H * N; idx += 1024) {
        const int h = idx / N, n = idx - h * N;
        Xs[((n >> 4) * H + h) * SP + (n & 15)] = rst_x0(p.x[base + idx], p.eps[base + idx], cr, crm1);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4, mt = H / 16, wt = W / 16;
    for (int tt = wave; tt < (N / 16) * mt; tt += 16) {
        const int s = tt / mt, m = tt - s * mt;
        const f32x4 acc = sep_tile(p.ph + (size_t)m * 16 * H, H, Xs + (size_t)s * H * SP, lane);
        const int n = 16 * s + i, w = n / C, c = n - w * C;
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[((m * C + c) * W + w) * SP + 4 * g + r] = acc[r];
    }
    __syncthreads();
    for (int tt = wave; tt < mt * C * wt; tt += 16) {
        const int mc = tt / wt, j = tt - mc * wt, m = mc / C, c = mc - m * C;
        const f32x4 acc = sep_tile(p.pw + (size_t)j * 16 * W, W, Ts + (size_t)mc * W * SP, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long e = base + ((long long)(16 * m + i) * W + 16 * j + 4 * g + r) * C + c;
            blur_finish(p, e, acc[r], tb, cr, crm1, a1, a2, sg, seed, stream);
        }
    }
}

// ---------------------------------------------------------------------------------------------- the size-changing form (section 3.15)
// out = L . in . R^T with L [Ho][Hi] and R [Wo][Wi]: the same tile and the same [K][16] operand, for what the square form never meets.
// Every size is a multiple of 4, so a matrix row is still whole float4s; the rest is guarded here:
//   K not a multiple of 16   the last super-step's lanes with 16 s + 4 g >= K feed zeros on both sides, and read neither M nor S there
//   a partial last tile      lanes whose matrix row is past `rows` load nothing; the caller guards its stores in both tile coordinates
//   a partial strip / group  the caller stages zeros into S's columns past the end
// With K a multiple of 16 and whole tiles this is sep_tile's sum, term by term.
__device__ __forceinline__ f32x4 sep_tile_rect(const float* __restrict__ Mrows, int K, int rows, const float* S, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const bool row = i < rows;
    const float4* __restrict__ a = reinterpret_cast<const float4*>(Mrows + (size_t)(row ? i : 0) * K) + g;
    const float* b = S + 4 * g * SP + i;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < (K + 15) / 16; ++s) {
        const bool kin = 16 * s + 4 * g < K;
        const float4 av = row && kin ? a[4 * s] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* bs = b + 16 * s * SP;
        const float b0 = kin ? bs[0] : 0.f, b1 = kin ? bs[SP] : 0.f, b2 = kin ? bs[2 * SP] : 0.f, b3 = kin ? bs[3 * SP] : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

struct RectShape {
    int Hi, Wi, Ho, Wo, C;
};

// Rows: T[b][:, strip] = L . in[b][:, strip], in as the matrix [Hi][Wi C], T [Ho][Wi C] (grid: ceil(Wi C / 16), B)
__global__ __launch_bounds__(256) void sep_rows_rect_kernel(const RectShape p, const float* __restrict__ in, const float* __restrict__ M,
                                                            float* __restrict__ T) {
    __shared__ __attribute__((aligned(16))) float S[SEP_MAX * SP];
    const int Hi = p.Hi, Ho = p.Ho, N = p.Wi * p.C, n0 = blockIdx.x * 16, b = blockIdx.y;
    const int cols = min(16, N - n0);
    const float* __restrict__ src = in + (long long)b * Hi * N + n0;
    for (int idx = threadIdx.x; idx < Hi * 16; idx += 256) {
        const int h = idx >> 4, j = idx & 15;
        S[h * SP + j] = j < cols ? src[(long long)h * N + j] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    float* __restrict__ dst = T + (long long)b * Ho * N + n0;
    for (int m = wave; 16 * m < Ho; m += 4) {
        const f32x4 acc = sep_tile_rect(M + (size_t)m * 16 * Hi, Hi, Ho - 16 * m, S, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int h = 16 * m + 4 * g + r;
            if (h < Ho && i < cols) dst[(long long)h * N + i] = acc[r];
        }
    }
}

// Columns: 16 rows of one image's T per workgroup (grid: ceil(Ho / 16), B), channel by channel: S[k][n] = T[h0 + n][k][c], the tile is
// out[h0 + n][16 j + m][c]; out is another tensor than T ([Ho][Wo] against [Ho][Wi])
__global__ __launch_bounds__(256) void sep_cols_rect_kernel(const RectShape p, const float* __restrict__ T, const float* __restrict__ M,
                                                            float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float S[SEP_MAX * SP];
    const int Wi = p.Wi, Ho = p.Ho, Wo = p.Wo, C = p.C, h0 = blockIdx.x * 16, b = blockIdx.y;
    const int rows = min(16, Ho - h0);
    const float* __restrict__ src = T + ((long long)b * Ho + h0) * Wi * C;
    float* __restrict__ dst = out + ((long long)b * Ho + h0) * Wo * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    for (int c = 0; c < C; ++c) {
        __syncthreads();          // the previous channel's tiles are done with S
        for (int idx = threadIdx.x; idx < 16 * Wi; idx += 256) {
            const int n = idx / Wi, k = idx - n * Wi;
            S[k * SP + n] = n < rows ? src[((long long)n * Wi + k) * C + c] : 0.f;
        }
        __syncthreads();
        for (int j = wave; 16 * j < Wo; j += 4) {
            const f32x4 acc = sep_tile_rect(M + (size_t)j * 16 * Wi, Wi, Wo - 16 * j, S, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int w = 16 * j + 4 * g + r;
                if (i < rows && w < Wo) dst[((long long)i * Wo + w) * C + c] = acc[r];
            }
        }
    }
}

static size_t one_launch_lds(int H, int W, int C) { return (size_t)10 * H * W * C; }

bool restore_blur_shape_ok(int H, int W, int channels) {
    return H >= 16 && H <= SEP_MAX && H % 16 == 0 && W >= 16 && W <= SEP_MAX && W % 16 == 0 && channels >= 1 && channels <= 8;
}

bool restore_blur_one_launch(int H, int W, int channels) { return one_launch_lds(H, W, channels) <= 160 * 1024; }

int separable_init_device() {
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&restore_blur_image_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return DDK_OK;
}

static int separable_apply(const float* in, const float* L, const float* R, float* out, int B, int H, int W, int C, hipStream_t st) {
    BlurStep p{};
    p.H = H; p.W = W; p.C = C;
    hipLaunchKernelGGL(sep_rows_kernel<false>, dim3(W * C / 16, B), dim3(256), 0, st, p, in, L, out);
    DDK_TRY(check_launch("sep_rows_kernel"));
    hipLaunchKernelGGL(sep_cols_kernel<false>, dim3(H / 16, B), dim3(256), 0, st, p, out, R, (uint64_t)0, (uint32_t)0, (const int64_t*)nullptr,
                       (int64_t*)nullptr);
    return check_launch("sep_cols_kernel");
}

bool separable_rect_size_ok(int n) { return n >= 4 && n <= SEP_MAX && n % 4 == 0; }

static int separable_apply_rect(const float* in, const float* L, const float* R, float* out, float* scratch, int B, const RectShape& p,
                                hipStream_t st) {
    hipLaunchKernelGGL(sep_rows_rect_kernel, dim3((p.Wi * p.C + 15) / 16, B), dim3(256), 0, st, p, in, L, scratch);
    DDK_TRY(check_launch("sep_rows_rect_kernel"));
    hipLaunchKernelGGL(sep_cols_rect_kernel, dim3((p.Ho + 15) / 16, B), dim3(256), 0, st, p, (const float*)scratch, R, out);
    return check_launch("sep_cols_rect_kernel");
}

int p_update_restore_blur(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st) {
    const int H = r.rst.H, W = r.rst.W;
    BlurStep p{r.x, eps_hat, r.blr.ph, r.blr.pw, r.rst.y, r.blr.tmp, t, r.c_recip, r.c_recipm1, r.c1, r.c2, r.sigma, H, W, channels};
    DDK_TRY(ensure_device_init());
    if (restore_blur_one_launch(H, W, channels)) {
        hipLaunchKernelGGL(restore_blur_image_kernel, dim3(B), dim3(1024), one_launch_lds(H, W, channels), st, p, h.seed, h.stream_id,
                           h.chain_state, h.dec_counter);
        return check_launch("restore_blur_image_kernel");
    }
    hipLaunchKernelGGL(sep_rows_kernel<true>, dim3(W * channels / 16, B), dim3(256), 0, st, p, (const float*)nullptr, r.blr.ph, (float*)nullptr);
    DDK_TRY(check_launch("sep_rows_kernel"));
    hipLaunchKernelGGL(sep_cols_kernel<true>, dim3(H / 16, B), dim3(256), 0, st, p, (float*)nullptr, r.blr.pw, h.seed, h.stream_id, h.chain_state,
                       h.dec_counter);
    return check_launch("sep_cols_kernel");
}

}  // namespace ddk

using namespace ddk;

extern "C" {

int ddk_separable_apply(const float* in, const float* L, const float* R, float* out, int B, int H, int W, int channels, ddk_stream_t s) {
    DDK_REQUIRE(in && L && R && out, "separable_apply: null pointer");
    DDK_REQUIRE(B > 0 && B <= 65535 && restore_blur_shape_ok(H, W, channels),
                "separable_apply: H and W must be multiples of 16 in [16, 256], channels in 1..8, B in 1..65535");
    DDK_REQUIRE(aligned16(in) && aligned16(L) && aligned16(R) && aligned16(out), "separable_apply: alignment");
    return separable_apply(in, L, R, out, B, H, W, channels, as_stream(s));
}

int ddk_separable_apply_rect(const float* in, const float* L, const float* R, float* out, float* scratch, int B, int Hi, int Wi, int Ho, int Wo,
                             int channels, ddk_stream_t s) {
    DDK_REQUIRE(in && L && R && out && scratch, "separable_apply_rect: null pointer");
    DDK_REQUIRE(B > 0 && B <= 65535 && separable_rect_size_ok(Hi) && separable_rect_size_ok(Wi) && separable_rect_size_ok(Ho) &&
                    separable_rect_size_ok(Wo) && channels >= 1 && channels <= 8,
                "separable_apply_rect: Hi, Wi, Ho and Wo must be multiples of 4 in [4, 256], channels in 1..8, B in 1..65535");
    DDK_REQUIRE(aligned16(in) && aligned16(L) && aligned16(R) && aligned16(out) && aligned16(scratch), "separable_apply_rect: alignment");
    const size_t bc = (size_t)B * channels;
    const char *i0 = (const char*)in, *o0 = (const char*)out, *t0 = (const char*)scratch;
    const size_t ni = bc * Hi * Wi * sizeof(float), no = bc * Ho * Wo * sizeof(float), nt = bc * Ho * Wi * sizeof(float);
    auto overlap = [](const char* a, size_t na, const char* b, size_t nb) { return a < b + nb && b < a + na; };
    DDK_REQUIRE(!overlap(o0, no, i0, ni) && !overlap(o0, no, t0, nt) && !overlap(t0, nt, i0, ni),
                "separable_apply_rect: in, scratch and out must not overlap (the two products have different shapes: nothing runs in place)");
    return separable_apply_rect(in, L, R, out, scratch, B, RectShape{Hi, Wi, Ho, Wo, channels}, as_stream(s));
}

int ddk_p_sample_update_restore_blur(float* x, const float* eps_hat, const float* P_h, const float* P_w, const float* Yp, float* scratch,
                                     const int64_t* t, const float* c_recip, const float* c_recipm1, const float* c1, const float* c2,
                                     const float* sigma, int B, int H, int W, int channels, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && channels > 0, "p_sample_update_restore_blur: B / H / W / channels must be positive");
    StepRule r{StepKind::RestoreBlur, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, sigma};
    r.blr = BlurOps{P_h, P_w, scratch, nullptr, nullptr};
    r.rst = RestoreOps{Yp, 0, H, W, 0, nullptr};
    return p_update(r, eps_hat, t, B, (long long)H * W * channels, ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s),
                    "p_sample_update_restore_blur");
}

}  // extern "C"
