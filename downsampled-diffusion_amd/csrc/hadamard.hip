// hadamard.hip -- the subsampled, permuted Walsh-Hadamard operator of DDNM's compressed-sensing task and the restore step built on it
// (DESIGN.md section 3.17).
//
// Per channel of an NHWC image, the plane flattened row-major (j = h W + w, N = H W a power of two):
//   a[j] = X[perm[j]],   v = s H a,  s = 1 / sqrt(N),  H the Sylvester matrix (H[k][j] = (-1)^popcount(k & j)),   A(X) = v[0 .. m - 1]
// A has orthonormal rows, so A+ = A^T.  The step: x0 (clipped, from x and eps_hat, never through memory) is gathered through perm,
// transformed, its first m coefficients are replaced by y (a select), it is transformed back and scattered into Restore's finish.
//
// One routine, fwht_bits, runs the butterflies of a range of index bits over an array in LDS: radix-4 passes (two bits each, one
// barrier each), the lowest two bits as one 16-byte access per thread, a radix-2 pass for an odd bit.  The order is fixed, there are no
// atomics: results are bit-identical run to run and between eager launches and graph replay.  A 4-byte LDS access is served in groups
// of 32 lanes over 32 banks: passes over bits 6 and up touch consecutive floats (no conflict), the pass over bits 2, 3 puts a group on
// 8 banks (4-way) and the pass over bits 4, 5 on 16 (2-way) (section 3.17, what remains).
//
// Plane form (N <= 32768, at most 128 KB of LDS): one workgroup per (image, channel) does the whole step in one launch.
// Scratch form (N = 65536): H_N = H_hi (x) H_lo with 256 x 256 factors, whose stages commute:
//   cs_low_in    gather, bits 0..7 over contiguous runs of 256                      -> T
//   cs_high      bits 8..15 of 16 columns, scale, select, bits 8..15 again          T -> T (in place: a workgroup owns its columns)
//   cs_low_out   bits 0..7, scale, scatter into the finish                          T -> x
//
// Every kernel reads perm[j] & (N - 1): a bad array gives wrong numbers, never an access outside the plane.
// Compiled with -ffp-contract=off (Makefile): the step's elementwise arithmetic rounds every operation like diffusion.hip's.
#include "ddk_internal.h"
#include "diffusion_step.h"

#include <cmath>

namespace ddk {

constexpr int CS_PLANE_MAX = 32768;      // floats of a plane the one-launch form holds in LDS (128 KB of the CU's 160 KB)
constexpr int CS_LO_BITS = 8;            // scratch form: N = 2^16 = 2^8 (high) x 2^8 (low)
constexpr int CS_RUN = 4096;             // scratch form: floats per workgroup (16 runs of 256, or 16 columns of 256)

// the index whose bits below `s` are q's and whose two bits at s, s + 1 are zero
__device__ __forceinline__ int cs_spread2(int q, int s) { return ((q >> s) << (s + 2)) | (q & ((1 << s) - 1)); }
__device__ __forceinline__ int cs_spread1(int q, int s) { return ((q >> s) << (s + 1)) | (q & ((1 << s) - 1)); }

__device__ __forceinline__ void cs_bfly4(float& a0, float& a1, float& a2, float& a3) {
    const float t0 = a0 + a1, t1 = a0 - a1, t2 = a2 + a3, t3 = a2 - a3;
    a0 = t0 + t2; a1 = t1 + t3; a2 = t0 - t2; a3 = t1 - t3;
}

// The unnormalised butterflies over bits [lo, hi) of the index of S[0 .. n), n a multiple of 4, by the workgroup's nt threads.  The
// caller's data must be visible (a barrier behind its stores); this returns behind a barrier.
__device__ __forceinline__ void fwht_bits(float* S, int n, int lo, int hi, int tid, int nt) {
    int s = lo;
    if (s == 0 && hi >= 2) {
        for (int q = tid; q < n / 4; q += nt) {
            float4 v = reinterpret_cast<float4*>(S)[q];
            cs_bfly4(v.x, v.y, v.z, v.w);
            reinterpret_cast<float4*>(S)[q] = v;
        }
        __syncthreads();
        s = 2;
    }
    for (; s + 2 <= hi; s += 2) {
        const int d = 1 << s;
        for (int q = tid; q < n / 4; q += nt) {
            const int i = cs_spread2(q, s);
            float a0 = S[i], a1 = S[i + d], a2 = S[i + 2 * d], a3 = S[i + 3 * d];
            cs_bfly4(a0, a1, a2, a3);
            S[i] = a0; S[i + d] = a1; S[i + 2 * d] = a2; S[i + 3 * d] = a3;
        }
        __syncthreads();
    }
    if (s < hi) {
        const int d = 1 << s;
        for (int q = tid; q < n / 2; q += nt) {
            const int i = cs_spread1(q, s);
            const float a0 = S[i], a1 = S[i + d];
            S[i] = a0 + a1; S[i + d] = a0 - a1;
        }
        __syncthreads();
    }
}

// one step's, or one lone transform's, operands (by value into the kernels; the chain's StepRule never grows for them)
struct CsStep {
    float* x;                     // [B][H][W][C]: the step's x, updated in place; measure: the image (read); adjoint: the output
    const float* eps;             // eps_hat, x's layout (step only)
    const float* y;               // [B][C][m] (step, adjoint)
    float* yout;                  // [B][C][m] (measure)
    const int* perm;              // [N]
    float* tmp;                   // T [B][C][N], scratch form only
    const int64_t* t;
    const float *c_recip, *c_recipm1, *c1, *c2, *sigma;
    int N, logn, C, m;
    float s;                      // fp32(1 / sqrt(N))
};

enum class CsMode { Step, Measure, Adjoint };

// the element's update once x0' is known: Restore's finish with the Ancestral kind's Philox keying
__device__ __forceinline__ void cs_finish(const CsStep& p, long long e, float x0p, int64_t tb, float a1, float a2, float sg, uint64_t seed,
                                          uint32_t stream) {
    const float xv = p.x[e];
    float z = comp4(philox_normal4((unsigned long long)(e >> 2), (uint32_t)tb, stream, seed), (int)(e & 3));
    p.x[e] = rst_finish<StepKind::RestoreHadamard>(xv, x0p, 1.0f, z, a1, a2, sg, 0.0f);
}

// Plane form: workgroup (b, c) = blockIdx.x holds the plane in LDS.
template <CsMode M>
__global__ __launch_bounds__(1024) void cs_plane_kernel(const CsStep p, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state,
                                                        int64_t* dec_counter) {
    extern __shared__ __attribute__((aligned(16))) float S[];
    if constexpr (M == CsMode::Step) rst_prologue(dec_counter, chain_state, seed, stream);
    const int N = p.N, C = p.C, m = p.m, tid = threadIdx.x, nt = blockDim.x;
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const long long base = (long long)b * N * C + c;             // element (b, pixel 0, c); pixel j at base + j C
    const long long ybase = (long long)blockIdx.x * m;
    int64_t tb = 0;
    float cr = 0.f, crm1 = 0.f, a1 = 0.f, a2 = 0.f, sg = 0.f;
    if constexpr (M == CsMode::Step) {
        tb = p.t[b];
        cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb]; a1 = p.c1[tb]; a2 = p.c2[tb];
        sg = tb > 0 ? p.sigma[tb] : 0.0f;
    }
    if constexpr (M != CsMode::Adjoint) {
        for (int j = tid; j < N; j += nt) {
            const long long e = base + (long long)(p.perm[j] & (N - 1)) * C;
            if constexpr (M == CsMode::Step) S[j] = rst_x0(p.x[e], p.eps[e], cr, crm1);
            else S[j] = p.x[e];
        }
        __syncthreads();
        fwht_bits(S, N, 0, p.logn, tid, nt);
    }
    if constexpr (M == CsMode::Measure) {
        for (int k = tid; k < m; k += nt) p.yout[ybase + k] = __fmul_rn(p.s, S[k]);
        return;
    }
    for (int k = tid; k < N; k += nt) {
        float w;
        if constexpr (M == CsMode::Step) w = k < m ? p.y[ybase + k] : __fmul_rn(p.s, S[k]);
        else w = k < m ? p.y[ybase + k] : 0.0f;
        S[k] = w;
    }
    __syncthreads();
    fwht_bits(S, N, 0, p.logn, tid, nt);
    for (int j = tid; j < N; j += nt) {
        const long long e = base + (long long)(p.perm[j] & (N - 1)) * C;
        const float v = __fmul_rn(p.s, S[j]);
        if constexpr (M == CsMode::Step) cs_finish(p, e, v, tb, a1, a2, sg, seed, stream);
        else p.x[e] = v;
    }
}

// Scratch form, launch 1 (grid: N / CS_RUN, B C): T[plane][j] for j in this workgroup's 4096, the low bits done.
template <bool X0>
__global__ __launch_bounds__(1024) void cs_low_in_kernel(const CsStep p) {
    __shared__ __attribute__((aligned(16))) float S[CS_RUN];
    const int N = p.N, C = p.C, tid = threadIdx.x, j0 = blockIdx.x * CS_RUN;
    const int b = blockIdx.y / C, c = blockIdx.y - b * C;
    const long long base = (long long)b * N * C + c;
    float cr = 0.f, crm1 = 0.f;
    if constexpr (X0) {
        const int64_t tb = p.t[b];
        cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb];
    }
    for (int i = tid; i < CS_RUN; i += 1024) {
        const long long e = base + (long long)(p.perm[j0 + i] & (N - 1)) * C;
        if constexpr (X0) S[i] = rst_x0(p.x[e], p.eps[e], cr, crm1);
        else S[i] = p.x[e];
    }
    __syncthreads();
    fwht_bits(S, CS_RUN, 0, CS_LO_BITS, tid, 1024);
    float* __restrict__ T = p.tmp + (long long)blockIdx.y * N + j0;
    for (int i = tid; i < CS_RUN; i += 1024) T[i] = S[i];
}

// Scratch form, launch 2 (grid: 256 / 16, B C): 16 columns jl of the [jh][jl] view of a plane, S[jh][16]: the high bits are bits
// 4..11 of the LDS index.  Step: T -> v -> select -> high bits again -> T.  Measure: T -> y.  Adjoint: y / 0 -> T.
template <CsMode M>
__global__ __launch_bounds__(1024) void cs_high_kernel(const CsStep p) {
    __shared__ __attribute__((aligned(16))) float S[CS_RUN];
    const int N = p.N, m = p.m, tid = threadIdx.x, l0 = blockIdx.x * 16;
    float* __restrict__ T = p.tmp + (long long)blockIdx.y * N;
    const long long ybase = (long long)blockIdx.y * m;
    if constexpr (M != CsMode::Adjoint) {
        for (int i = tid; i < CS_RUN; i += 1024) S[i] = T[((i >> 4) << CS_LO_BITS) + l0 + (i & 15)];
        __syncthreads();
        fwht_bits(S, CS_RUN, 4, 4 + 16 - CS_LO_BITS, tid, 1024);
    }
    for (int i = tid; i < CS_RUN; i += 1024) {
        const int k = ((i >> 4) << CS_LO_BITS) + l0 + (i & 15);
        if constexpr (M == CsMode::Measure) {
            if (k < m) p.yout[ybase + k] = __fmul_rn(p.s, S[i]);
        } else if constexpr (M == CsMode::Step) {
            S[i] = k < m ? p.y[ybase + k] : __fmul_rn(p.s, S[i]);
        } else {
            S[i] = k < m ? p.y[ybase + k] : 0.0f;
        }
    }
    if constexpr (M == CsMode::Measure) return;
    __syncthreads();
    fwht_bits(S, CS_RUN, 4, 4 + 16 - CS_LO_BITS, tid, 1024);
    for (int i = tid; i < CS_RUN; i += 1024) T[((i >> 4) << CS_LO_BITS) + l0 + (i & 15)] = S[i];
}

// Scratch form, launch 3 (grid: (N / CS_RUN) B C, one-dimensional: the step's last kernel, rst_prologue's workgroup 0 decrements)
template <bool FINISH>
__global__ __launch_bounds__(1024) void cs_low_out_kernel(const CsStep p, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state,
                                                          int64_t* dec_counter) {
    __shared__ __attribute__((aligned(16))) float S[CS_RUN];
    if constexpr (FINISH) rst_prologue(dec_counter, chain_state, seed, stream);
    const int N = p.N, C = p.C, tid = threadIdx.x, runs = N / CS_RUN;
    const int plane = blockIdx.x / runs, j0 = (blockIdx.x - plane * runs) * CS_RUN;
    const int b = plane / C, c = plane - b * C;
    const long long base = (long long)b * N * C + c;
    int64_t tb = 0;
    float a1 = 0.f, a2 = 0.f, sg = 0.f;
    if constexpr (FINISH) {
        tb = p.t[b];
        a1 = p.c1[tb]; a2 = p.c2[tb];
        sg = tb > 0 ? p.sigma[tb] : 0.0f;
    }
    const float* __restrict__ T = p.tmp + (long long)plane * N + j0;
    for (int i = tid; i < CS_RUN; i += 1024) S[i] = T[i];
    __syncthreads();
    fwht_bits(S, CS_RUN, 0, CS_LO_BITS, tid, 1024);
    for (int i = tid; i < CS_RUN; i += 1024) {
        const long long e = base + (long long)(p.perm[j0 + i] & (N - 1)) * C;
        const float v = __fmul_rn(p.s, S[i]);
        if constexpr (FINISH) cs_finish(p, e, v, tb, a1, a2, sg, seed, stream);
        else p.x[e] = v;
    }
}

static int ilog2(long long n) {
    int l = 0;
    while ((1ll << l) < n) ++l;
    return l;
}
static bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

bool restore_cs_shape_ok(int H, int W, int channels) { return pow2_in(H, 16, 256) && pow2_in(W, 16, 256) && channels >= 1 && channels <= 8; }
bool restore_cs_rows_ok(int H, int W, int m) { return m >= 4 && m % 4 == 0 && (long long)m <= (long long)H * W; }
bool restore_cs_plane_form(int H, int W) { return (long long)H * W <= CS_PLANE_MAX; }

int hadamard_init_device() {
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cs_plane_kernel<CsMode::Step>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CS_PLANE_MAX * 4));
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cs_plane_kernel<CsMode::Measure>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CS_PLANE_MAX * 4));
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cs_plane_kernel<CsMode::Adjoint>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CS_PLANE_MAX * 4));
    return DDK_OK;
}

static CsStep cs_shape(int H, int W, int C, int m, const int* perm, float* tmp) {
    CsStep p{};
    p.N = H * W; p.logn = ilog2(p.N); p.C = C; p.m = m; p.perm = perm; p.tmp = tmp;
    p.s = (float)(1.0 / std::sqrt((double)p.N));
    return p;
}
static unsigned cs_plane_threads(int N) { return (unsigned)(N / 4 < 64 ? 64 : N / 4 > 1024 ? 1024 : N / 4); }

// the three entries behind the C ABI: shapes and pointers are the caller's to have checked
template <CsMode M>
static int cs_run(const CsStep& p, int B, bool plane, const ChainHooks& h, hipStream_t st) {
    const int N = p.N, C = p.C;
    DDK_TRY(ensure_device_init());
    if (plane) {
        hipLaunchKernelGGL(cs_plane_kernel<M>, dim3(B * C), dim3(cs_plane_threads(N)), (size_t)N * sizeof(float), st, p, h.seed, h.stream_id,
                           h.chain_state, h.dec_counter);
        return check_launch("cs_plane_kernel");
    }
    if constexpr (M != CsMode::Adjoint) {
        hipLaunchKernelGGL(cs_low_in_kernel<M == CsMode::Step>, dim3(N / CS_RUN, B * C), dim3(1024), 0, st, p);
        DDK_TRY(check_launch("cs_low_in_kernel"));
    }
    hipLaunchKernelGGL(cs_high_kernel<M>, dim3((1 << CS_LO_BITS) / 16, B * C), dim3(1024), 0, st, p);
    DDK_TRY(check_launch("cs_high_kernel"));
    if constexpr (M != CsMode::Measure) {
        hipLaunchKernelGGL(cs_low_out_kernel<M == CsMode::Step>, dim3((N / CS_RUN) * B * C), dim3(1024), 0, st, p, h.seed, h.stream_id,
                           h.chain_state, h.dec_counter);
        DDK_TRY(check_launch("cs_low_out_kernel"));
    }
    return DDK_OK;
}

int p_update_restore_cs(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st) {
    CsStep p = cs_shape(r.rst.H, r.rst.W, channels, r.had.m, r.had.perm, r.had.tmp);
    p.x = r.x; p.eps = eps_hat; p.y = r.rst.y; p.t = t;
    p.c_recip = r.c_recip; p.c_recipm1 = r.c_recipm1; p.c1 = r.c1; p.c2 = r.c2; p.sigma = r.sigma;
    return cs_run<CsMode::Step>(p, B, restore_cs_plane_form(r.rst.H, r.rst.W), h, st);
}

// what the two lone transforms ask beyond their tensors: null when sound
static const char* cs_op_fault(const void* img, const void* y, const int* perm, const float* scratch, int B, int H, int W, int C, int m) {
    if (!(img && y && perm)) return "null pointer";
    if (!(B > 0 && (long long)B * C <= 65535 && restore_cs_shape_ok(H, W, C))) return "H and W must be powers of two in [16, 256], channels in 1..8, B channels <= 65535";
    if (!restore_cs_rows_ok(H, W, m)) return "m must be a multiple of 4 in [4, H W]";
    if (!restore_cs_plane_form(H, W) && !scratch) return "a 256 x 256 plane needs the scratch";
    if (!(aligned16(img) && aligned16(y) && aligned16(perm) && aligned16(scratch))) return "alignment";
    return nullptr;
}

}  // namespace ddk

using namespace ddk;

extern "C" {

int ddk_hadamard_measure(const float* x, const int32_t* perm, float* y, float* scratch, int B, int H, int W, int channels, int m, ddk_stream_t s) {
    if (const char* fault = cs_op_fault(x, y, perm, scratch, B, H, W, channels, m)) {
        set_error("bad argument: hadamard_measure: %s", fault);
        return DDK_ERR_ARG;
    }
    CsStep p = cs_shape(H, W, channels, m, perm, scratch);
    p.x = const_cast<float*>(x); p.yout = y;
    return cs_run<CsMode::Measure>(p, B, restore_cs_plane_form(H, W), ChainHooks{}, as_stream(s));
}

int ddk_hadamard_adjoint(const float* y, const int32_t* perm, float* out, float* scratch, int B, int H, int W, int channels, int m, ddk_stream_t s) {
    if (const char* fault = cs_op_fault(out, y, perm, scratch, B, H, W, channels, m)) {
        set_error("bad argument: hadamard_adjoint: %s", fault);
        return DDK_ERR_ARG;
    }
    CsStep p = cs_shape(H, W, channels, m, perm, scratch);
    p.x = out; p.y = y;
    return cs_run<CsMode::Adjoint>(p, B, restore_cs_plane_form(H, W), ChainHooks{}, as_stream(s));
}

int ddk_p_sample_update_restore_cs(float* x, const float* eps_hat, const float* y, const int32_t* perm, float* scratch, const int64_t* t,
                                   const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* sigma, int B, int H,
                                   int W, int channels, int m, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && channels > 0, "p_sample_update_restore_cs: B / H / W / channels must be positive");
    StepRule r{StepKind::RestoreHadamard, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, sigma};
    r.had = HadamardOps{perm, scratch, m};
    r.rst = RestoreOps{y, 0, H, W, 0, nullptr};
    return p_update(r, eps_hat, t, B, (long long)H * W * channels, ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s),
                    "p_sample_update_restore_cs");
}

}  // extern "C"
