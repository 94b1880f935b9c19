// fft_conv.hip -- circular convolution with a 2-D point-spread function through a complex FFT in LDS, and the DDNM restore step built
// on it.
//
// Per channel of an NHWC image, the plane X [H][W] (H, W powers of two, N = H W), F2 the unnormalised 2-D DFT:
//   apply:  out = Re F2^-1(S . F2(X)) / N            for a complex fp32 multiplier S [H][W] (A: S = K^, A+: S = P^)
//   step:   x0' = Re F2^-1(M ? 0 : F2(x0)) / N + Yp  with x0 the clipped x0 (from x and eps_hat, never through memory), M the kept
//           frequencies (a select), Yp = A+ y; then Restore's finish.
//
// One routine, fft_bits, runs the butterflies of a range of index bits over a complex array in LDS (float2, re and im side by side):
// forward as decimation in frequency (natural in, bit-reversed out), inverse as decimation in time with the conjugate twiddles
// (bit-reversed in, natural out), so no reordering pass exists.  A pass does two radix-2 stages in registers (a radix-4 butterfly with
// radix-2's arithmetic: every value is rounded as often as in a radix-2 transform) behind one barrier; an odd bit takes a radix-2
// pass.  The spectrum therefore sits at (brev(u), brev(v)); the select / multiply walks the frequencies in natural order, so mask and
// multiplier are read as the caller gave them, and addresses LDS through the reversed bits.  Twiddles exp(-2 pi i j / Lmax),
// j < Lmax / 2, Lmax = max(H, W), come from the caller's table (float64 on the host, rounded to fp32) and are copied into LDS.
// The order is fixed, there are no atomics: results are bit-identical run to run and between eager launches and graph replay.
//
// Plane form (N <= 16384: the complex plane is at most 128 KB of LDS): one workgroup per (image, channel), one launch.
// Multi-launch form (N = 32768, 65536) through a complex scratch T [B][C][N]:
//   fc_rows_in    gather, row transforms of a run of 4096 pixels                                      -> T
//   fc_cols       a strip of 16 columns: column transforms, select / multiply, column transforms back  T -> T (in place)
//   fc_rows_out   row transforms back, scale, (+ Yp, finish)                                          T -> x / out
//
// The noisy step (the kernels named *_noisy further down) is the same step for a blurred image that carries
// noise: per frequency the spectrum of x0 moves towards that of A+ y by lam and the draw's spectrum is scaled by phi.  In the plane
// form x0 and the draw share one complex transform; in the multi-launch form the draw travels through a second scratch T2.
//
// Compiled with -ffp-contract=off (Makefile): every product and sum below rounds on its own.
#include "ddk_internal.h"
#include "diffusion_step.h"

namespace ddk {

constexpr int FC_PLANE_MAX = 16384;      // complex elements of a plane the one-launch form holds in LDS (128 KB of the CU's 160 KB)
constexpr int FC_RUN = 4096;             // multi-launch form: complex elements per workgroup (32 KB)
constexpr int FC_STRIP = 16;             // multi-launch form: columns per workgroup of fc_cols (16 x 256 = FC_RUN)
constexpr int FC_TW_MAX = 128;           // twiddles of the longest axis (256 / 2)

// the index whose bits below `s` are q's and whose two bits (one bit) at s are zero
__device__ __forceinline__ int fc_spread2(int q, int s) { return ((q >> s) << (s + 2)) | (q & ((1 << s) - 1)); }
__device__ __forceinline__ int fc_spread1(int q, int s) { return ((q >> s) << (s + 1)) | (q & ((1 << s) - 1)); }

__device__ __forceinline__ float2 fc_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 fc_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a w, or (INV) a conj(w)
template <bool INV>
__device__ __forceinline__ float2 fc_mul(float2 a, float2 w) {
    if constexpr (INV) return make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y);
    else return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// The unnormalised DFT (INV: its conjugate) over bits [lo, hi) of the index of S[0 .. n): for every setting of the other bits, the
// transform of length 2^(hi - lo) and stride 2^lo.  Forward: natural in, bit-reversed out; inverse: bit-reversed in, natural out.
// tw: exp(-2 pi i j / 2^logt), j < 2^(logt - 1), hi - lo <= logt.  The caller's data must be visible (a barrier behind its stores);
// this returns behind a barrier.
template <bool INV>
__device__ __forceinline__ void fft_bits(float2* S, int n, int lo, int hi, const float2* tw, int logt, int tid, int nt) {
    if constexpr (!INV) {
        int s = hi - 1;
        for (; s - 1 >= lo; s -= 2) {          // stages s and s - 1
            const int d = 1 << (s - 1), sh = logt - (s - lo + 1), kmask = (1 << (s - lo)) - 1;
            for (int q = tid; q < n / 4; q += nt) {
                const int i = fc_spread2(q, s - 1), k0 = (i >> lo) & kmask;
                const float2 a0 = S[i], a1 = S[i + d], a2 = S[i + 2 * d], a3 = S[i + 3 * d];
                const float2 b0 = fc_add(a0, a2), b2 = fc_mul<false>(fc_sub(a0, a2), tw[k0 << sh]);
                const float2 b1 = fc_add(a1, a3), b3 = fc_mul<false>(fc_sub(a1, a3), tw[(k0 + (d >> lo)) << sh]);
                const float2 w2 = tw[k0 << (sh + 1)];
                S[i] = fc_add(b0, b1); S[i + d] = fc_mul<false>(fc_sub(b0, b1), w2);
                S[i + 2 * d] = fc_add(b2, b3); S[i + 3 * d] = fc_mul<false>(fc_sub(b2, b3), w2);
            }
            __syncthreads();
        }
        if (s == lo) {
            const int d = 1 << s;              // the last stage's twiddle is 1
            for (int q = tid; q < n / 2; q += nt) {
                const int i = fc_spread1(q, s);
                const float2 a0 = S[i], a1 = S[i + d];
                S[i] = fc_add(a0, a1); S[i + d] = fc_sub(a0, a1);
            }
            __syncthreads();
        }
    } else {
        int s = lo;
        if ((hi - lo) & 1) {                   // the first stage's twiddle is 1
            const int d = 1 << s;
            for (int q = tid; q < n / 2; q += nt) {
                const int i = fc_spread1(q, s);
                const float2 a0 = S[i], a1 = S[i + d];
                S[i] = fc_add(a0, a1); S[i + d] = fc_sub(a0, a1);
            }
            __syncthreads();
            ++s;
        }
        for (; s + 2 <= hi; s += 2) {          // stages s and s + 1
            const int d = 1 << s, sh = logt - (s - lo + 1), kmask = (1 << (s - lo)) - 1;
            for (int q = tid; q < n / 4; q += nt) {
                const int i = fc_spread2(q, s), k0 = (i >> lo) & kmask;
                const float2 a0 = S[i], a1 = S[i + d], a2 = S[i + 2 * d], a3 = S[i + 3 * d];
                const float2 w1 = tw[k0 << sh];
                const float2 t1 = fc_mul<true>(a1, w1), t3 = fc_mul<true>(a3, w1);
                const float2 b0 = fc_add(a0, t1), b1 = fc_sub(a0, t1), b2 = fc_add(a2, t3), b3 = fc_sub(a2, t3);
                const float2 u2 = fc_mul<true>(b2, tw[k0 << (sh - 1)]), u3 = fc_mul<true>(b3, tw[(k0 + (d >> lo)) << (sh - 1)]);
                S[i] = fc_add(b0, u2); S[i + 2 * d] = fc_sub(b0, u2);
                S[i + d] = fc_add(b1, u3); S[i + 3 * d] = fc_sub(b1, u3);
            }
            __syncthreads();
        }
    }
}

// one step's, or one lone convolution's, operands (by value into the kernels; the chain's StepRule never grows for them)
struct FcStep {
    float* x;                     // [B][H][W][C]: the step's x, updated in place; apply: the output
    const float* in;              // apply: the input image (may be x)
    const float* eps;             // eps_hat, x's layout (step only)
    const float* yp;              // Yp = A+ y, x's layout (step only)
    const float* mask;            // [H][W], nonzero where the frequency is kept (step only)
    const float2* mul;            // [H][W] complex multiplier (apply only)
    const float2* tw;             // [max(H, W) / 2]
    float2* tmp;                  // T [B][C][N], multi-launch form only
    const int64_t* t;
    const float *c_recip, *c_recipm1, *c1, *c2, *sigma;
    int N, logw, logh, logt, C;
    float inv_n;                  // 1 / N, a power of two
};

enum class FcMode { Step, Apply, Spectrum };      // Spectrum: Apply's forward half, mul . F2(in) left in the transform's order (x: complex [B][C][N])

__device__ __forceinline__ void fc_load_tw(float2* TW, const FcStep& p, int tid, int nt) {
    for (int j = tid; j < (1 << (p.logt - 1)); j += nt) TW[j] = p.tw[j];
}
__device__ __forceinline__ int fc_brev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// the element's update once x0' is known: Restore's finish with the Ancestral kind's Philox keying
__device__ __forceinline__ void fc_finish(const FcStep& p, long long e, float x0p, int64_t tb, float a1, float a2, float sg, uint64_t seed,
                                          uint32_t stream) {
    const float xv = p.x[e];
    float z = comp4(philox_normal4((unsigned long long)(e >> 2), (uint32_t)tb, stream, seed), (int)(e & 3));
    p.x[e] = rst_finish<StepKind::RestoreFFT>(xv, x0p, 1.0f, z, a1, a2, sg, 0.0f);
}

// Plane form: workgroup (b, c) = blockIdx.x holds the complex plane in LDS.
template <FcMode M>
__global__ __launch_bounds__(1024) void fc_plane_kernel(const FcStep p, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state,
                                                        int64_t* dec_counter) {
    extern __shared__ __attribute__((aligned(16))) float2 S[];
    __shared__ float2 TW[FC_TW_MAX];
    if constexpr (M == FcMode::Step) rst_prologue(dec_counter, chain_state, seed, stream);
    const int N = p.N, C = p.C, tid = threadIdx.x, nt = blockDim.x, logw = p.logw, logn = p.logw + p.logh;
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const long long base = (long long)b * N * C + c;             // element (b, pixel 0, c); pixel j at base + j C
    int64_t tb = 0;
    float cr = 0.f, crm1 = 0.f, a1 = 0.f, a2 = 0.f, sg = 0.f;
    if constexpr (M == FcMode::Step) {
        tb = p.t[b];
        cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb]; a1 = p.c1[tb]; a2 = p.c2[tb];
        sg = tb > 0 ? p.sigma[tb] : 0.0f;
    }
    fc_load_tw(TW, p, tid, nt);
    for (int j = tid; j < N; j += nt) {
        const long long e = base + (long long)j * C;
        if constexpr (M == FcMode::Step) S[j] = make_float2(rst_x0(p.x[e], p.eps[e], cr, crm1), 0.0f);
        else S[j] = make_float2(p.in[e], 0.0f);
    }
    __syncthreads();
    fft_bits<false>(S, N, 0, logw, TW, p.logt, tid, nt);
    fft_bits<false>(S, N, logw, logn, TW, p.logt, tid, nt);
    for (int f = tid; f < N; f += nt) {                          // frequency (u, v) = f in natural order sits at (brev(u), brev(v))
        const int q = (fc_brev(f >> logw, p.logh) << logw) | fc_brev(f & ((1 << logw) - 1), logw);
        if constexpr (M == FcMode::Step) {
            if (p.mask[f] != 0.0f) S[q] = make_float2(0.0f, 0.0f);
        } else {
            S[q] = fc_mul<false>(S[q], p.mul[f]);
        }
    }
    __syncthreads();
    if constexpr (M == FcMode::Spectrum) {
        float2* __restrict__ out = reinterpret_cast<float2*>(p.x) + (long long)blockIdx.x * N;
        for (int j = tid; j < N; j += nt) out[j] = S[j];
        return;
    }
    fft_bits<true>(S, N, logw, logn, TW, p.logt, tid, nt);
    fft_bits<true>(S, N, 0, logw, TW, p.logt, tid, nt);
    for (int j = tid; j < N; j += nt) {
        const long long e = base + (long long)j * C;
        const float r = __fmul_rn(S[j].x, p.inv_n);
        if constexpr (M == FcMode::Step) fc_finish(p, e, __fadd_rn(r, p.yp[e]), tb, a1, a2, sg, seed, stream);
        else p.x[e] = r;
    }
}

// Multi-launch form, launch 1 (grid: N / FC_RUN, B C): the row transforms of this workgroup's 4096 pixels (whole rows) into T.
template <FcMode M>
__global__ __launch_bounds__(1024) void fc_rows_in_kernel(const FcStep p) {
    __shared__ __attribute__((aligned(16))) float2 S[FC_RUN];
    __shared__ float2 TW[FC_TW_MAX];
    const int N = p.N, C = p.C, tid = threadIdx.x, j0 = blockIdx.x * FC_RUN;
    const int b = blockIdx.y / C, c = blockIdx.y - b * C;
    const long long base = (long long)b * N * C + c;
    float cr = 0.f, crm1 = 0.f;
    if constexpr (M == FcMode::Step) {
        const int64_t tb = p.t[b];
        cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb];
    }
    fc_load_tw(TW, p, tid, 1024);
    for (int i = tid; i < FC_RUN; i += 1024) {
        const long long e = base + (long long)(j0 + i) * C;
        if constexpr (M == FcMode::Step) S[i] = make_float2(rst_x0(p.x[e], p.eps[e], cr, crm1), 0.0f);
        else S[i] = make_float2(p.in[e], 0.0f);
    }
    __syncthreads();
    fft_bits<false>(S, FC_RUN, 0, p.logw, TW, p.logt, tid, 1024);
    float2* __restrict__ T = p.tmp + (long long)blockIdx.y * N + j0;
    for (int i = tid; i < FC_RUN; i += 1024) T[i] = S[i];
}

// Multi-launch form, launch 2 (grid: W / FC_STRIP, B C): 16 columns of a plane, S[r][16]: the column index bits are bits 4 .. of the
// LDS index.  T's column c holds the row frequency brev(c).
template <FcMode M>
__global__ __launch_bounds__(1024) void fc_cols_kernel(const FcStep p) {
    __shared__ __attribute__((aligned(16))) float2 S[FC_RUN];
    __shared__ float2 TW[FC_TW_MAX];
    const int N = p.N, tid = threadIdx.x, c0 = blockIdx.x * FC_STRIP, logw = p.logw, logh = p.logh, n = FC_STRIP << logh;
    float2* __restrict__ T = p.tmp + (long long)blockIdx.y * N;
    fc_load_tw(TW, p, tid, 1024);
    for (int i = tid; i < n; i += 1024) S[i] = T[((i >> 4) << logw) + c0 + (i & 15)];
    __syncthreads();
    fft_bits<false>(S, n, 4, 4 + logh, TW, p.logt, tid, 1024);
    for (int i = tid; i < n; i += 1024) {                        // i = (u, column): the frequency (u, brev(c0 + column)) sits at row brev(u)
        const int u = i >> 4, cc = i & 15, q = (fc_brev(u, logh) << 4) | cc;
        const int f = (u << logw) | fc_brev(c0 + cc, logw);
        if constexpr (M == FcMode::Step) {
            if (p.mask[f] != 0.0f) S[q] = make_float2(0.0f, 0.0f);
        } else {
            S[q] = fc_mul<false>(S[q], p.mul[f]);
        }
    }
    __syncthreads();
    if constexpr (M == FcMode::Spectrum) {                       // T's own layout is the transform's order: row brev(u), column brev(v)
        float2* __restrict__ out = reinterpret_cast<float2*>(p.x) + (long long)blockIdx.y * N;
        for (int i = tid; i < n; i += 1024) out[((i >> 4) << logw) + c0 + (i & 15)] = S[i];
        return;
    }
    fft_bits<true>(S, n, 4, 4 + logh, TW, p.logt, tid, 1024);
    for (int i = tid; i < n; i += 1024) T[((i >> 4) << logw) + c0 + (i & 15)] = S[i];
}

// Multi-launch form, launch 3 (grid: (N / FC_RUN) B C, one-dimensional: the step's last kernel, rst_prologue's workgroup 0 decrements)
template <FcMode M>
__global__ __launch_bounds__(1024) void fc_rows_out_kernel(const FcStep p, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state,
                                                           int64_t* dec_counter) {
    __shared__ __attribute__((aligned(16))) float2 S[FC_RUN];
    __shared__ float2 TW[FC_TW_MAX];
    if constexpr (M == FcMode::Step) rst_prologue(dec_counter, chain_state, seed, stream);
    const int N = p.N, C = p.C, tid = threadIdx.x, runs = N / FC_RUN;
    const int plane = blockIdx.x / runs, j0 = (blockIdx.x - plane * runs) * FC_RUN;
    const int b = plane / C, c = plane - b * C;
    const long long base = (long long)b * N * C + c;
    int64_t tb = 0;
    float a1 = 0.f, a2 = 0.f, sg = 0.f;
    if constexpr (M == FcMode::Step) {
        tb = p.t[b];
        a1 = p.c1[tb]; a2 = p.c2[tb];
        sg = tb > 0 ? p.sigma[tb] : 0.0f;
    }
    fc_load_tw(TW, p, tid, 1024);
    const float2* __restrict__ T = p.tmp + (long long)plane * N + j0;
    for (int i = tid; i < FC_RUN; i += 1024) S[i] = T[i];
    __syncthreads();
    fft_bits<true>(S, FC_RUN, 0, p.logw, TW, p.logt, tid, 1024);
    for (int i = tid; i < FC_RUN; i += 1024) {
        const long long e = base + (long long)(j0 + i) * C;
        const float r = __fmul_rn(S[i].x, p.inv_n);
        if constexpr (M == FcMode::Step) fc_finish(p, e, __fadd_rn(r, p.yp[e]), tb, a1, a2, sg, seed, stream);
        else p.x[e] = r;
    }
}

// ---- DDNM+ per frequency: the step for a blurred image with noise of standard deviation sigma_y ------------
// The Step operands (yp unused) and what the noisy step reads besides; by value into kernels of its own, so FcStep stays what it was.
struct FcNoisy {
    FcStep s;
    const float* gain;            // [H][W], natural frequency order: 1 / |K^| where kept, 0 elsewhere
    const float* nsc;             // per row: |c1| sigma_y
    const float2* yhat;           // the spectrum of A+ y, [B][C][N] in the transform's order (row brev(u), column brev(v))
    float2* tmp2;                 // T2 [B][C][N], the draw's transform; multi-launch form only
};

// the frequency's two multipliers from the row's s (the draw's scale, 0 at row 0) and g = nsc gain: every operation rounds on its own
__device__ __forceinline__ void fc_noisy_mult(bool kept, float s, float ns, float gain, float& lam, float& phi) {
    if (!kept) { lam = 0.0f; phi = s; return; }
    const float g = __fmul_rn(ns, gain);
    if (s >= g) {
        lam = 1.0f;
        phi = __fsqrt_rn(fmaxf(__fsub_rn(__fmul_rn(s, s), __fmul_rn(g, g)), 0.0f));
    } else {
        lam = __fdiv_rn(s, g);
        phi = 0.0f;
    }
}
// the element's draw, keyed exactly as fc_finish's (none at row 0)
__device__ __forceinline__ float fc_draw(long long e, int64_t tb, uint64_t seed, uint32_t stream) {
    if (tb <= 0) return 0.0f;
    return comp4(philox_normal4((unsigned long long)(e >> 2), (uint32_t)tb, stream, seed), (int)(e & 3));
}
__device__ __forceinline__ float fc_noisy_finish(float xv, float x0p, float n, float a1, float a2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a1, x0p), __fmul_rn(a2, xv)), n);
}

// Plane form: fc_plane_kernel's launch (same LDS, same threads) with x0 + i z in the one complex transform.  Both are real, so at the
// select the thread that owns the pair {f, -f} separates X^(f) = (C^(f) + conj C^(-f)) / 2 and Z^(f) = (C^(f) - conj C^(-f)) / (2 i),
// applies the real, even lam and phi and writes X^' + i Z^' back at both places: the inverse transform then carries x0' in the real
// part and the shaped draw n in the imaginary part.
__global__ __launch_bounds__(1024) void fc_plane_noisy_kernel(const FcNoisy pn, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state,
                                                              int64_t* dec_counter) {
    extern __shared__ __attribute__((aligned(16))) float2 S[];
    __shared__ float2 TW[FC_TW_MAX];
    rst_prologue(dec_counter, chain_state, seed, stream);
    const FcStep& p = pn.s;
    const int N = p.N, C = p.C, tid = threadIdx.x, nt = blockDim.x, logw = p.logw, logh = p.logh, logn = p.logw + p.logh;
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const long long base = (long long)b * N * C + c;
    const int64_t tb = p.t[b];
    const float cr = p.c_recip[tb], crm1 = p.c_recipm1[tb], a1 = p.c1[tb], a2 = p.c2[tb], sg = tb > 0 ? p.sigma[tb] : 0.0f, ns = pn.nsc[tb];
    fc_load_tw(TW, p, tid, nt);
    for (int j = tid; j < N; j += nt) {
        const long long e = base + (long long)j * C;
        S[j] = make_float2(rst_x0(p.x[e], p.eps[e], cr, crm1), fc_draw(e, tb, seed, stream));
    }
    __syncthreads();
    fft_bits<false>(S, N, 0, logw, TW, p.logt, tid, nt);
    fft_bits<false>(S, N, logw, logn, TW, p.logt, tid, nt);
    const float2* __restrict__ Yh = pn.yhat + (long long)blockIdx.x * N;
    const int wm = (1 << logw) - 1, hm = (1 << logh) - 1;
    for (int f = tid; f < N; f += nt) {                          // the pair's lower natural index does the work
        const int u = f >> logw, v = f & wm, fn = ((-u & hm) << logw) | (-v & wm);
        if (fn < f) continue;
        const int q = (fc_brev(u, logh) << logw) | fc_brev(v, logw), qn = (fc_brev(fn >> logw, logh) << logw) | fc_brev(fn & wm, logw);
        const bool kept = p.mask[f] != 0.0f;
        float lam, phi;
        fc_noisy_mult(kept, sg, ns, pn.gain[f], lam, phi);
        const float2 a = S[q], m = S[qn];
        float2 X = make_float2(0.5f * (a.x + m.x), 0.5f * (a.y - m.y));
        const float2 Z = make_float2(phi * (0.5f * (a.y + m.y)), phi * (0.5f * (m.x - a.x)));
        if (kept) {                                              // a select: a dropped frequency's spectrum of A+ y is never read
            const float2 y0 = Yh[q], y1 = Yh[qn];                // (Y^(f) + conj Y^(-f)) / 2: what the real part behind the inverse keeps of it
            const float2 Y = make_float2(0.5f * (y0.x + y1.x), 0.5f * (y0.y - y1.y));
            X = make_float2(X.x + lam * (Y.x - X.x), X.y + lam * (Y.y - X.y));
        }
        S[q] = make_float2(X.x - Z.y, X.y + Z.x);
        if (fn != f) S[qn] = make_float2(X.x + Z.y, Z.x - X.y);
    }
    __syncthreads();
    fft_bits<true>(S, N, logw, logn, TW, p.logt, tid, nt);
    fft_bits<true>(S, N, 0, logw, TW, p.logt, tid, nt);
    for (int j = tid; j < N; j += nt) {
        const long long e = base + (long long)j * C;
        const float2 r = S[j];
        p.x[e] = fc_noisy_finish(p.x[e], __fmul_rn(r.x, p.inv_n), __fmul_rn(r.y, p.inv_n), a1, a2);
    }
}

// Multi-launch form: the three launches of the deconvolution step with the draw travelling through T2 beside x0 in T.  A strip of
// fc_cols holds 16 columns and the partner column -v lies in another strip, so the two real signals are not packed here.
// Launch 1 (grid: N / FC_RUN, B C): the row transforms of x0 into T, then of the draw into T2, one after the other on the same LDS.
__global__ __launch_bounds__(1024) void fc_rows_in_noisy_kernel(const FcNoisy pn, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state) {
    __shared__ __attribute__((aligned(16))) float2 S[FC_RUN];
    __shared__ float2 TW[FC_TW_MAX];
    rst_prologue(nullptr, chain_state, seed, stream);
    const FcStep& p = pn.s;
    const int N = p.N, C = p.C, tid = threadIdx.x, j0 = blockIdx.x * FC_RUN;
    const int b = blockIdx.y / C, c = blockIdx.y - b * C;
    const long long base = (long long)b * N * C + c;
    const int64_t tb = p.t[b];
    const float cr = p.c_recip[tb], crm1 = p.c_recipm1[tb];
    fc_load_tw(TW, p, tid, 1024);
    for (int i = tid; i < FC_RUN; i += 1024) {
        const long long e = base + (long long)(j0 + i) * C;
        S[i] = make_float2(rst_x0(p.x[e], p.eps[e], cr, crm1), 0.0f);
    }
    __syncthreads();
    fft_bits<false>(S, FC_RUN, 0, p.logw, TW, p.logt, tid, 1024);
    float2* __restrict__ T = p.tmp + (long long)blockIdx.y * N + j0;
    for (int i = tid; i < FC_RUN; i += 1024) {
        T[i] = S[i];
        S[i] = make_float2(fc_draw(base + (long long)(j0 + i) * C, tb, seed, stream), 0.0f);      // this thread's own elements: no barrier between
    }
    __syncthreads();
    fft_bits<false>(S, FC_RUN, 0, p.logw, TW, p.logt, tid, 1024);
    float2* __restrict__ T2 = pn.tmp2 + (long long)blockIdx.y * N + j0;
    for (int i = tid; i < FC_RUN; i += 1024) T2[i] = S[i];
}

// Launch 2 (grid: W / FC_STRIP, B C, 2): fc_cols on T with X^' = X^ + lam (Y^ - X^) (z = 0), and on T2 with Z^' = phi Z^ (z = 1)
__global__ __launch_bounds__(1024) void fc_cols_noisy_kernel(const FcNoisy pn) {
    __shared__ __attribute__((aligned(16))) float2 S[FC_RUN];
    __shared__ float2 TW[FC_TW_MAX];
    const FcStep& p = pn.s;
    const int N = p.N, tid = threadIdx.x, c0 = blockIdx.x * FC_STRIP, logw = p.logw, logh = p.logh, n = FC_STRIP << logh;
    const bool draw = blockIdx.z != 0;
    float2* __restrict__ T = (draw ? pn.tmp2 : p.tmp) + (long long)blockIdx.y * N;
    const float2* __restrict__ Yh = pn.yhat + (long long)blockIdx.y * N;
    const int64_t tb = p.t[blockIdx.y / p.C];
    const float sg = tb > 0 ? p.sigma[tb] : 0.0f, ns = pn.nsc[tb];
    fc_load_tw(TW, p, tid, 1024);
    for (int i = tid; i < n; i += 1024) S[i] = T[((i >> 4) << logw) + c0 + (i & 15)];
    __syncthreads();
    fft_bits<false>(S, n, 4, 4 + logh, TW, p.logt, tid, 1024);
    for (int i = tid; i < n; i += 1024) {
        const int u = i >> 4, cc = i & 15, ru = fc_brev(u, logh), q = (ru << 4) | cc;
        const int f = (u << logw) | fc_brev(c0 + cc, logw);
        const bool kept = p.mask[f] != 0.0f;
        float lam, phi;
        fc_noisy_mult(kept, sg, ns, pn.gain[f], lam, phi);
        const float2 a = S[q];
        if (draw) {
            S[q] = make_float2(phi * a.x, phi * a.y);
        } else if (kept) {
            const float2 Y = Yh[(ru << logw) + c0 + cc];
            S[q] = make_float2(a.x + lam * (Y.x - a.x), a.y + lam * (Y.y - a.y));
        }
    }
    __syncthreads();
    fft_bits<true>(S, n, 4, 4 + logh, TW, p.logt, tid, 1024);
    for (int i = tid; i < n; i += 1024) T[((i >> 4) << logw) + c0 + (i & 15)] = S[i];
}

// Launch 3 (grid: (N / FC_RUN) B C, one-dimensional: the step's last kernel): the rows of T back, x0' kept in registers, then the
// rows of T2 back on the same LDS, and the finish
__global__ __launch_bounds__(1024) void fc_rows_out_noisy_kernel(const FcNoisy pn, uint64_t seed, uint32_t stream, const int64_t* __restrict__ chain_state,
                                                                 int64_t* dec_counter) {
    __shared__ __attribute__((aligned(16))) float2 S[FC_RUN];
    __shared__ float2 TW[FC_TW_MAX];
    rst_prologue(dec_counter, chain_state, seed, stream);
    const FcStep& p = pn.s;
    const int N = p.N, C = p.C, tid = threadIdx.x, runs = N / FC_RUN;
    const int plane = blockIdx.x / runs, j0 = (blockIdx.x - plane * runs) * FC_RUN;
    const int b = plane / C, c = plane - b * C;
    const long long base = (long long)b * N * C + c;
    const int64_t tb = p.t[b];
    const float a1 = p.c1[tb], a2 = p.c2[tb];
    fc_load_tw(TW, p, tid, 1024);
    const float2* __restrict__ T = p.tmp + (long long)plane * N + j0;
    const float2* __restrict__ T2 = pn.tmp2 + (long long)plane * N + j0;
    for (int i = tid; i < FC_RUN; i += 1024) S[i] = T[i];
    __syncthreads();
    fft_bits<true>(S, FC_RUN, 0, p.logw, TW, p.logt, tid, 1024);
    float x0p[FC_RUN / 1024];
#pragma unroll
    for (int k = 0; k < FC_RUN / 1024; ++k) {
        const int i = tid + k * 1024;
        x0p[k] = __fmul_rn(S[i].x, p.inv_n);
        S[i] = T2[i];                                            // this thread's own elements
    }
    __syncthreads();
    fft_bits<true>(S, FC_RUN, 0, p.logw, TW, p.logt, tid, 1024);
#pragma unroll
    for (int k = 0; k < FC_RUN / 1024; ++k) {
        const int i = tid + k * 1024;
        const long long e = base + (long long)(j0 + i) * C;
        p.x[e] = fc_noisy_finish(p.x[e], x0p[k], __fmul_rn(S[i].x, p.inv_n), a1, a2);
    }
}

static int ilog2(long long n) {
    int l = 0;
    while ((1ll << l) < n) ++l;
    return l;
}
static bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

bool restore_fft_shape_ok(int H, int W, int channels) { return pow2_in(H, 16, 256) && pow2_in(W, 16, 256) && channels >= 1 && channels <= 8; }
bool restore_fft_plane_form(int H, int W) { return (long long)H * W <= FC_PLANE_MAX; }

int fft_conv_init_device() {
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fc_plane_kernel<FcMode::Step>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                FC_PLANE_MAX * 8));
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fc_plane_kernel<FcMode::Apply>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                FC_PLANE_MAX * 8));
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fc_plane_kernel<FcMode::Spectrum>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                FC_PLANE_MAX * 8));
    DDK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fc_plane_noisy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, FC_PLANE_MAX * 8));
    return DDK_OK;
}

static FcStep fc_shape(int H, int W, int C, const float* tw, float* tmp) {
    FcStep p{};
    p.N = H * W; p.logw = ilog2(W); p.logh = ilog2(H); p.logt = p.logw > p.logh ? p.logw : p.logh; p.C = C;
    p.tw = reinterpret_cast<const float2*>(tw); p.tmp = reinterpret_cast<float2*>(tmp);
    p.inv_n = 1.0f / (float)p.N;
    return p;
}
static unsigned fc_plane_threads(int N) { return (unsigned)(N / 4 < 64 ? 64 : N / 4 > 1024 ? 1024 : N / 4); }

// the entries behind the C ABI: shapes and pointers are the caller's to have checked
template <FcMode M>
static int fc_run(const FcStep& p, int B, int H, int W, const ChainHooks& h, hipStream_t st) {
    const int N = p.N, C = p.C;
    DDK_TRY(ensure_device_init());
    if (restore_fft_plane_form(H, W)) {
        hipLaunchKernelGGL(fc_plane_kernel<M>, dim3(B * C), dim3(fc_plane_threads(N)), (size_t)N * sizeof(float2), st, p, h.seed, h.stream_id,
                           h.chain_state, h.dec_counter);
        return check_launch("fc_plane_kernel");
    }
    hipLaunchKernelGGL(fc_rows_in_kernel<M>, dim3(N / FC_RUN, B * C), dim3(1024), 0, st, p);
    DDK_TRY(check_launch("fc_rows_in_kernel"));
    hipLaunchKernelGGL(fc_cols_kernel<M>, dim3(W / FC_STRIP, B * C), dim3(1024), 0, st, p);
    DDK_TRY(check_launch("fc_cols_kernel"));
    hipLaunchKernelGGL(fc_rows_out_kernel<M>, dim3((N / FC_RUN) * B * C), dim3(1024), 0, st, p, h.seed, h.stream_id, h.chain_state,
                       h.dec_counter);
    return check_launch("fc_rows_out_kernel");
}

int p_update_restore_fft(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st) {
    FcStep p = fc_shape(r.rst.H, r.rst.W, channels, r.fft.tw, r.fft.tmp);
    p.x = r.x; p.eps = eps_hat; p.yp = r.rst.y; p.mask = r.fft.mask; p.t = t;
    p.c_recip = r.c_recip; p.c_recipm1 = r.c_recipm1; p.c1 = r.c1; p.c2 = r.c2; p.sigma = r.sigma;
    return fc_run<FcMode::Step>(p, B, r.rst.H, r.rst.W, h, st);
}

// what the lone convolution asks beyond its tensors: null when sound
const char* circular_conv_fault(const void* in, const void* mul, const void* tw, const void* out, const void* scratch, int B, int H, int W, int C) {
    if (!(in && mul && tw && out)) return "null pointer";
    if (!(B > 0 && (long long)B * C <= 65535 && restore_fft_shape_ok(H, W, C))) return "H and W must be powers of two in [16, 256], channels in 1..8, B channels <= 65535";
    if (!restore_fft_plane_form(H, W) && !scratch) return "a plane above 16384 pixels needs the scratch for T";
    if (!(aligned16(in) && aligned16(mul) && aligned16(tw) && aligned16(out) && aligned16(scratch))) return "alignment";
    return nullptr;
}

int circular_conv(const float* in, const float* mul, const float* tw, float* out, float* scratch, int B, int H, int W, int C, hipStream_t st) {
    FcStep p = fc_shape(H, W, C, tw, scratch);
    p.in = in; p.x = out; p.mul = reinterpret_cast<const float2*>(mul);
    return fc_run<FcMode::Apply>(p, B, H, W, ChainHooks{}, st);
}

// the forward half of circular_conv: out [B][C][N] complex = mul . F2(in), left in the transform's order
int circular_spectrum(const float* in, const float* mul, const float* tw, float* out, float* scratch, int B, int H, int W, int C, hipStream_t st) {
    FcStep p = fc_shape(H, W, C, tw, scratch);
    p.in = in; p.x = out; p.mul = reinterpret_cast<const float2*>(mul);
    const int N = p.N;
    const ChainHooks h{};
    DDK_TRY(ensure_device_init());
    if (restore_fft_plane_form(H, W)) {
        hipLaunchKernelGGL(fc_plane_kernel<FcMode::Spectrum>, dim3(B * C), dim3(fc_plane_threads(N)), (size_t)N * sizeof(float2), st, p, h.seed,
                           h.stream_id, h.chain_state, h.dec_counter);
        return check_launch("fc_plane_kernel");
    }
    hipLaunchKernelGGL(fc_rows_in_kernel<FcMode::Apply>, dim3(N / FC_RUN, B * C), dim3(1024), 0, st, p);
    DDK_TRY(check_launch("fc_rows_in_kernel"));
    hipLaunchKernelGGL(fc_cols_kernel<FcMode::Spectrum>, dim3(W / FC_STRIP, B * C), dim3(1024), 0, st, p);
    return check_launch("fc_cols_kernel");
}

int p_update_restore_fft_noisy(const StepRule& r, const float* eps_hat, const int64_t* t, int B, int channels, const ChainHooks& h, hipStream_t st) {
    const int H = r.rst.H, W = r.rst.W;
    FcNoisy pn{};
    FcStep& p = pn.s;
    p = fc_shape(H, W, channels, r.fnz.tw, r.fnz.tmp);
    p.x = r.x; p.eps = eps_hat; p.mask = r.fnz.mask; p.t = t;
    p.c_recip = r.c_recip; p.c_recipm1 = r.c_recipm1; p.c1 = r.c1; p.c2 = r.c2; p.sigma = r.sigma;
    pn.gain = r.fnz.gain; pn.nsc = r.fnz.nsc; pn.yhat = reinterpret_cast<const float2*>(r.rst.y);
    const int N = p.N, C = channels;
    pn.tmp2 = p.tmp ? p.tmp + (long long)B * C * N : nullptr;      // T2 lies behind T
    DDK_TRY(ensure_device_init());
    if (restore_fft_plane_form(H, W)) {
        hipLaunchKernelGGL(fc_plane_noisy_kernel, dim3(B * C), dim3(fc_plane_threads(N)), (size_t)N * sizeof(float2), st, pn, h.seed, h.stream_id,
                           h.chain_state, h.dec_counter);
        return check_launch("fc_plane_noisy_kernel");
    }
    hipLaunchKernelGGL(fc_rows_in_noisy_kernel, dim3(N / FC_RUN, B * C), dim3(1024), 0, st, pn, h.seed, h.stream_id, h.chain_state);
    DDK_TRY(check_launch("fc_rows_in_noisy_kernel"));
    hipLaunchKernelGGL(fc_cols_noisy_kernel, dim3(W / FC_STRIP, B * C, 2), dim3(1024), 0, st, pn);
    DDK_TRY(check_launch("fc_cols_noisy_kernel"));
    hipLaunchKernelGGL(fc_rows_out_noisy_kernel, dim3((N / FC_RUN) * B * C), dim3(1024), 0, st, pn, h.seed, h.stream_id, h.chain_state,
                       h.dec_counter);
    return check_launch("fc_rows_out_noisy_kernel");
}

}  // namespace ddk

using namespace ddk;

extern "C" {

int ddk_circular_conv(const float* x, const float* S, const float* twiddles, float* out, float* scratch, int B, int H, int W, int channels,
                      ddk_stream_t s) {
    if (const char* fault = circular_conv_fault(x, S, twiddles, out, scratch, B, H, W, channels)) {
        set_error("bad argument: circular_conv: %s", fault);
        return DDK_ERR_ARG;
    }
    return circular_conv(x, S, twiddles, out, scratch, B, H, W, channels, as_stream(s));
}

int ddk_p_sample_update_restore_fft(float* x, const float* eps_hat, const float* mask, const float* twiddles, const float* Yp, float* scratch,
                                    const int64_t* t, const float* c_recip, const float* c_recipm1, const float* c1, const float* c2,
                                    const float* sigma, int B, int H, int W, int channels, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && channels > 0, "p_sample_update_restore_fft: B / H / W / channels must be positive");
    StepRule r{StepKind::RestoreFFT, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, sigma};
    r.fft = FftOps{mask, twiddles, scratch, nullptr};
    r.rst = RestoreOps{Yp, 0, H, W, 0, nullptr};
    return p_update(r, eps_hat, t, B, (long long)H * W * channels, ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s),
                    "p_sample_update_restore_fft");
}

int ddk_circular_spectrum(const float* x, const float* S, const float* twiddles, float* out, float* scratch, int B, int H, int W, int channels,
                          ddk_stream_t s) {
    if (const char* fault = circular_conv_fault(x, S, twiddles, out, scratch, B, H, W, channels)) {
        set_error("bad argument: circular_spectrum: %s", fault);
        return DDK_ERR_ARG;
    }
    return circular_spectrum(x, S, twiddles, out, scratch, B, H, W, channels, as_stream(s));
}

int ddk_p_sample_update_restore_fft_noisy(float* x, const float* eps_hat, const float* mask, const float* gain, const float* nsc,
                                          const float* twiddles, const float* Yhat, float* scratch, const int64_t* t, const float* c_recip,
                                          const float* c_recipm1, const float* c1, const float* c2, const float* sigma, int B, int H, int W,
                                          int channels, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && channels > 0, "p_sample_update_restore_fft_noisy: B / H / W / channels must be positive");
    StepRule r{StepKind::RestoreFFTNoisy, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, sigma};
    r.fnz = FftNoisyOps{mask, twiddles, scratch, gain, nsc, nullptr};
    r.rst = RestoreOps{Yhat, 0, H, W, 0, nullptr};
    return p_update(r, eps_hat, t, B, (long long)H * W * channels, ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s),
                    "p_sample_update_restore_fft_noisy");
}

}  // extern "C"
