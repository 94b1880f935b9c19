// The device arithmetic that diffusion.hip, separable.hip, hadamard.hip and fft_conv.hip share: the Philox draws, the clipped x0 of a restore step and the
// update behind it.  All four files are compiled with -ffp-contract=off (Makefile): every product below rounds on its own.
#pragma once
#include "ddk_internal.h"

namespace ddk {

// ---- Philox4x32-10 (Salmon et al. SC'11; Random123 philox4x32_R(10)) -----------------------------
struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    }
    return c;
}

__device__ __forceinline__ float u01(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f; }  // 2^-24

__device__ __forceinline__ float4 philox_normal4(unsigned long long idx4, uint32_t step, uint32_t stream, uint64_t seed) {
    const U4 r = philox4x32_10(U4{(uint32_t)idx4, (uint32_t)(idx4 >> 32), step, stream}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float two_pi = 6.283185307179586f;
    float4 z;
    float sn, cs;
    float rad = sqrtf(-2.0f * logf(u01(r.x)));
    sincosf(two_pi * u01(r.y), &sn, &cs);
    z.x = rad * cs; z.y = rad * sn;
    rad = sqrtf(-2.0f * logf(u01(r.z)));
    sincosf(two_pi * u01(r.w), &sn, &cs);
    z.z = rad * cs; z.w = rad * sn;
    return z;
}

template <StepKind K>
struct RestoreTraits {
    static constexpr bool RESTORE = restore_kind(K);
    static constexpr bool PLANE = plane_kind(K);
    static constexpr bool MASK = RESTORE && K != StepKind::Restore && !PLANE;
    static constexpr bool MASK_REQUIRED = K == StepKind::RestoreMasked;
    static constexpr bool HIST = K == StepKind::RestoreMultistep;
    static constexpr bool NOISY = K == StepKind::RestoreNoisy || K == StepKind::RestoreGray;
    static constexpr bool GRAY = K == StepKind::RestoreGray;
    static constexpr bool POINT = MASK && !GRAY;      // n = 1 is pointwise
};

// clamp_(-1, 1) as torch computes it: a finite x0 keeps its bits, a NaN stays a NaN (fminf / fmaxf would return the bound: a NaN in
// eps_hat would leave the step as x0 = -1 and the sample would be finite garbage)
__device__ __forceinline__ float clamp_pm1(float x0) { return x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0); }

// max(v, lo) that keeps a NaN in v, as torch's clamp(min=lo)
__device__ __forceinline__ float clamp_min_nan(float v, float lo) { return v < lo ? lo : v; }

__device__ __forceinline__ float rst_x0(float x, float e, float cr, float crm1) {
    const float x0 = __fsub_rn(__fmul_rn(cr, x), __fmul_rn(crm1, e));     // as p_step
    return clamp_pm1(x0);
}

// The ancestral / DDIM step rule of ddk_p_sample_update, ddk_final_tail and ddk_p_sample_update_guided: one function, so given the
// same eps_hat and draw they agree bit for bit.
__device__ __forceinline__ float p_step(float x, float e, float z, float cr, float crm1, float c1, float c2, float sg) {
    float x0 = __fsub_rn(__fmul_rn(cr, x), __fmul_rn(crm1, e));     // ddpm.py:152-155
    x0 = clamp_pm1(x0);                                             // ddpm.py:157 clamp_(-1, 1): a NaN stays a NaN
    const float mean = __fadd_rn(__fmul_rn(c1, x0), __fmul_rn(c2, x));  // ddpm.py:177-180
    return __fadd_rn(mean, __fmul_rn(sg, z));                       // ddpm.py:227 (sg already carries the t>0 mask)
}

// zh: the draw, or (HIST) the history, which leaves holding x0'; a5: sigma, or (HIST) c3; sgm: NOISY
template <StepKind K>
__device__ __forceinline__ float rst_finish(float x, float x0p, float mk, float& zh, float c1, float c2, float a5, float sgm) {
    using T = RestoreTraits<K>;
    const float mean = __fadd_rn(__fmul_rn(c1, x0p), __fmul_rn(c2, x));
    float sc = a5;
    if constexpr (T::NOISY) sc = mk != 0.0f ? sgm : a5;
    const float out = __fadd_rn(mean, __fmul_rn(sc, zh));
    if constexpr (T::HIST) zh = x0p;
    return out;
}

__device__ __forceinline__ float comp4(float4 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// what the unfused restore kernels begin with: the counter decrement and the chain's Philox key, as in p_update_kernel
__device__ __forceinline__ void rst_prologue(int64_t* dec_counter, const int64_t* __restrict__ chain_state, uint64_t& seed, uint32_t& stream) {
    if (dec_counter && blockIdx.x == 0 && threadIdx.x == 0) *dec_counter -= 1;
    if (chain_state) {
        seed = (uint64_t)chain_state[1];
        stream = (uint32_t)chain_state[2];
    }
}

}  // namespace ddk
