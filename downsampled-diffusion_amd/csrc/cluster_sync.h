// cluster_sync.h -- the in-launch exchange between the workgroups of one launch, written once for every kernel that does one:
// the in-launch GroupNorm of the Winograd convs (conv_wino.hip, conv_wino2_kernel.inc) and of the first Block (conv_first.hip),
// the k-split pair hand-off (conv_wino2_kernel.inc) and the level chains (level_chain.hip).
//
// The form is row 1 of MI355X_MICROARCH.md's sc1 table ("Valid forms"): every record byte is stored sc1 by ONE wave, which drains
// its stores (s_waitcnt vmcnt(0)) before its lane 0 adds to the cluster's arrival counter (agent scope); one lane polls the counter
// with sc1 loads (cl_wait_ge), the other waves pass a workgroup barrier behind it, and every record is read with sc1 loads
// (hipMalloc memory, ONE workgroup per CU).  Measured form, not an architectural guarantee; a record has its 128-byte line to
// itself.  Who stores, drains, signals and polls, and the barrier behind the poll, stay at each site: only what every site repeats
// lives here.  The workgroups of a cluster have consecutive launch indices inside one XCD's run, so they are co-resident whenever
// the dispatcher works in order on a whole, otherwise idle device (conv_wino_cluster_device_ok gates on that); the wait is bounded
// by wall time anyway, and a give-up is never silent: NaN output + sticky counters (ddk_unet_cluster_check,
// ddk_debug_cluster_timeouts).
#pragma once
#include <hip/hip_runtime.h>

namespace ddk {

constexpr unsigned long long CL_TIMEOUT_TICKS = 2000000ull;   // 20 ms of the 100 MHz s_memrealtime clock: a peer is normally < 0.1 ms away

// Workgroups of this code object that gave up waiting.  Without -fgpu-rdc every .hip file is its own code object and a __device__
// variable cannot be shared between them: each file that includes this header keeps its own count, and cl_timeouts_read() is its
// host reader; ddk_debug_cluster_timeouts() sums them.
static __device__ unsigned g_cl_timeouts;

static unsigned cl_timeouts_read() {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_cl_timeouts), sizeof(v)) != hipSuccess) return ~0u;
    return v;
}

// One lane waits until *cnt >= want: checked once, then polled behind s_sleep SLEEP (each site keeps its own) with relaxed
// agent-scope (sc1) loads, bounded by wall time.  Returns true when it gave up: the process-wide count and the sticky fail word
// (when non-null) have moved, and the caller poisons its output.
template <int SLEEP>
__device__ __forceinline__ bool cl_wait_ge(const unsigned* cnt, unsigned want, unsigned* fail) {
    if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return false;
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return false;
        if (__builtin_amdgcn_s_memrealtime() - t_begin > CL_TIMEOUT_TICKS) {
            atomicAdd(&g_cl_timeouts, 1u);
            if (fail) __hip_atomic_fetch_add(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
    }
}

// Departure: the last of n workgroups out re-arms both counters for the next launch.
__device__ __forceinline__ void cl_depart(unsigned* arrive, unsigned* depart, unsigned n) {
    if (__hip_atomic_fetch_add(depart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n - 1u) {
        __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(depart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A GroupNorm record: {mean, M2} of one group over one tile, 8 bytes, stored and loaded whole (sc1).
__device__ __forceinline__ void cl_store_stats(unsigned long long* rec, float mean, float m2) {
    const unsigned long long bits = (unsigned long long)__float_as_uint(mean) | ((unsigned long long)__float_as_uint(m2) << 32);
    __hip_atomic_store(rec, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the np (<= MAXP) records r0[i * stride] of one group, in tile order
template <int MAXP>
__device__ __forceinline__ void cl_load_stats(const unsigned long long* r0, long long stride, int np, float (&rm)[MAXP], float (&rq)[MAXP]) {
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
        rm[i] = rq[i] = 0.f;
        if (i < np) {
            const unsigned long long bits = __hip_atomic_load(r0 + i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rm[i] = __uint_as_float((unsigned)bits);
            rq[i] = __uint_as_float((unsigned)(bits >> 32));
        }
    }
}

// The group's statistics over np tiles of n_i values each: mean of the means, M2 = sum M2_i + n_i sum (mean_i - mean)^2, summed in
// tile order -- the arithmetic of gn_apply_parts_kernel, so the fused and the unfused path give the same bits (the two products
// contracted into fmas as the compiler does there, spelled out so that a neighbouring vectorised product cannot split them).
// {mean, rstd}; a poisoned exchange (a give-up) makes both NaN.
template <int MAXP>
__device__ __forceinline__ float2 cl_merge_stats(const float (&rm)[MAXP], const float (&rq)[MAXP], int np, float n_i, float eps, bool poisoned) {
    float ms = 0.f;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) if (i < np) ms += rm[i];
    const float mean = poisoned ? __builtin_nanf("") : ms / (float)np;
    float m2 = 0.f, d2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) if (i < np) { m2 += rq[i]; d2 = __builtin_fmaf(rm[i] - mean, rm[i] - mean, d2); }
    return make_float2(mean, 1.0f / sqrtf(__builtin_fmaf(n_i, d2, m2) / ((float)np * n_i) + eps));
}

}  // namespace ddk
