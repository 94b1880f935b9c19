// manifold.hip -- the k-nearest-neighbour manifold estimate behind precision / recall of generated samples (Kynkaanniemi et al.,
// "Improved precision and recall metric for assessing generative models", NeurIPS 2019), on [N][D] fp32 feature rows.
// DESIGN.md section 3.16.
//
// Squared distance, everywhere: d(u, v) = max((|u|^2 - 2 u.v) + |v|^2, 0) in fp32, the row norms computed once.  The dot products of a
// 128 x 128 tile of (row, column) pairs run on v_mfma_f32_32x32x2_f32 from LDS-staged operands; the tile never leaves the chip:
//   * ddk_knn_radii keeps, per row, the 8 smallest distances met so far (k + 1 <= 8) across the column tiles its workgroup walks, and a
//     finish kernel merges the lists of the workgroups that shared a row block's columns;
//   * ddk_manifold_members tests d <= r in the accumulators and stores 1 into zeroed uint8 flags.
// Numerics: a dot product is one fmaf chain over k in a fixed order (within a group of 8 features: 0 4 1 5 2 6 3 7) that depends on
// nothing but D, so the column split, the launch geometry and the arrival order change no bit.  Selection works on the multiset of a
// row's distances and flags only ever receive a 1: no atomics, no order anywhere.
//
// On the same tiles:
//   * ddk_manifold_ball_counts counts d <= r per row instead of testing for any (density / coverage, Naeem et al. 2020): integer adds;
//   * ddk_poly_mmd_sums replaces the distance by the cubic kernel k = (gamma u.v + coef0)^3 and the test by a sum (KID, Binkowski et
//     al. 2018): fp32 up to k, double from there on, one partial per tile and a finish kernel that adds them in a fixed order.
#include "ddk_internal.h"

#include <algorithm>
#include <cmath>

namespace ddk {

constexpr int MF_TILE = 128;              // rows and columns of a workgroup's tile: 2 x 2 waves of 64 x 64, each 2 x 2 MFMA tiles of 32 x 32
constexpr int MF_BK = 32;                 // features per LDS stage
constexpr int MF_LDK = MF_BK + 4;         // operand row pitch in floats: 16-byte aligned rows, 9 float4 apart, so the b128 reads of
                                          // 32 consecutive rows spread over the banks
constexpr int MF_THREADS = 256;
constexpr int MF_KEEP = 8;                // smallest distances kept per row: k + 1 <= 8
constexpr int MF_HALF = 64;               // columns of the tile selected per epilogue pass (one column of waves)
constexpr int MF_LDD = MF_HALF + 1;       // distance row pitch: a wave scans 64 different rows at one column, 65 floats apart
constexpr int MF_RESIDENT_WGS = 512;      // workgroups a whole MI355X holds at once: 2 per CU (215 registers per lane), 256 CUs
constexpr int MF_MAX_SPLITS = 8;          // column ranges per row block, at most (the partial lists are splits x N x 8 floats)
constexpr int MF_MAX_ROWS = 1 << 24;

using mf_f32x16 = __attribute__((ext_vector_type(16))) float;
using mf_f32x4 = __attribute__((ext_vector_type(4))) float;

struct MfOperands {
    float a[MF_TILE][MF_LDK];
    float b[MF_TILE][MF_LDK];
};
union MfSmem {
    MfOperands op;                        // main loop
    float d[MF_TILE][MF_LDD];             // radii epilogue: one 128 x 64 half of the tile's distances
    float merge[MF_TILE][MF_KEEP];        // radii: the second half-row scanner's list on its way to the first
};

// norms[i] = |x_i|^2: one wave per row, lane l adds features 4l .. 4l + 3, 4l + 256 .., then the butterfly
__global__ __launch_bounds__(256) void mf_norms_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ norms) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* p = x + (size_t)row * D;
    float s = 0.0f;
    for (int k = lane * 4; k < D; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(p + k);
        s = fmaf(v.x, v.x, s);
        s = fmaf(v.y, v.y, s);
        s = fmaf(v.z, v.z, s);
        s = fmaf(v.w, v.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) norms[row] = s;
}

// features k0 + 4 (t & 7) .. + 3 of rows row0 + (t >> 3) + 32 i; rows past n and features past D (D % 4 == 0) read as 0
__device__ __forceinline__ void mf_fetch(const float* __restrict__ x, int n, int row0, int D, int k0, float4 (&r)[4]) {
    const int c = k0 + (threadIdx.x & 7) * 4, rr = row0 + (threadIdx.x >> 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = rr + 32 * i;
        r[i] = (row < n && c < D) ? *reinterpret_cast<const float4*>(x + (size_t)row * D + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

__device__ __forceinline__ void mf_stage(float (*s)[MF_LDK], const float4 (&r)[4]) {
    const int c = (threadIdx.x & 7) * 4, rr = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&s[rr + 32 * i][c]) = r[i];
}

// acc[mi][ni] <- the dot products of rows rbase + wm 64 + mi 32 + .. of a with rows cbase + wn 64 + ni 32 + .. of b, in the C/D
// layout of the 32 x 32 MFMA: register g of lane l is (row (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31).
// The operand of lane (r, h) in MFMA j of an 8-feature group is feature 4 h + j of row r, read as one float4 per group: any
// assignment of features to (MFMA, lane half) sums the same products, and this one needs no LDS transpose.
// Every thread of the workgroup calls it; it begins with a barrier, so the caller's earlier use of `sm` is over when it is overwritten.
__device__ __forceinline__ void mf_tile_dots(const float* __restrict__ a, int Na, int rbase, const float* __restrict__ b, int Nb, int cbase,
                                             int D, MfSmem& sm, mf_f32x16 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[mi][ni][g] = 0.0f;
    float4 ga[4], gb[4];
    mf_fetch(a, Na, rbase, D, 0, ga);
    mf_fetch(b, Nb, cbase, D, 0, gb);
    for (int k0 = 0; k0 < D; k0 += MF_BK) {
        __syncthreads();
        mf_stage(sm.op.a, ga);
        mf_stage(sm.op.b, gb);
        __syncthreads();
        if (k0 + MF_BK < D) {             // the next stage's global loads fly under this stage's MFMAs
            mf_fetch(a, Na, rbase, D, k0 + MF_BK, ga);
            mf_fetch(b, Nb, cbase, D, k0 + MF_BK, gb);
        }
#pragma unroll
        for (int kc = 0; kc < MF_BK / 8; ++kc) {
            mf_f32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const mf_f32x4*>(&sm.op.a[wm * 64 + i * 32 + lr][kc * 8 + lh * 4]);
                fb[i] = *reinterpret_cast<const mf_f32x4*>(&sm.op.b[wn * 64 + i * 32 + lr][kc * 8 + lh * 4]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][j], fb[ni][j], acc[mi][ni], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ float mf_dist(float nu, float dot, float nv) { return fmaxf((nu - 2.0f * dot) + nv, 0.0f); }

// best: ascending, the MF_KEEP smallest values seen; d joins it if it is smaller than the largest
__device__ __forceinline__ void mf_insert(float (&best)[MF_KEEP], float d) {
    if (d < best[MF_KEEP - 1]) {
        best[MF_KEEP - 1] = d;
#pragma unroll
        for (int i = MF_KEEP - 2; i >= 0; --i) {
            const float lo = fminf(best[i], best[i + 1]), hi = fmaxf(best[i], best[i + 1]);
            best[i] = lo;
            best[i + 1] = hi;
        }
    }
}

// workgroup (rb, sp): rows rb 128 .. of x against column tiles sp tps .. (sp + 1) tps - 1; lists[sp][row][8] = the row's 8 smallest
// distances in that range, ascending, +inf where the range has fewer columns
__global__ __launch_bounds__(MF_THREADS) void mf_knn_kernel(const float* __restrict__ x, const float* __restrict__ norms, int N, int D,
                                                            int col_tiles, int tps, float* __restrict__ lists) {
    __shared__ MfSmem sm;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int rbase = blockIdx.x * MF_TILE, sp = blockIdx.y;
    const int t0 = sp * tps, t1 = min(col_tiles, t0 + tps);
    const int srow = threadIdx.x & (MF_TILE - 1), shalf = threadIdx.x >> 7;       // selection: two threads per row, 32 columns each per pass
    float best[MF_KEEP];
#pragma unroll
    for (int i = 0; i < MF_KEEP; ++i) best[i] = INFINITY;
    for (int t = t0; t < t1; ++t) {
        const int cbase = t * MF_TILE;
        mf_f32x16 acc[2][2];
        mf_tile_dots(x, N, rbase, x, N, cbase, D, sm, acc);
        for (int p = 0; p < 2; ++p) {
            __syncthreads();              // the operands (p = 0) or the first half's distances (p = 1) have been read
            if (wn == p) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const int cl = ni * 32 + lr, col = cbase + p * MF_HALF + cl;
                    const bool cv = col < N;
                    const float nv = cv ? norms[col] : 0.0f;
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int g = 0; g < 16; ++g) {
                            const int rl = wm * 64 + mi * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh, row = rbase + rl;
                            const float nu = row < N ? norms[row] : 0.0f;
                            sm.d[rl][cl] = cv ? mf_dist(nu, acc[mi][ni][g], nv) : INFINITY;
                        }
                }
            }
            __syncthreads();
#pragma unroll 8
            for (int j = 0; j < MF_HALF / 2; ++j) mf_insert(best, sm.d[srow][shalf * (MF_HALF / 2) + j]);
        }
    }
    __syncthreads();
    if (shalf == 1) {
#pragma unroll
        for (int i = 0; i < MF_KEEP; ++i) sm.merge[srow][i] = best[i];
    }
    __syncthreads();
    if (shalf == 0 && rbase + srow < N) {
#pragma unroll
        for (int i = 0; i < MF_KEEP; ++i) mf_insert(best, sm.merge[srow][i]);
        float* o = lists + ((size_t)sp * N + rbase + srow) * MF_KEEP;
#pragma unroll
        for (int i = 0; i < MF_KEEP; ++i) o[i] = best[i];
    }
}

// radii[row] = element k of the merged lists of the row (thread per row)
__global__ __launch_bounds__(256) void mf_knn_finish_kernel(const float* __restrict__ lists, int N, int splits, int k,
                                                            float* __restrict__ radii) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    float best[MF_KEEP];
#pragma unroll
    for (int i = 0; i < MF_KEEP; ++i) best[i] = INFINITY;
    for (int sp = 0; sp < splits; ++sp) {
        const float* l = lists + ((size_t)sp * N + row) * MF_KEEP;
#pragma unroll
        for (int i = 0; i < MF_KEEP; ++i) mf_insert(best, l[i]);
    }
    float r = best[0];
#pragma unroll
    for (int i = 1; i < MF_KEEP; ++i) r = (i == k) ? best[i] : r;
    radii[row] = r;
}

// workgroup (rb, sp): rows rb 128 .. of a against its column tiles of b; a_in[i] = 1 where some d(a_i, b_j) <= rb[j],
// b_in[j] = 1 where some d(a_i, b_j) <= ra[i].  Both arrays are zero before the launch; every store writes 1.
__global__ __launch_bounds__(MF_THREADS) void mf_members_kernel(const float* __restrict__ a, const float* __restrict__ na,
                                                                const float* __restrict__ ra, int Na, const float* __restrict__ b,
                                                                const float* __restrict__ nb, const float* __restrict__ rb, int Nb, int D,
                                                                int col_tiles, int tps, uint8_t* __restrict__ a_in,
                                                                uint8_t* __restrict__ b_in) {
    __shared__ MfSmem sm;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int rbase = blockIdx.x * MF_TILE, sp = blockIdx.y;
    const int t0 = sp * tps, t1 = min(col_tiles, t0 + tps);
    for (int t = t0; t < t1; ++t) {
        const int cbase = t * MF_TILE;
        mf_f32x16 acc[2][2];
        mf_tile_dots(a, Na, rbase, b, Nb, cbase, D, sm, acc);
        int col[2];
        bool cv[2], bhit[2] = {false, false};
        float nv[2], rv[2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            col[ni] = cbase + wn * 64 + ni * 32 + lr;
            cv[ni] = col[ni] < Nb;
            nv[ni] = cv[ni] ? nb[col[ni]] : 0.0f;
            rv[ni] = (cv[ni] && rb) ? rb[col[ni]] : 0.0f;
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = rbase + wm * 64 + mi * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
                if (row >= Na) continue;
                const float nu = na[row], ru = ra ? ra[row] : 0.0f;
                bool ahit = false;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const float d = mf_dist(nu, acc[mi][ni][g], nv[ni]);
                    ahit = ahit || (cv[ni] && rb && d <= rv[ni]);
                    bhit[ni] = bhit[ni] || (cv[ni] && ra && d <= ru);
                }
                if (ahit) a_in[row] = 1;
            }
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
            if (bhit[ni]) b_in[col[ni]] = 1;
    }
}

// workgroup (rb, sp): rows rb 128 .. of a against its column tiles of b; counts[i] += the number of its columns j with
// d(a_i, b_j) <= ra[i].  counts is zero before the launch; integer adds are exact in any order.
// Every lane counts its own columns over the whole column walk; a row's columns sit in the 32 lanes of a half wave, which are added
// once at the end.
__global__ __launch_bounds__(MF_THREADS) void mf_ball_counts_kernel(const float* __restrict__ a, const float* __restrict__ na,
                                                                    const float* __restrict__ ra, int Na, const float* __restrict__ b,
                                                                    const float* __restrict__ nb, int Nb, int D, int col_tiles, int tps,
                                                                    int* __restrict__ counts) {
    __shared__ MfSmem sm;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int rbase = blockIdx.x * MF_TILE, sp = blockIdx.y;
    const int t0 = sp * tps, t1 = min(col_tiles, t0 + tps);
    int cnt[2][16];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int g = 0; g < 16; ++g) cnt[mi][g] = 0;
    for (int t = t0; t < t1; ++t) {
        const int cbase = t * MF_TILE;
        mf_f32x16 acc[2][2];
        mf_tile_dots(a, Na, rbase, b, Nb, cbase, D, sm, acc);
        bool cv[2];
        float nv[2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int col = cbase + wn * 64 + ni * 32 + lr;
            cv[ni] = col < Nb;
            nv[ni] = cv[ni] ? nb[col] : 0.0f;
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = rbase + wm * 64 + mi * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
                const bool rv = row < Na;
                const float nu = rv ? na[row] : 0.0f, ru = rv ? ra[row] : 0.0f;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) cnt[mi][g] += (rv && cv[ni] && mf_dist(nu, acc[mi][ni][g], nv[ni]) <= ru) ? 1 : 0;
            }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            int c = cnt[mi][g];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);       // offsets below 32 stay inside the half wave
            const int row = rbase + wm * 64 + mi * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
            if (lr == 0 && row < Na && c > 0) atomicAdd(counts + row, c);
        }
}

// ---- the kernel-matrix sums of MMD^2 with k(x, y) = (gamma x.y + coef0)^3 (KID)
// Tiles of one segment, in this order: the upper triangle (ti <= tj, row-major) of the ta x ta tiles of a x a, the same of b x b, then
// the ta x tb tiles of a x b.  Every tile gives one double partial; an off-diagonal tile of a symmetric matrix counts twice (its mirror
// image holds the same fmaf chains, bit for bit, so 2 x is the same sum).

// item r of the row-major upper triangle of T x T tiles -> (ti, tj); row ti begins at ti T - ti (ti - 1) / 2
__device__ __forceinline__ void mf_triangle(long long r, long long T, int* ti, int* tj) {
    const double w = 2.0 * (double)T + 1.0;
    long long i = (long long)((w - sqrt(fmax(w * w - 8.0 * (double)r, 0.0))) * 0.5);
    i = max(0ll, min(T - 1, i));
    while (i > 0 && i * T - i * (i - 1) / 2 > r) --i;                         // the square root may be off by one either way
    while (i + 1 < T && (i + 1) * T - (i + 1) * i / 2 <= r) ++i;
    *ti = (int)i;
    *tj = (int)(i + (r - (i * T - i * (i - 1) / 2)));
}

__device__ __forceinline__ double mf_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// partials[item] for item = blockIdx.x, + gridDim.x, ..: segment item / per, tile item % per in the order above.  Rows of a tile past
// the segment's end are read as zeros by mf_fetch (its n is the segment's row count) and masked here by index, as is the diagonal.
__global__ __launch_bounds__(MF_THREADS) void mf_mmd_kernel(const float* __restrict__ a, const float* __restrict__ b, int ma, int mb, int D,
                                                            float gamma, float coef0, long long total, double* __restrict__ partials) {
    __shared__ MfSmem sm;
    __shared__ double red[MF_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const long long ta = (ma + MF_TILE - 1) / MF_TILE, tb = (mb + MF_TILE - 1) / MF_TILE;
    const long long naa = ta * (ta + 1) / 2, nbb = tb * (tb + 1) / 2, per = naa + nbb + ta * tb;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        const long long seg = item / per;
        long long r = item - seg * per;
        const float* pa = a + (size_t)seg * ma * D;
        const float* pb = b + (size_t)seg * mb * D;
        const float *u, *v;
        int nu, nv, ti, tj;
        bool sym = true;
        if (r < naa) {
            u = v = pa;
            nu = nv = ma;
            mf_triangle(r, ta, &ti, &tj);
        } else if (r < naa + nbb) {
            u = v = pb;
            nu = nv = mb;
            mf_triangle(r - naa, tb, &ti, &tj);
        } else {
            r -= naa + nbb;
            sym = false;
            u = pa, nu = ma;
            v = pb, nv = mb;
            ti = (int)(r / tb), tj = (int)(r % tb);
        }
        const int rbase = ti * MF_TILE, cbase = tj * MF_TILE;
        const bool diag = sym && ti == tj;
        mf_f32x16 acc[2][2];
        mf_tile_dots(u, nu, rbase, v, nv, cbase, D, sm, acc);
        double s = 0.0;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int col = cbase + wn * 64 + ni * 32 + lr;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = rbase + wm * 64 + mi * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
                    const float t = fmaf(gamma, acc[mi][ni][g], coef0);
                    const float k = (t * t) * t;
                    s += (row < nu && col < nv && !(diag && row == col)) ? (double)k : 0.0;
                }
        }
        s = mf_wave_sum_f64(s);
        if (lane == 0) red[wave] = s;         // read below before the barrier that opens the next item's mf_tile_dots
        __syncthreads();
        if (threadIdx.x == 0) partials[item] = ((sym && !diag) ? 2.0 : 1.0) * (((red[0] + red[1]) + red[2]) + red[3]);
    }
}

// sums[seg][m] = the partials of matrix m of the segment: thread t adds partials t, t + 256, .. in that order, then a fixed tree
__global__ __launch_bounds__(256) void mf_mmd_finish_kernel(const double* __restrict__ partials, long long outputs, long long naa,
                                                            long long nbb, long long nab, double* __restrict__ sums) {
    __shared__ double red[256];
    const long long per = naa + nbb + nab;
    for (long long o = blockIdx.x; o < outputs; o += gridDim.x) {
        const long long seg = o / 3;
        const int m = (int)(o - seg * 3);
        const long long off = m == 0 ? 0 : (m == 1 ? naa : naa + nbb), n = m == 0 ? naa : (m == 1 ? nbb : nab);
        const double* p = partials + seg * per + off;
        double s = 0.0;
        for (long long i = threadIdx.x; i < n; i += 256) s += p[i];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[o] = red[0];
        __syncthreads();
    }
}

constexpr long long MF_MAX_GRID = 1 << 20;      // workgroups of a launch at most; the kernels above stride over what is left

// tiles of one segment: *naa, *nbb upper triangles, *nab the rectangle; false when the arguments are out of range
static bool mf_mmd_tiles(int S, int ma, int mb, long long* naa, long long* nbb, long long* nab) {
    if (S < 1 || ma < 2 || mb < 2 || (long long)S * ma > MF_MAX_ROWS || (long long)S * mb > MF_MAX_ROWS) return false;
    const long long ta = ceil_div(ma, MF_TILE), tb = ceil_div(mb, MF_TILE);
    *naa = ta * (ta + 1) / 2;
    *nbb = tb * (tb + 1) / 2;
    *nab = ta * tb;
    return true;
}

// How the column tiles of a launch with `row_blocks` row blocks are shared out: *tps tiles per workgroup, the return value ranges.
// A launch of W workgroups runs in ceil(W / MF_RESIDENT_WGS) rounds of the time of one workgroup, tps tiles; the split is the smallest
// number of ranges that minimises rounds x tps.  N = 10 000: 79 row blocks x 6 ranges = 474 workgroups of 14 tiles, one round, where
// the unsplit launch leaves 177 of 256 CUs idle for 79 tiles.  The result depends on the shape only.
static int mf_col_splits(long long row_blocks, long long col_tiles, int* tps) {
    long long best = 0, best_cost = -1;
    for (long long s = 1; s <= MF_MAX_SPLITS && s <= col_tiles; ++s) {
        const long long t = ceil_div(col_tiles, s), cost = ceil_div(row_blocks * ceil_div(col_tiles, t), MF_RESIDENT_WGS) * t;
        if (best_cost < 0 || cost < best_cost) {
            best = s;
            best_cost = cost;
        }
    }
    *tps = (int)ceil_div(col_tiles, best);
    return (int)ceil_div(col_tiles, *tps);
}

static bool mf_shape_ok(int N, int D) { return N > 0 && N <= MF_MAX_ROWS && D > 0 && D % 4 == 0; }

static int mf_norms(const float* x, int N, int D, float* norms, hipStream_t st) {
    hipLaunchKernelGGL(mf_norms_kernel, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, st, x, N, D, norms);
    return check_launch("mf_norms_kernel");
}

}  // namespace ddk

using namespace ddk;

extern "C" {

size_t ddk_knn_radii_workspace_bytes(int N) {
    if (N <= 0 || N > MF_MAX_ROWS) return 0;
    int tps;
    const long long tiles = ceil_div(N, MF_TILE);
    const int splits = mf_col_splits(tiles, tiles, &tps);
    return ((size_t)N + (size_t)splits * N * MF_KEEP) * sizeof(float);
}

int ddk_knn_radii(const float* x, int N, int D, int k, float* radii, void* workspace, size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(x && radii, "knn_radii: null pointer");
    DDK_REQUIRE(mf_shape_ok(N, D), "knn_radii: N in 1..2^24, D positive and a multiple of 4");
    DDK_REQUIRE(k >= 1 && k < MF_KEEP, "knn_radii: k must be in 1..7");
    DDK_REQUIRE(N >= k + 1, "knn_radii: N must be at least k + 1");
    DDK_REQUIRE(aligned16(x), "knn_radii: x must be 16-byte aligned");
    DDK_REQUIRE(workspace && workspace_bytes >= ddk_knn_radii_workspace_bytes(N) && aligned16(workspace),
                "knn_radii: workspace (ddk_knn_radii_workspace_bytes, 16-byte aligned)");
    int tps;
    const long long tiles = ceil_div(N, MF_TILE);
    const int splits = mf_col_splits(tiles, tiles, &tps);
    float* norms = static_cast<float*>(workspace);
    float* lists = norms + N;
#ifdef DDK_HOST_SANITIZE
    san::extent("knn_radii x", x, (long long)N * D * 4); san::extent("knn_radii radii", radii, (long long)N * 4);
    san::extent("knn_radii norms", norms, (long long)N * 4); san::extent("knn_radii lists", lists, (long long)splits * N * MF_KEEP * 4);
#endif
    DDK_TRY(mf_norms(x, N, D, norms, as_stream(s)));
    hipLaunchKernelGGL(mf_knn_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(MF_THREADS), 0, as_stream(s), x, (const float*)norms, N, D,
                       (int)tiles, tps, lists);
    DDK_TRY(check_launch("mf_knn_kernel"));
    hipLaunchKernelGGL(mf_knn_finish_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, as_stream(s), (const float*)lists, N, splits, k,
                       radii);
    return check_launch("mf_knn_finish_kernel");
}

size_t ddk_manifold_members_workspace_bytes(int Na, int Nb) {
    if (Na <= 0 || Nb <= 0 || Na > MF_MAX_ROWS || Nb > MF_MAX_ROWS) return 0;
    return ((size_t)Na + (size_t)Nb) * sizeof(float);
}

int ddk_manifold_members(const float* a, const float* ra, int Na, const float* b, const float* rb, int Nb, int D, uint8_t* a_in,
                         uint8_t* b_in, void* workspace, size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(a && b, "manifold_members: null pointer");
    DDK_REQUIRE(mf_shape_ok(Na, D) && mf_shape_ok(Nb, D), "manifold_members: Na, Nb in 1..2^24, D positive and a multiple of 4");
    DDK_REQUIRE(!rb || a_in, "manifold_members: rb without a_in");
    DDK_REQUIRE(!ra || b_in, "manifold_members: ra without b_in");
    DDK_REQUIRE(ra || rb, "manifold_members: neither ra nor rb: nothing to compute");
    DDK_REQUIRE(aligned16(a) && aligned16(b), "manifold_members: a and b must be 16-byte aligned");
    DDK_REQUIRE(workspace && workspace_bytes >= ddk_manifold_members_workspace_bytes(Na, Nb) && aligned16(workspace),
                "manifold_members: workspace (ddk_manifold_members_workspace_bytes, 16-byte aligned)");
    float* na = static_cast<float*>(workspace);
    float* nb = na + Na;
#ifdef DDK_HOST_SANITIZE
    san::extent("manifold_members a", a, (long long)Na * D * 4); san::extent("manifold_members b", b, (long long)Nb * D * 4);
    san::extent("manifold_members ra", ra, (long long)Na * 4); san::extent("manifold_members rb", rb, (long long)Nb * 4);
    san::extent("manifold_members a_in", rb ? a_in : nullptr, Na); san::extent("manifold_members b_in", ra ? b_in : nullptr, Nb);
    san::extent("manifold_members norms", na, ((long long)Na + Nb) * 4);
#endif
    if (rb) DDK_HIP(hipMemsetAsync(a_in, 0, (size_t)Na, as_stream(s)));
    if (ra) DDK_HIP(hipMemsetAsync(b_in, 0, (size_t)Nb, as_stream(s)));
    DDK_TRY(mf_norms(a, Na, D, na, as_stream(s)));
    DDK_TRY(mf_norms(b, Nb, D, nb, as_stream(s)));
    int tps;
    const long long row_blocks = ceil_div(Na, MF_TILE), col_tiles = ceil_div(Nb, MF_TILE);
    const int splits = mf_col_splits(row_blocks, col_tiles, &tps);
    hipLaunchKernelGGL(mf_members_kernel, dim3((unsigned)row_blocks, (unsigned)splits), dim3(MF_THREADS), 0, as_stream(s), a, (const float*)na,
                       ra, Na, b, (const float*)nb, rb, Nb, D, (int)col_tiles, tps, a_in, b_in);
    return check_launch("mf_members_kernel");
}

size_t ddk_manifold_ball_counts_workspace_bytes(int Na, int Nb) { return ddk_manifold_members_workspace_bytes(Na, Nb); }

int ddk_manifold_ball_counts(const float* a, const float* ra, int Na, const float* b, int Nb, int D, int* counts, void* workspace,
                             size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(a && ra && b && counts, "manifold_ball_counts: null pointer");
    DDK_REQUIRE(mf_shape_ok(Na, D) && mf_shape_ok(Nb, D), "manifold_ball_counts: Na, Nb in 1..2^24, D positive and a multiple of 4");
    DDK_REQUIRE(aligned16(a) && aligned16(b), "manifold_ball_counts: a and b must be 16-byte aligned");
    DDK_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 3u) == 0, "manifold_ball_counts: counts must be 4-byte aligned");
    DDK_REQUIRE(workspace && workspace_bytes >= ddk_manifold_ball_counts_workspace_bytes(Na, Nb) && aligned16(workspace),
                "manifold_ball_counts: workspace (ddk_manifold_ball_counts_workspace_bytes, 16-byte aligned)");
    float* na = static_cast<float*>(workspace);
    float* nb = na + Na;
#ifdef DDK_HOST_SANITIZE
    san::extent("manifold_ball_counts a", a, (long long)Na * D * 4); san::extent("manifold_ball_counts b", b, (long long)Nb * D * 4);
    san::extent("manifold_ball_counts ra", ra, (long long)Na * 4); san::extent("manifold_ball_counts counts", counts, (long long)Na * 4);
    san::extent("manifold_ball_counts norms", na, ((long long)Na + Nb) * 4);
#endif
    DDK_HIP(hipMemsetAsync(counts, 0, (size_t)Na * sizeof(int), as_stream(s)));
    DDK_TRY(mf_norms(a, Na, D, na, as_stream(s)));
    DDK_TRY(mf_norms(b, Nb, D, nb, as_stream(s)));
    int tps;
    const long long row_blocks = ceil_div(Na, MF_TILE), col_tiles = ceil_div(Nb, MF_TILE);
    const int splits = mf_col_splits(row_blocks, col_tiles, &tps);
    hipLaunchKernelGGL(mf_ball_counts_kernel, dim3((unsigned)row_blocks, (unsigned)splits), dim3(MF_THREADS), 0, as_stream(s), a,
                       (const float*)na, ra, Na, b, (const float*)nb, Nb, D, (int)col_tiles, tps, counts);
    return check_launch("mf_ball_counts_kernel");
}

size_t ddk_poly_mmd_workspace_bytes(int S, int ma, int mb) {
    long long naa, nbb, nab;
    if (!mf_mmd_tiles(S, ma, mb, &naa, &nbb, &nab)) return 0;
    return (size_t)S * (size_t)(naa + nbb + nab) * sizeof(double);
}

int ddk_poly_mmd_sums(const float* a, const float* b, int S, int ma, int mb, int D, float gamma, float coef0, double* sums, void* workspace,
                      size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(a && b && sums, "poly_mmd_sums: null pointer");
    DDK_REQUIRE(D > 0 && D % 4 == 0, "poly_mmd_sums: D positive and a multiple of 4");
    DDK_REQUIRE(S >= 1 && ma >= 2 && mb >= 2, "poly_mmd_sums: S >= 1 segments of ma >= 2 and mb >= 2 rows");
    long long naa, nbb, nab;
    DDK_REQUIRE(mf_mmd_tiles(S, ma, mb, &naa, &nbb, &nab), "poly_mmd_sums: S ma and S mb must be at most 2^24 rows");
    DDK_REQUIRE(std::isfinite(gamma) && std::isfinite(coef0), "poly_mmd_sums: gamma and coef0 must be finite");
    DDK_REQUIRE(aligned16(a) && aligned16(b), "poly_mmd_sums: a and b must be 16-byte aligned");
    DDK_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7u) == 0, "poly_mmd_sums: sums must be 8-byte aligned");
    DDK_REQUIRE(workspace && workspace_bytes >= ddk_poly_mmd_workspace_bytes(S, ma, mb) && aligned16(workspace),
                "poly_mmd_sums: workspace (ddk_poly_mmd_workspace_bytes, 16-byte aligned)");
    const long long total = (long long)S * (naa + nbb + nab), outputs = 3ll * S;
    double* partials = static_cast<double*>(workspace);
#ifdef DDK_HOST_SANITIZE
    san::extent("poly_mmd_sums a", a, (long long)S * ma * D * 4); san::extent("poly_mmd_sums b", b, (long long)S * mb * D * 4);
    san::extent("poly_mmd_sums sums", sums, outputs * 8); san::extent("poly_mmd_sums partials", partials, total * 8);
#endif
    hipLaunchKernelGGL(mf_mmd_kernel, dim3((unsigned)std::min(total, MF_MAX_GRID)), dim3(MF_THREADS), 0, as_stream(s), a, b, ma, mb, D, gamma,
                       coef0, total, partials);
    DDK_TRY(check_launch("mf_mmd_kernel"));
    hipLaunchKernelGGL(mf_mmd_finish_kernel, dim3((unsigned)std::min(outputs, MF_MAX_GRID)), dim3(256), 0, as_stream(s),
                       (const double*)partials, outputs, naa, nbb, nab, sums);
    return check_launch("mf_mmd_finish_kernel");
}
}
