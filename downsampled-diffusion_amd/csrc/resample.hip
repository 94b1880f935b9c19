// resample.hip -- the dDDPM's 'deterministic' and 'convolutional' resamplers (reference models/downsampled/convblocks.py:8-89,
// wrapper.py:22-26,49-55) and their gradients, on NCHW planes with 1..32 channels.  fp32, memory-bound, coalesced along W.
//
//   bicubic resize (F.interpolate(mode='bicubic', align_corners=True)): the caller hands per-output-index tap tables (4 indices,
//     4 weights per row and per column, built on the host in float64); one launch does the 2-D resize, 16 taps per output, rows
//     outer, columns inner.  Its input gradient is the transpose in gather form: per input row / column a list of (output
//     index, weight) pairs, again built on the host, so every input element sums its outputs in a fixed order.
//   Conv2d(k3, s2, p1) and ConvTranspose2d(k4, s2, p1): one thread per output pixel computing every output channel, eight at a
//     time, the filter in LDS as [c_in][tap][c_out].  Two kernels cover forward and input gradient of both layers:
//       strided_conv_kernel<K>   out[o] = sum_k in[2 o - 1 + k] w[co][ci][k]     K = 3: the conv, K = 4: the transpose conv's input gradient
//       transposed_conv_kernel<K> out[o] = sum_k in[(o + 1 - k) / 2] w[ci][co][k]  K = 4: the transpose conv, K = 3: the conv's input gradient
//   Weight and bias gradients: per-workgroup partial sums over a chunk of B x H x W, then a finish that adds the chunks in order.
// No atomics anywhere: every result is bit-stable from run to run.
#include "ddk_internal.h"

namespace ddk {

static inline unsigned blocks_for(long long total, int per_block) { return (unsigned)ceil_div(total, per_block); }

// ------------------------------------------------------------------------------------------------ bicubic
__global__ __launch_bounds__(256) void bicubic_resize_kernel(const float* __restrict__ x, float* __restrict__ out, const int4* __restrict__ ih,
                                                             const float4* __restrict__ wh, const int4* __restrict__ iw,
                                                             const float4* __restrict__ ww, int Hin, int Win, int Hout, int Wout,
                                                             long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % Wout);
    const long long r = idx / Wout;
    const int oy = (int)(r % Hout);
    const long long plane = r / Hout;
    const int4 ri = ih[oy], ci = iw[ox];
    const float4 rw = wh[oy], cw = ww[ox];
    const float* p = x + plane * Hin * Win;
    const int rows[4] = {ri.x, ri.y, ri.z, ri.w}, cols[4] = {ci.x, ci.y, ci.z, ci.w};
    const float rwt[4] = {rw.x, rw.y, rw.z, rw.w}, cwt[4] = {cw.x, cw.y, cw.z, cw.w};
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float* row = p + (long long)rows[a] * Win;
#pragma unroll
        for (int b = 0; b < 4; ++b) acc = fmaf(rwt[a] * cwt[b], row[cols[b]], acc);
    }
    out[idx] = acc;
}

// The same resize when it enlarges a small plane (the decoder: 32x32 -> 256x256): every source element is tapped dozens of times, so
// a workgroup first stages its whole source plane (<= 16 KiB) in LDS and gathers from there -- 16 LDS reads per output instead
// of 16 reads through the texture path, which bounded the kernel at 1/7 of the rate its 25 MB of output can be written at.
// Same taps in the same order: the results are bit-identical to bicubic_resize_kernel's.
constexpr int BICUBIC_LDS_FLOATS = 4096;      // largest staged source plane
constexpr int BICUBIC_LDS_PER_WG = 2048;      // outputs per workgroup (8 per thread)
__global__ __launch_bounds__(256) void bicubic_resize_lds_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                 const int4* __restrict__ ih, const float4* __restrict__ wh,
                                                                 const int4* __restrict__ iw, const float4* __restrict__ ww, int Hin, int Win,
                                                                 int Hout, int Wout) {
    __shared__ float sp[BICUBIC_LDS_FLOATS];
    const long long plane = blockIdx.y;
    const int n_in = Hin * Win, n_out = Hout * Wout;
    const float* p = x + plane * n_in;
    for (int i = threadIdx.x; i < n_in; i += 256) sp[i] = p[i];
    __syncthreads();
    const int o0 = blockIdx.x * BICUBIC_LDS_PER_WG;
    const int o1 = o0 + BICUBIC_LDS_PER_WG < n_out ? o0 + BICUBIC_LDS_PER_WG : n_out;
    for (int o = o0 + threadIdx.x; o < o1; o += 256) {
        const int oy = o / Wout, ox = o - oy * Wout;
        const int4 ri = ih[oy], ci = iw[ox];
        const float4 rw = wh[oy], cw = ww[ox];
        const int rows[4] = {ri.x, ri.y, ri.z, ri.w}, cols[4] = {ci.x, ci.y, ci.z, ci.w};
        const float rwt[4] = {rw.x, rw.y, rw.z, rw.w}, cwt[4] = {cw.x, cw.y, cw.z, cw.w};
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float* row = sp + rows[a] * Win;
#pragma unroll
            for (int b = 0; b < 4; ++b) acc = fmaf(rwt[a] * cwt[b], row[cols[b]], acc);
        }
        out[plane * n_out + o] = acc;
    }
}

// dx[plane][iy][ix] = sum over the outputs that tap (iy, ix): rows hs[iy] .. hs[iy+1] of (ho, hw), columns likewise.
// S lanes share one input element: lane s takes the columns c0 + s, c0 + s + S, ... of every row, and the S partial sums meet in a
// butterfly of shuffles -- a fixed order, like the loops.  S = 1 when the lists are short (the gradient of a downsizing resize: an
// input column lies under one or two outputs), S = 16 when they are long (the gradient of the 32 -> 256 decoder: ~32 x 32 terms per
// input element, which one lane would walk as 1024 dependent gathers).
template <int S>
__global__ __launch_bounds__(256) void bicubic_resize_grad_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                  const int* __restrict__ hs, const int* __restrict__ ho,
                                                                  const float* __restrict__ hw, const int* __restrict__ ws,
                                                                  const int* __restrict__ wo, const float* __restrict__ wwt, int Hin,
                                                                  int Win, int Hout, int Wout, long long total) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long idx = tid / S;
    const int sub = (int)(tid % S);
    const bool live = idx < total;              // the lanes of a group leave together: idx is the same for all S of them
    float acc = 0.f;
    if (live) {
        const int ix = (int)(idx % Win);
        const long long r = idx / Win;
        const int iy = (int)(r % Hin);
        const long long plane = r / Hin;
        const float* p = dy + plane * Hout * Wout;
        const int r0 = hs[iy], r1 = hs[iy + 1], c0 = ws[ix], c1 = ws[ix + 1];
        for (int a = r0; a < r1; ++a) {
            const float* row = p + (long long)ho[a] * Wout;
            const float wa = hw[a];
            for (int b = c0 + sub; b < c1; b += S) acc = fmaf(wa * wwt[b], row[wo[b]], acc);
        }
    }
#pragma unroll
    for (int o = S / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (live && sub == 0) dx[idx] = acc;
}

// ------------------------------------------------------------------------------------------------ small-channel stride-2 convs
constexpr int CO_T = 8;      // output channels per pass of a thread

// stage w (global [A][Bc][KK], A = the filter's leading dimension) into LDS as [ci][k][cop], zero beyond cout.
// LEAD_OUT: the leading dimension is the output channel (nn.Conv2d, OIHW); otherwise the input channel (nn.ConvTranspose2d, IOHW)
template <bool LEAD_OUT>
__device__ __forceinline__ void stage_filter(const float* __restrict__ w, float* sw, int cin, int cout, int cop, int KK) {
    const int n = cin * KK * cop;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int co = i % cop, rk = i / cop, k = rk % KK, ci = rk / KK;
        float v = 0.f;
        if (co < cout) v = LEAD_OUT ? w[((long long)co * cin + ci) * KK + k] : w[((long long)ci * cout + co) * KK + k];
        sw[i] = v;
    }
    __syncthreads();
}

// out[b][co][oy][ox] = bias[co] + sum_{ci, ky, kx} x[b][ci][2 oy - 1 + ky][2 ox - 1 + kx] w[co][ci][ky][kx]   (zero padding)
template <int K>
__global__ __launch_bounds__(256) void strided_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out, int cin, int cout,
                                                           int cop, int H, int W, int Ho, int Wo, long long total) {
    extern __shared__ float sw[];
    stage_filter<true>(w, sw, cin, cout, cop, K * K);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % Wo);
    const long long r = idx / Wo;
    const int oy = (int)(r % Ho);
    const long long b = r / Ho;
    const int iy0 = 2 * oy - 1, ix0 = 2 * ox - 1;
    const long long in_plane = (long long)H * W, out_plane = (long long)Ho * Wo;
    for (int c0 = 0; c0 < cout; c0 += CO_T) {
        float acc[CO_T];
#pragma unroll
        for (int j = 0; j < CO_T; ++j) acc[j] = (bias && c0 + j < cout) ? bias[c0 + j] : 0.f;
        for (int ci = 0; ci < cin; ++ci) {
            const float* xp = x + (b * cin + ci) * in_plane;
            const float* wp = sw + (long long)ci * K * K * cop + c0;
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const int iy = iy0 + ky;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int ix = ix0 + kx;
                    const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
                    const float v = in ? xp[(long long)iy * W + ix] : 0.f;
                    const float* wk = wp + (ky * K + kx) * cop;
#pragma unroll
                    for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(v, wk[j], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CO_T; ++j)
            if (c0 + j < cout) out[(b * cout + c0 + j) * out_plane + (long long)oy * Wo + ox] = acc[j];
    }
}

// out[b][co][oy][ox] = bias[co] + sum_{ci, ky, kx : oy + 1 - ky = 2 iy, ox + 1 - kx = 2 ix} x[b][ci][iy][ix] w[ci][co][ky][kx]
// (x is [H][W], out is [Ho][Wo]; per dimension the taps are ky = (oy + 1) % 2 + 2 t, t = 0, 1, with iy = (oy + 1 - ky) / 2)
template <int K>
__global__ __launch_bounds__(256) void transposed_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ out, int cin, int cout,
                                                              int cop, int H, int W, int Ho, int Wo, long long total) {
    extern __shared__ float sw[];
    stage_filter<false>(w, sw, cin, cout, cop, K * K);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % Wo);
    const long long r = idx / Wo;
    const int oy = (int)(r % Ho);
    const long long b = r / Ho;
    int ky[2], kx[2], iy[2], ix[2];
    bool vy[2], vx[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        ky[t] = ((oy + 1) & 1) + 2 * t;
        kx[t] = ((ox + 1) & 1) + 2 * t;
        iy[t] = (oy + 1 - ky[t]) >> 1;      // exact: the numerator is even (and >= -2, an arithmetic shift)
        ix[t] = (ox + 1 - kx[t]) >> 1;
        vy[t] = ky[t] < K && iy[t] >= 0 && iy[t] < H;
        vx[t] = kx[t] < K && ix[t] >= 0 && ix[t] < W;
    }
    const long long in_plane = (long long)H * W, out_plane = (long long)Ho * Wo;
    for (int c0 = 0; c0 < cout; c0 += CO_T) {
        float acc[CO_T];
#pragma unroll
        for (int j = 0; j < CO_T; ++j) acc[j] = (bias && c0 + j < cout) ? bias[c0 + j] : 0.f;
        for (int ci = 0; ci < cin; ++ci) {
            const float* xp = x + (b * cin + ci) * in_plane;
            const float* wp = sw + (long long)ci * K * K * cop + c0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const bool in = vy[a] && vx[c];
                    const float v = in ? xp[(long long)iy[a] * W + ix[c]] : 0.f;
                    const float* wk = wp + (in ? (ky[a] * K + kx[c]) * cop : 0);
#pragma unroll
                    for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(v, wk[j], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CO_T; ++j)
            if (c0 + j < cout) out[(b * cout + c0 + j) * out_plane + (long long)oy * Wo + ox] = acc[j];
    }
}

static inline int pad_co(int c) { return (c + CO_T - 1) / CO_T * CO_T; }

template <int K>
static int launch_strided(const char* who, const float* x, const float* w, const float* bias, float* out, int B, int cin, int cout, int H,
                          int W, int Ho, int Wo, hipStream_t st) {
    const long long total = (long long)B * Ho * Wo;
    const int cop = pad_co(cout);
    const size_t lds = (size_t)cin * K * K * cop * sizeof(float);
    hipLaunchKernelGGL((strided_conv_kernel<K>), dim3(blocks_for(total, 256)), dim3(256), lds, st, x, w, bias, out, cin, cout, cop, H, W, Ho,
                       Wo, total);
    return check_launch(who);
}

template <int K>
static int launch_transposed(const char* who, const float* x, const float* w, const float* bias, float* out, int B, int cin, int cout,
                             int H, int W, int Ho, int Wo, hipStream_t st) {
    const long long total = (long long)B * Ho * Wo;
    const int cop = pad_co(cout);
    const size_t lds = (size_t)cin * K * K * cop * sizeof(float);
    hipLaunchKernelGGL((transposed_conv_kernel<K>), dim3(blocks_for(total, 256)), dim3(256), lds, st, x, w, bias, out, cin, cout, cop, H, W,
                       Ho, Wo, total);
    return check_launch(who);
}

// ------------------------------------------------------------------------------------------------ weight / bias gradients
// g[cs][cl][ky][kx] = sum_{b, y, x} s[b][cs][y][x] * l[b][cl][2 y - 1 + ky][2 x - 1 + kx]      (s: [Hs][Ws], l: [Hl][Wl], zero outside)
//   the conv:            s = dy, l = x   -> g = dW (OIHW),  bias gradient = sum of s          (BIAS_S)
//   the transpose conv:  s = x,  l = dy  -> g = dW (IOHW),  bias gradient = sum of l, taken over the taps (1..2, 1..2): with
//                        Hl = 2 Hs they tile l exactly once                                   (BIAS_L, K = 4 only)
// Stage 1: workgroup (chunk, pair = cs * Cl + cl) sums its chunk of the B x Hs x Ws positions: K*K + 1 values to
// part[pair][chunk][K*K + 1].  Stage 2 adds the chunks in order.
constexpr int BIAS_S = 1, BIAS_L = 2;
constexpr int WG_POS = 4096;         // positions per chunk aimed at (16 per thread)
constexpr int WG_MAX_CHUNKS = 256;

static inline int wgrad_chunks(long long positions) {
    const long long n = ceil_div(positions, WG_POS);
    return (int)(n < 1 ? 1 : n > WG_MAX_CHUNKS ? WG_MAX_CHUNKS : n);
}

template <int K>
__global__ __launch_bounds__(256) void small_wgrad_partial_kernel(const float* __restrict__ s, const float* __restrict__ l,
                                                                  float* __restrict__ part, int Cs, int Cl, int Hs, int Ws, int Hl, int Wl,
                                                                  long long positions, long long per_chunk, int bias_mode) {
    __shared__ float red[32];
    constexpr int KK = K * K;
    const int chunk = blockIdx.x, nchunks = gridDim.x, pair = blockIdx.y;
    const int cs = pair / Cl, cl = pair - cs * Cl;
    const long long p0 = chunk * per_chunk;
    const long long p1 = p0 + per_chunk < positions ? p0 + per_chunk : positions;
    const long long s_plane = (long long)Hs * Ws, l_plane = (long long)Hl * Wl;
    float acc[KK], bacc = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[k] = 0.f;
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
        const int x = (int)(p % Ws);
        const long long r = p / Ws;
        const int y = (int)(r % Hs);
        const long long b = r / Hs;
        const float sv = s[(b * Cs + cs) * s_plane + (long long)y * Ws + x];
        const float* lp = l + (b * Cl + cl) * l_plane;
        if (bias_mode == BIAS_S) bacc += sv;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int ly = 2 * y - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int lx = 2 * x - 1 + kx;
                const bool in = ly >= 0 && ly < Hl && lx >= 0 && lx < Wl;
                const float lv = in ? lp[(long long)ly * Wl + lx] : 0.f;
                acc[ky * K + kx] = fmaf(sv, lv, acc[ky * K + kx]);
                if (K == 4 && bias_mode == BIAS_L && (ky == 1 || ky == 2) && (kx == 1 || kx == 2)) bacc += lv;
            }
        }
    }
    float* dst = part + ((long long)pair * nchunks + chunk) * (KK + 1);
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const float v = block_sum(acc[k], red);
        if (threadIdx.x == 0) dst[k] = v;
    }
    const float bv = block_sum(bacc, red);
    if (threadIdx.x == 0) dst[KK] = bv;
}

// g[pair][k] = sum over the chunks in order; the bias gradient from the pairs (c, 0) (BIAS_S) or (0, c) (BIAS_L)
__global__ __launch_bounds__(256) void small_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ g, float* __restrict__ gb,
                                                                 int Cs, int Cl, int KK, int nchunks, int bias_mode) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nw = Cs * Cl * KK;
    const int nb = bias_mode == BIAS_S ? Cs : bias_mode == BIAS_L ? Cl : 0;
    if (idx >= nw + nb) return;
    long long pair;
    int k;
    if (idx < nw) {
        pair = idx / KK;
        k = idx - (int)pair * KK;
    } else {
        const int c = idx - nw;
        pair = bias_mode == BIAS_S ? (long long)c * Cl : c;
        k = KK;
    }
    const float* src = part + pair * nchunks * (KK + 1) + k;
    float acc = 0.f;
    for (int c = 0; c < nchunks; ++c) acc += src[(long long)c * (KK + 1)];
    if (idx < nw) g[idx] = acc;
    else gb[idx - nw] = acc;
}

static size_t small_wgrad_ws_bytes(int B, int Cs, int Cl, int Hs, int Ws, int K) {
    return (size_t)Cs * Cl * wgrad_chunks((long long)B * Hs * Ws) * (K * K + 1) * sizeof(float);
}

template <int K>
static int small_wgrad(const char* who, const float* s, const float* l, float* g, float* gb, int B, int Cs, int Cl, int Hs, int Ws, int Hl,
                       int Wl, int bias_mode, void* ws, size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < small_wgrad_ws_bytes(B, Cs, Cl, Hs, Ws, K)) return fail_arg("small wgrad: workspace too small");
    const long long positions = (long long)B * Hs * Ws;
    const int nchunks = wgrad_chunks(positions);
    const long long per_chunk = ceil_div(positions, nchunks);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL((small_wgrad_partial_kernel<K>), dim3(nchunks, Cs * Cl), dim3(256), 0, st, s, l, part, Cs, Cl, Hs, Ws, Hl, Wl, positions,
                       per_chunk, gb ? bias_mode : 0);
    DDK_TRY(check_launch(who));
    const int n = Cs * Cl * K * K + (gb ? (bias_mode == BIAS_S ? Cs : Cl) : 0);
    hipLaunchKernelGGL(small_wgrad_finish_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, part, g, gb, Cs, Cl, K * K, nchunks,
                       gb ? bias_mode : 0);
    return check_launch("small_wgrad_finish_kernel");
}

static inline bool chan_ok(int c) { return c >= 1 && c <= 32; }
static inline bool fits31(long long v) { return v > 0 && v < (1LL << 31); }

}  // namespace ddk

using namespace ddk;

extern "C" {

int ddk_bicubic_resize(const float* x, float* out, const int* idx_h, const float* w_h, const int* idx_w, const float* w_w, long long planes,
                       int Hin, int Win, int Hout, int Wout, ddk_stream_t s) {
    DDK_REQUIRE(x && out && idx_h && w_h && idx_w && w_w, "bicubic_resize: null pointer");
    DDK_REQUIRE(planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "bicubic_resize: sizes");
    DDK_REQUIRE(aligned16(idx_h) && aligned16(w_h) && aligned16(idx_w) && aligned16(w_w), "bicubic_resize: tap tables must be 16-byte aligned");
    const long long total = planes * Hout * Wout;
    DDK_REQUIRE(fits31(ceil_div(total, 256)) && fits31(planes * Hin * Win / 256 + 1), "bicubic_resize: too many elements");
    const int4* ih = reinterpret_cast<const int4*>(idx_h);
    const int4* iw = reinterpret_cast<const int4*>(idx_w);
    const float4* wh = reinterpret_cast<const float4*>(w_h);
    const float4* ww = reinterpret_cast<const float4*>(w_w);
    const long long n_in = (long long)Hin * Win, n_out = (long long)Hout * Wout;
    if (n_in <= BICUBIC_LDS_FLOATS && n_out >= 4 * n_in && n_out < (1LL << 30) && planes <= 65535) {
        hipLaunchKernelGGL(bicubic_resize_lds_kernel, dim3(blocks_for(n_out, BICUBIC_LDS_PER_WG), (unsigned)planes), dim3(256), 0, as_stream(s), x,
                           out, ih, wh, iw, ww, Hin, Win, Hout, Wout);
        return check_launch("bicubic_resize_lds_kernel");
    }
    hipLaunchKernelGGL(bicubic_resize_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, as_stream(s), x, out, ih, wh, iw, ww, Hin, Win, Hout,
                       Wout, total);
    return check_launch("bicubic_resize_kernel");
}

int ddk_bicubic_resize_grad(const float* dy, float* dx, const int* start_h, const int* out_h, const float* w_h, const int* start_w,
                            const int* out_w, const float* w_w, int longest_w, long long planes, int Hin, int Win, int Hout, int Wout,
                            ddk_stream_t s) {
    DDK_REQUIRE(dy && dx && start_h && out_h && w_h && start_w && out_w && w_w, "bicubic_resize_grad: null pointer");
    DDK_REQUIRE(planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && longest_w >= 0, "bicubic_resize_grad: sizes");
    const long long total = planes * Hin * Win;
    DDK_REQUIRE(fits31(ceil_div(total, 256 / 16)) && fits31(planes * Hout * Wout / 256 + 1), "bicubic_resize_grad: too many elements");
    // longest_w only chooses how many lanes share an element; any value gives the same sums up to their order
    if (longest_w > 8)
        hipLaunchKernelGGL((bicubic_resize_grad_kernel<16>), dim3(blocks_for(total * 16, 256)), dim3(256), 0, as_stream(s), dy, dx, start_h, out_h,
                           w_h, start_w, out_w, w_w, Hin, Win, Hout, Wout, total);
    else
        hipLaunchKernelGGL((bicubic_resize_grad_kernel<1>), dim3(blocks_for(total, 256)), dim3(256), 0, as_stream(s), dy, dx, start_h, out_h, w_h,
                           start_w, out_w, w_w, Hin, Win, Hout, Wout, total);
    return check_launch("bicubic_resize_grad_kernel");
}

int ddk_conv_small_s2(const float* x, const float* w, const float* bias, float* out, int B, int cin, int cout, int H, int W, ddk_stream_t s) {
    DDK_REQUIRE(x && w && out, "conv_small_s2: null pointer");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && chan_ok(cin) && chan_ok(cout), "conv_small_s2: sizes (1 <= channels <= 32)");
    DDK_REQUIRE(fits31((long long)B * H * W), "conv_small_s2: 2^31 pixels or more");
    return launch_strided<3>("conv_small_s2", x, w, bias, out, B, cin, cout, H, W, (H + 1) / 2, (W + 1) / 2, as_stream(s));
}

int ddk_conv_small_s2_dgrad(const float* dy, const float* w, float* dx, int B, int cin, int cout, int H, int W, ddk_stream_t s) {
    DDK_REQUIRE(dy && w && dx, "conv_small_s2_dgrad: null pointer");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && chan_ok(cin) && chan_ok(cout), "conv_small_s2_dgrad: sizes (1 <= channels <= 32)");
    DDK_REQUIRE(fits31((long long)B * H * W), "conv_small_s2_dgrad: 2^31 pixels or more");
    // dy [B][cout][ceil(H/2)][ceil(W/2)] -> dx [B][cin][H][W]; w is the conv's OIHW tensor = [in of this gather][out][3][3]
    return launch_transposed<3>("conv_small_s2_dgrad", dy, w, nullptr, dx, B, cout, cin, (H + 1) / 2, (W + 1) / 2, H, W, as_stream(s));
}

size_t ddk_conv_small_s2_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !chan_ok(cin) || !chan_ok(cout)) return 0;
    return small_wgrad_ws_bytes(B, cout, cin, (H + 1) / 2, (W + 1) / 2, 3);
}

int ddk_conv_small_s2_wgrad(const float* x, const float* dy, float* dw, float* db, int B, int cin, int cout, int H, int W, void* workspace,
                            size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(x && dy && dw && workspace, "conv_small_s2_wgrad: null pointer");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && chan_ok(cin) && chan_ok(cout), "conv_small_s2_wgrad: sizes (1 <= channels <= 32)");
    DDK_REQUIRE(fits31((long long)B * H * W), "conv_small_s2_wgrad: 2^31 pixels or more");
    return small_wgrad<3>("conv_small_s2_wgrad", dy, x, dw, db, B, cout, cin, (H + 1) / 2, (W + 1) / 2, H, W, BIAS_S, workspace,
                          workspace_bytes, as_stream(s));
}

int ddk_convt_small_s2(const float* x, const float* w, const float* bias, float* out, int B, int cin, int cout, int H, int W, ddk_stream_t s) {
    DDK_REQUIRE(x && w && out, "convt_small_s2: null pointer");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && chan_ok(cin) && chan_ok(cout), "convt_small_s2: sizes (1 <= channels <= 32)");
    DDK_REQUIRE(fits31(4LL * B * H * W), "convt_small_s2: 2^31 pixels or more");
    return launch_transposed<4>("convt_small_s2", x, w, bias, out, B, cin, cout, H, W, 2 * H, 2 * W, as_stream(s));
}

int ddk_convt_small_s2_dgrad(const float* dy, const float* w, float* dx, int B, int cin, int cout, int H, int W, ddk_stream_t s) {
    DDK_REQUIRE(dy && w && dx, "convt_small_s2_dgrad: null pointer");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && chan_ok(cin) && chan_ok(cout), "convt_small_s2_dgrad: sizes (1 <= channels <= 32)");
    DDK_REQUIRE(fits31(4LL * B * H * W), "convt_small_s2_dgrad: 2^31 pixels or more");
    // dy [B][cout][2H][2W] -> dx [B][cin][H][W]; w is the layer's IOHW tensor = [out of this conv][in][4][4]
    return launch_strided<4>("convt_small_s2_dgrad", dy, w, nullptr, dx, B, cout, cin, 2 * H, 2 * W, H, W, as_stream(s));
}

size_t ddk_convt_small_s2_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !chan_ok(cin) || !chan_ok(cout)) return 0;
    return small_wgrad_ws_bytes(B, cin, cout, H, W, 4);
}

int ddk_convt_small_s2_wgrad(const float* x, const float* dy, float* dw, float* db, int B, int cin, int cout, int H, int W, void* workspace,
                             size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(x && dy && dw && workspace, "convt_small_s2_wgrad: null pointer");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0 && chan_ok(cin) && chan_ok(cout), "convt_small_s2_wgrad: sizes (1 <= channels <= 32)");
    DDK_REQUIRE(fits31(4LL * B * H * W), "convt_small_s2_wgrad: 2^31 pixels or more");
    return small_wgrad<4>("convt_small_s2_wgrad", x, dy, dw, db, B, cin, cout, H, W, 2 * H, 2 * W, BIAS_L, workspace, workspace_bytes,
                          as_stream(s));
}
}
