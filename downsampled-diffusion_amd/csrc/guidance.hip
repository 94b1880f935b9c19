// guidance.hip -- the device ops of Diffusion Posterior Sampling (Chung, Kim, Mccann, Klasky, Ye, "Diffusion posterior sampling for
// general noisy inverse problems", ICLR 2023): the measurement distance of an image and its adjoint, the clipped x0 of a step as a
// differentiable op, and the reverse-step update that also moves x against a gradient.  DESIGN.md section 3.22.
//
//   ddk_measure_residual       u = mask o (n x n block mean) of img, r = mask phi'(u) (phi(u) - y), dist[b] = sqrt(sum_b mask (phi(u) - y)^2)
//   ddk_measure_adjoint        v = s[b] r[b, i / n, j / n, c] / n^2,  s[b] = gout[b] / dist[b]  (0 where dist[b] == 0)
//   ddk_x0_from_eps (_bwd)     x0 = clamp(c_recip x - c_recipm1 eps, -1, 1) and its two input gradients
//   ddk_p_sample_update_guided the update of ddk_p_sample_update (p_step, diffusion_step.h), then x <- x - zeta[t] g
//
// The distance: every thread squares its own elements in fp32 and adds them in double; a workgroup adds its threads by the butterfly
// and its four waves by name; an image of more than MEASURE_SLICE elements is spread over slices whose sums measure_finish_kernel adds
// in index order.  No atomics and no arrival order anywhere: the same bits from run to run, and an image's sum is made of that image's
// elements only -- a NaN in one image stays in that image.
// Compiled with -ffp-contract=off like the other files that share diffusion_step.h (Makefile).
#include "ddk_internal.h"
#include "diffusion_step.h"

#include <climits>

namespace ddk {

constexpr int MEASURE_THREADS = 256;          // four waves: measure_block_sum adds their sums by name
constexpr int MEASURE_SLICE = 2048;           // measured elements per workgroup: 8 per thread
constexpr int MEASURE_MAX_SLICES = 64;        // one wave adds an image's slices, a lane each

static int measure_slices(long long m) {
    const long long ns = ceil_div(m, MEASURE_SLICE);
    return (int)(ns < 1 ? 1 : ns > MEASURE_MAX_SLICES ? MEASURE_MAX_SLICES : ns);
}

static int guide_grid(long long n) {
    const long long b = ceil_div(n > 0 ? n : 1, 256);
    return (int)(b < 2048 ? b : 2048);
}

__device__ __forceinline__ double measure_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum over the workgroup's MEASURE_THREADS threads, valid in thread 0
__device__ __forceinline__ double measure_block_sum(double v, double* red) {
    v = measure_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// phi and phi' of the response at the block mean u.  SATURATE: clamp(gain u, -1, 1), whose slope is gain where |gain u| <= 1 -- the
// bounds included, as torch's clamp backward has it -- and 0 elsewhere (also for a NaN, which phi itself keeps)
template <int RESPONSE>
__device__ __forceinline__ void measure_response(float u, float gain, float& phi, float& dphi) {
    if constexpr (RESPONSE == DDK_RESPONSE_SATURATE) {
        const float gu = __fmul_rn(gain, u);
        phi = clamp_pm1(gu);
        dphi = (gu >= -1.0f && gu <= 1.0f) ? gain : 0.0f;
    } else {
        phi = u;
        dphi = 1.0f;
    }
}

// workgroup = slice sl of image b (blockIdx.x = b * ns + sl): measured elements sl * 256 + tid, + ns * 256, ... of the image's
// m = h w C.  An element's block is summed in row-major order and scaled by the exact 1 / n^2.  Where the mask is 0 neither the
// block nor y is read: r is 0 and nothing enters the sum.  ns == 1: dist[b] is finished here; else the slice's sum goes to partials.
template <int RESPONSE>
__global__ __launch_bounds__(MEASURE_THREADS) void measure_residual_kernel(const float* __restrict__ img, const float* __restrict__ y,
                                                                           const float* __restrict__ mask, int n, float gain, int h, int w,
                                                                           int C, int ns, float* __restrict__ r, float* __restrict__ dist,
                                                                           double* __restrict__ partials) {
    __shared__ double red[MEASURE_THREADS / 64];
    const int b = blockIdx.x / ns, sl = blockIdx.x % ns;
    const long long m = (long long)h * w * C;
    const int W = w * n;
    const float* ib = img + (size_t)b * m * n * n;
    const float* yb = y + (size_t)b * m;
    const float* mb = mask ? mask + (size_t)b * h * w : nullptr;
    float* rb = r + (size_t)b * m;
    const float inv = 1.0f / (float)(n * n);
    double acc = 0.0;
    for (long long o = sl * (long long)MEASURE_THREADS + threadIdx.x; o < m; o += (long long)ns * MEASURE_THREADS) {
        const long long p = o / C;
        const int c = (int)(o - p * C), i = (int)(p / w), j = (int)(p - (long long)i * w);
        float res = 0.0f;
        if (!mb || mb[p] != 0.0f) {
            float sum = 0.0f;
            for (int di = 0; di < n; ++di) {
                const float* row = ib + ((size_t)(i * n + di) * W + (size_t)j * n) * C + c;
                for (int dj = 0; dj < n; ++dj) sum = __fadd_rn(sum, row[(size_t)dj * C]);
            }
            float phi, dphi;
            measure_response<RESPONSE>(__fmul_rn(sum, inv), gain, phi, dphi);
            const float d = __fsub_rn(phi, yb[o]);
            res = __fmul_rn(dphi, d);
            acc += (double)__fmul_rn(d, d);
        }
        rb[o] = res;
    }
    acc = measure_block_sum(acc, red);
    if (threadIdx.x == 0) {
        if (ns == 1) dist[b] = (float)sqrt(acc);
        else partials[blockIdx.x] = acc;
    }
}

// one wave per image: lane l holds slice l's sum (ns <= 64), the butterfly adds them
__global__ __launch_bounds__(64) void measure_finish_kernel(const double* __restrict__ partials, int ns, float* __restrict__ dist) {
    double s = (int)threadIdx.x < ns ? partials[(size_t)blockIdx.x * ns + threadIdx.x] : 0.0;
    s = measure_wave_sum(s);
    if (threadIdx.x == 0) dist[blockIdx.x] = (float)sqrt(s);
}

// v[b][i][j][c] = (s[b] r[b][i / n][j / n][c]) / n^2 over the B H W C elements of v
__global__ __launch_bounds__(256) void measure_adjoint_kernel(const float* __restrict__ r, const float* __restrict__ dist,
                                                              const float* __restrict__ gout, int n, int H, int W, int C, long long total,
                                                              float* __restrict__ v) {
    const int h = H / n, w = W / n;
    const long long per = (long long)H * W * C;
    const float inv = 1.0f / (float)(n * n);
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / per, q = e - b * per, p = q / C;
        const int c = (int)(q - p * C), i = (int)(p / W), j = (int)(p - (long long)i * W);
        const float db = dist[b];
        const float s = db == 0.0f ? 0.0f : gout[b] / db;
        const float rv = r[(((size_t)b * h + i / n) * w + j / n) * C + c];
        v[e] = __fmul_rn(__fmul_rn(s, rv), inv);
    }
}

template <bool CLIP>
__global__ __launch_bounds__(256) void x0_from_eps_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                          const int64_t* __restrict__ t, const float* __restrict__ c_recip,
                                                          const float* __restrict__ c_recipm1, long long per4, long long total4,
                                                          float* __restrict__ x0) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int64_t tb = t[i / per4];
        const float cr = c_recip[tb], crm1 = c_recipm1[tb];
        const float4 xv = reinterpret_cast<const float4*>(x)[i], ev = reinterpret_cast<const float4*>(eps)[i];
        auto f = [=](float xx, float ee) {
            return CLIP ? rst_x0(xx, ee, cr, crm1) : __fsub_rn(__fmul_rn(cr, xx), __fmul_rn(crm1, ee));
        };
        reinterpret_cast<float4*>(x0)[i] = make_float4(f(xv.x, ev.x), f(xv.y, ev.y), f(xv.z, ev.z), f(xv.w, ev.w));
    }
}

// dx = c_recip m dx0, deps = -c_recipm1 m dx0 with m = 1 where the unclipped x0 lies in [-1, 1] (bounds included), else 0
template <bool CLIP>
__global__ __launch_bounds__(256) void x0_from_eps_bwd_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                              const float* __restrict__ dx0, const int64_t* __restrict__ t,
                                                              const float* __restrict__ c_recip, const float* __restrict__ c_recipm1,
                                                              long long per4, long long total4, float* __restrict__ dx,
                                                              float* __restrict__ deps) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int64_t tb = t[i / per4];
        const float cr = c_recip[tb], crm1 = c_recipm1[tb];
        const float4 xv = reinterpret_cast<const float4*>(x)[i], ev = reinterpret_cast<const float4*>(eps)[i];
        const float4 gv = reinterpret_cast<const float4*>(dx0)[i];
        auto gate = [=](float xx, float ee, float g) {
            if (!CLIP) return g;
            const float raw = __fsub_rn(__fmul_rn(cr, xx), __fmul_rn(crm1, ee));
            return (raw >= -1.0f && raw <= 1.0f) ? g : 0.0f;
        };
        const float4 mg = make_float4(gate(xv.x, ev.x, gv.x), gate(xv.y, ev.y, gv.y), gate(xv.z, ev.z, gv.z), gate(xv.w, ev.w, gv.w));
        reinterpret_cast<float4*>(dx)[i] = make_float4(__fmul_rn(cr, mg.x), __fmul_rn(cr, mg.y), __fmul_rn(cr, mg.z), __fmul_rn(cr, mg.w));
        const float ncr = -crm1;
        reinterpret_cast<float4*>(deps)[i] = make_float4(__fmul_rn(ncr, mg.x), __fmul_rn(ncr, mg.y), __fmul_rn(ncr, mg.z), __fmul_rn(ncr, mg.w));
    }
}

// p_update_kernel<Ancestral>'s loop (diffusion.hip) -- the same row gather, the same draw of (i, t[b], stream, seed), the same p_step --
// and behind it x <- x - zeta[t[b]] g.  A row whose zeta is 0 takes no step at all: its result is p_step's, bit for bit, whatever g holds.
__global__ __launch_bounds__(256) void p_update_guided_kernel(float* __restrict__ x, const float* __restrict__ eps_hat,
                                                              const float* __restrict__ noise, const float* __restrict__ g,
                                                              const int64_t* __restrict__ t, const float* __restrict__ c_recip,
                                                              const float* __restrict__ c_recipm1, const float* __restrict__ c1,
                                                              const float* __restrict__ c2, const float* __restrict__ sigma,
                                                              const float* __restrict__ zeta, long long per4, long long total4, uint64_t seed,
                                                              uint32_t stream) {
    float4* __restrict__ xp = reinterpret_cast<float4*>(x);
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int64_t tb = t[i / per4];
        const float cr = c_recip[tb], crm1 = c_recipm1[tb], a1 = c1[tb], a2 = c2[tb], zt = zeta[tb];
        const float sg = tb > 0 ? sigma[tb] : 0.0f;
        const float4 xv = xp[i], ev = reinterpret_cast<const float4*>(eps_hat)[i], gv = reinterpret_cast<const float4*>(g)[i];
        const float4 zv = noise ? reinterpret_cast<const float4*>(noise)[i] : philox_normal4((unsigned long long)i, (uint32_t)tb, stream, seed);
        auto f = [=](float xx, float ee, float zz, float gg) {
            const float o = p_step(xx, ee, zz, cr, crm1, a1, a2, sg);
            return zt != 0.0f ? __fsub_rn(o, __fmul_rn(zt, gg)) : o;
        };
        xp[i] = make_float4(f(xv.x, ev.x, zv.x, gv.x), f(xv.y, ev.y, zv.y, gv.y), f(xv.z, ev.z, zv.z, gv.z), f(xv.w, ev.w, zv.w, gv.w));
    }
}

// the shape both measurement entries take: n in {1, 2, 4, 8} dividing H and W, every count within one launch
static const char* measure_shape_fault(int B, int H, int W, int C, int n) {
    if (!(B > 0 && H > 0 && W > 0 && C > 0)) return "B / H / W / C must be positive";
    if (!(n == 1 || n == 2 || n == 4 || n == 8)) return "n must be 1, 2, 4 or 8";
    if (H % n || W % n) return "n must divide H and W";
    if ((long long)H * W * C > INT32_MAX) return "too many elements per image";      // (the kernels index within an image in int)
    if ((long long)B * MEASURE_MAX_SLICES > INT32_MAX) return "too many images for one launch";
    return nullptr;
}

}  // namespace ddk

using namespace ddk;

extern "C" {

size_t ddk_measure_residual_workspace_bytes(int B, int H, int W, int C, int n) {
    if (measure_shape_fault(B, H, W, C, n)) return 0;
    const int ns = measure_slices((long long)(H / n) * (W / n) * C);
    return ns == 1 ? 0 : (size_t)B * ns * sizeof(double);
}

int ddk_measure_residual(const float* img, const float* y, const float* mask, int n, int response, float gain, float* r, float* dist,
                         int B, int H, int W, int C, void* workspace, size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(img && y && r && dist, "measure_residual: null pointer");
    if (const char* fault = measure_shape_fault(B, H, W, C, n)) {
        set_error("bad argument: measure_residual: %s", fault);
        return DDK_ERR_ARG;
    }
    DDK_REQUIRE(response == DDK_RESPONSE_LINEAR || response == DDK_RESPONSE_SATURATE, "measure_residual: response must be LINEAR or SATURATE");
    DDK_REQUIRE(response == DDK_RESPONSE_LINEAR || (gain == gain && gain > 0.0f && gain <= 3.0e38f), "measure_residual: gain must be finite and > 0");
    const int h = H / n, w = W / n;
    const int ns = measure_slices((long long)h * w * C);
    const size_t need = ddk_measure_residual_workspace_bytes(B, H, W, C, n);
    DDK_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0),
                "measure_residual: workspace (ddk_measure_residual_workspace_bytes)");
    double* partials = need ? static_cast<double*>(workspace) : nullptr;
    const dim3 grid((unsigned)(B * ns));
    if (response == DDK_RESPONSE_SATURATE)
        hipLaunchKernelGGL(measure_residual_kernel<DDK_RESPONSE_SATURATE>, grid, dim3(MEASURE_THREADS), 0, as_stream(s), img, y, mask, n, gain, h,
                           w, C, ns, r, dist, partials);
    else
        hipLaunchKernelGGL(measure_residual_kernel<DDK_RESPONSE_LINEAR>, grid, dim3(MEASURE_THREADS), 0, as_stream(s), img, y, mask, n, gain, h, w,
                           C, ns, r, dist, partials);
    DDK_TRY(check_launch("measure_residual_kernel"));
    if (ns == 1) return DDK_OK;
    hipLaunchKernelGGL(measure_finish_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(s), (const double*)partials, ns, dist);
    return check_launch("measure_finish_kernel");
}

int ddk_measure_adjoint(const float* r, const float* dist, const float* gout, int n, float* v, int B, int H, int W, int C, ddk_stream_t s) {
    DDK_REQUIRE(r && dist && gout && v, "measure_adjoint: null pointer");
    if (const char* fault = measure_shape_fault(B, H, W, C, n)) {
        set_error("bad argument: measure_adjoint: %s", fault);
        return DDK_ERR_ARG;
    }
    const long long total = (long long)B * H * W * C;
    hipLaunchKernelGGL(measure_adjoint_kernel, dim3(guide_grid(total)), dim3(256), 0, as_stream(s), r, dist, gout, n, H, W, C, total, v);
    return check_launch("measure_adjoint_kernel");
}

int ddk_x0_from_eps(const float* x, const float* eps, const int64_t* t, const float* c_recip, const float* c_recipm1, int clip, float* x0,
                    int B, long long per, ddk_stream_t s) {
    DDK_REQUIRE(x && eps && t && c_recip && c_recipm1 && x0, "x0_from_eps: null pointer");
    DDK_REQUIRE(B > 0 && per > 0 && per % 4 == 0, "x0_from_eps: per-sample element count must be a multiple of 4");
    DDK_REQUIRE(aligned16(x) && aligned16(eps) && aligned16(x0), "x0_from_eps: alignment");
    const long long total4 = B * per / 4;
    if (clip)
        hipLaunchKernelGGL(x0_from_eps_kernel<true>, dim3(guide_grid(total4)), dim3(256), 0, as_stream(s), x, eps, t, c_recip, c_recipm1, per / 4,
                           total4, x0);
    else
        hipLaunchKernelGGL(x0_from_eps_kernel<false>, dim3(guide_grid(total4)), dim3(256), 0, as_stream(s), x, eps, t, c_recip, c_recipm1, per / 4,
                           total4, x0);
    return check_launch("x0_from_eps_kernel");
}

int ddk_x0_from_eps_bwd(const float* x, const float* eps, const float* dx0, const int64_t* t, const float* c_recip, const float* c_recipm1,
                        int clip, float* dx, float* deps, int B, long long per, ddk_stream_t s) {
    DDK_REQUIRE(x && eps && dx0 && t && c_recip && c_recipm1 && dx && deps, "x0_from_eps_bwd: null pointer");
    DDK_REQUIRE(B > 0 && per > 0 && per % 4 == 0, "x0_from_eps_bwd: per-sample element count must be a multiple of 4");
    DDK_REQUIRE(aligned16(x) && aligned16(eps) && aligned16(dx0) && aligned16(dx) && aligned16(deps), "x0_from_eps_bwd: alignment");
    const long long total4 = B * per / 4;
    if (clip)
        hipLaunchKernelGGL(x0_from_eps_bwd_kernel<true>, dim3(guide_grid(total4)), dim3(256), 0, as_stream(s), x, eps, dx0, t, c_recip, c_recipm1,
                           per / 4, total4, dx, deps);
    else
        hipLaunchKernelGGL(x0_from_eps_bwd_kernel<false>, dim3(guide_grid(total4)), dim3(256), 0, as_stream(s), x, eps, dx0, t, c_recip, c_recipm1,
                           per / 4, total4, dx, deps);
    return check_launch("x0_from_eps_bwd_kernel");
}

int ddk_p_sample_update_guided(float* x, const float* eps_hat, const float* noise, const float* g, const int64_t* t, const float* c_recip,
                               const float* c_recipm1, const float* c1, const float* c2, const float* sigma, const float* zeta, int B,
                               long long per, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    DDK_REQUIRE(x && eps_hat && g && t && c_recip && c_recipm1 && c1 && c2 && sigma && zeta, "p_sample_update_guided: null pointer");
    DDK_REQUIRE(B > 0 && per > 0 && per % 4 == 0, "p_sample_update_guided: per-sample element count must be a multiple of 4");
    DDK_REQUIRE(aligned16(x) && aligned16(eps_hat) && aligned16(noise) && aligned16(g), "p_sample_update_guided: alignment");
    const long long total4 = B * per / 4;
    hipLaunchKernelGGL(p_update_guided_kernel, dim3(guide_grid(total4)), dim3(256), 0, as_stream(s), x, eps_hat, noise, g, t, c_recip, c_recipm1,
                       c1, c2, sigma, zeta, per / 4, total4, seed, stream_id);
    return check_launch("p_update_guided_kernel");
}

}  // extern "C"
