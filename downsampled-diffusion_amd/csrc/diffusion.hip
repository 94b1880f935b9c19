// diffusion.hip -- noise-schedule arithmetic of the DDPM (HBM-bound elementwise kernels).
//
// Reference: models/diffusion/ddpm.py:256-273 (q_sample), :149-158 (predict_x_from_eps, clamp),
// :177-185 (q_posterior mean), :203-227 (p_sample), :241 (x_T ~ N(0,1)), :279 + utils/utils.py:34-40
// (per-sample squared-error sum); models/utils/helpers.py:31-40 (extract, noise_like).
//
// The coefficient tables are the module's [T] fp32 buffers; each sample gathers its own t.  Products and
// sums use __fmul_rn/__fadd_rn in the reference's evaluation order (no FMA contraction), so given the
// same eps_hat and noise the update is bit-identical to the torch expression.
#include "ddk_internal.h"
#include "diffusion_step.h"      // Philox, RestoreTraits, rst_x0, rst_finish, comp4, rst_prologue

#include <climits>

// hipcc contracts a*b+c into an FMA by default (-ffp-contract=fast), even through __fmul_rn/__fadd_rn; the
// schedule arithmetic below must round every product like the reference's separate torch ops do, so this
// file is compiled with -ffp-contract=off (see Makefile).

namespace ddk {

static int grid1d(long long n) {
    const long long b = ceil_div(n > 0 ? n : 1, 256);
    return (int)(b < 2048 ? b : 2048);
}

__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, long long n4, long long n, uint64_t seed, uint32_t step,
                                                    uint32_t stream) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 z = philox_normal4((unsigned long long)i, step, stream, seed);
        if (i * 4 + 3 < n) {
            reinterpret_cast<float4*>(out)[i] = z;
        } else {
            const float zz[4] = {z.x, z.y, z.z, z.w};
            for (int j = 0; j < 4 && i * 4 + j < n; ++j) out[i * 4 + j] = zz[j];
        }
    }
}

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                       const int64_t* __restrict__ t, const float* __restrict__ ca,
                                                       const float* __restrict__ cb, float* __restrict__ out, long long per4,
                                                       long long total4) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int64_t tb = t[i / per4];
        const float a = ca[tb], b = cb[tb];
        const float4 xv = reinterpret_cast<const float4*>(x)[i], ev = reinterpret_cast<const float4*>(eps)[i];
        float4 o;
        o.x = __fadd_rn(__fmul_rn(a, xv.x), __fmul_rn(b, ev.x));
        o.y = __fadd_rn(__fmul_rn(a, xv.y), __fmul_rn(b, ev.y));
        o.z = __fadd_rn(__fmul_rn(a, xv.z), __fmul_rn(b, ev.z));
        o.w = __fadd_rn(__fmul_rn(a, xv.w), __fmul_rn(b, ev.w));
        reinterpret_cast<float4*>(out)[i] = o;
    }
}

// (p_step, the ancestral / DDIM rule, lives in diffusion_step.h: guidance.hip's guided update runs it too)

// DPM-Solver++(2M) (models/diffusion/respace.py dpm_solver_tables): the same clamped x0, then
// x_prev = (c1 x0 + c2 x) + c3 h with h the previous step's x0, which the step leaves in h.  One function for the fused and the
// unfused tail, so given the same eps_hat they are bit-identical.
__device__ __forceinline__ float ms_step(float x, float e, float& h, float cr, float crm1, float c1, float c2, float c3) {
    float x0 = __fsub_rn(__fmul_rn(cr, x), __fmul_rn(crm1, e));
    x0 = clamp_pm1(x0);
    const float mean = __fadd_rn(__fmul_rn(c1, x0), __fmul_rn(c2, x));
    const float out = __fadd_rn(mean, __fmul_rn(c3, h));
    h = x0;
    return out;
}

// f applied to the x, y, z and w components of its float4 operands in turn (a float4& operand hands f a float& it may rewrite)
template <class F, class... V>
__device__ __forceinline__ float4 each4(F&& f, V&&... v) {
    float4 o;
    o.x = f(v.x...);
    o.y = f(v.y...);
    o.z = f(v.z...);
    o.w = f(v.w...);
    return o;
}

__device__ __forceinline__ float4 ms_step4(float4 xv, float4 ev, float4& h, float cr, float crm1, float c1, float c2, float c3) {
    return each4([=](float x, float e, float& hh) { return ms_step(x, e, hh, cr, crm1, c1, c2, c3); }, xv, ev, h);
}

// RePaint (models/diffusion/respace.py repaint_tables).  One reverse op at spaced timestep tau:
//   x_unk = p_step(x, eps_hat, z1);  x_kn = ka x0_known + kb z2 (ka = 1, kb = 0 at tau = 0: exactly x0_known);
//   x = mask ? x_kn : x_unk (a select, not a blend: the known region stays exact and NaN-free);  jump: x = ja x + jb z3.
// inp_known and inp_step are the arithmetic of both tails, so given the same eps_hat they are bit-identical.
__device__ __forceinline__ float4 inp_known4(float4 k, float4 z2, float ka, float kb) {
    return each4([=](float kn, float z) { return __fadd_rn(__fmul_rn(ka, kn), __fmul_rn(kb, z)); }, k, z2);
}

__device__ __forceinline__ float inp_step(float x, float e, float z1, float xk, float m, float z3, float cr, float crm1, float c1,
                                          float c2, float sg, float ja, float jb, bool jump) {
    const float o = m != 0.0f ? xk : p_step(x, e, z1, cr, crm1, c1, c2, sg);
    return jump ? __fadd_rn(__fmul_rn(ja, o), __fmul_rn(jb, z3)) : o;
}

__device__ __forceinline__ float4 inp_step4(float4 xv, float4 ev, float4 z1, float4 xk, float4 m, float4 z3, float cr, float crm1,
                                            float c1, float c2, float sg, float ja, float jb, bool jump) {
    return each4([=](float x, float e, float z, float k, float mk, float zj) { return inp_step(x, e, z, k, mk, zj, cr, crm1, c1, c2, sg, ja, jb, jump); },
                 xv, ev, z1, xk, m, z3);
}

// The last kernel of an unfused step: the rule's update of x given eps_hat in memory, one template for the three sampler kinds.
// Shared: the grid-stride loop over float4s, row t[i / per4] of the tables, the counter decrement (in the sampler this is the step's
// last kernel; see final_tail_kernel) and the Philox key, which a chain keeps in device memory so that one captured graph serves
// every seed.  Per kind: the operands fetched and the device function called.
//   Ancestral: the draw is injected (draw k = t_first - t of a [n_steps][...] array; stride 0: a single tensor) or Philox's
//   Multistep: no draw; the history x0_hist (same layout as x) is read and rewritten element by element
//   Inpaint:   three Philox draws per float4, keyed (index, row t, stream / | 2^30 / | 2^29, seed); the jump's only where the row has one
// (vlb_sweep_terms_kernel, the sweep's unfused epilogue, reduces per slice instead of updating x and stays a kernel of its own)
// (the chain hooks arrive as scalars: as a by-value ChainHooks the Ancestral instantiation takes two VGPRs more)
template <StepKind K>
__global__ __launch_bounds__(256) void p_update_kernel(const StepRule r, const float* __restrict__ eps_hat, const int64_t* __restrict__ t,
                                                       long long per4, long long total4, uint64_t seed, uint32_t stream,
                                                       const int64_t* __restrict__ chain_state, int64_t* dec_counter) {
    if (dec_counter && blockIdx.x == 0 && threadIdx.x == 0) *dec_counter -= 1;
    if (chain_state) {
        seed = (uint64_t)chain_state[1];
        stream = (uint32_t)chain_state[2];
    }
    float4* __restrict__ x = reinterpret_cast<float4*>(r.x);
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int64_t tb = t[i / per4];
        const float cr = r.c_recip[tb], crm1 = r.c_recipm1[tb], a1 = r.c1[tb], a2 = r.c2[tb];
        // the fifth coefficient: c3 of the multistep rule, else sigma = nonzero_mask * exp(0.5 logvar), ddpm.py:220-227
        const float a5 = K == StepKind::Multistep ? r.c3[tb] : (tb > 0 ? r.sigma[tb] : 0.0f);
        const float4 xv = x[i], ev = reinterpret_cast<const float4*>(eps_hat)[i];
        if constexpr (K == StepKind::Multistep) {
            float4 hv = reinterpret_cast<const float4*>(r.x0_hist)[i];
            x[i] = ms_step4(xv, ev, hv, cr, crm1, a1, a2, a5);
            reinterpret_cast<float4*>(r.x0_hist)[i] = hv;
        } else {
            const float sg = a5;
            if constexpr (K == StepKind::Inpaint) {
                const float ka = r.inp.ka[tb], kb = r.inp.kb[tb], ja = r.inp.ja[tb], jb = r.inp.jb[tb];
                const bool jump = jb != 0.0f;
                const float4 kv = reinterpret_cast<const float4*>(r.inp.known)[i], mv = reinterpret_cast<const float4*>(r.inp.mask)[i];
                const float4 z1 = philox_normal4((unsigned long long)i, (uint32_t)tb, stream, seed);
                const float4 xk = inp_known4(kv, philox_normal4((unsigned long long)i, (uint32_t)tb, stream | INPAINT_Z2_BIT, seed), ka, kb);
                const float4 z3 = jump ? philox_normal4((unsigned long long)i, (uint32_t)tb, stream | INPAINT_Z3_BIT, seed)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
                x[i] = inp_step4(xv, ev, z1, xk, mv, z3, cr, crm1, a1, a2, sg, ja, jb, jump);
            } else {
                const float4 zv = r.noise ? reinterpret_cast<const float4*>(r.noise + (long long)(r.t_first - tb) * r.noise_step_stride)[i]
                                          : philox_normal4((unsigned long long)i, (uint32_t)tb, stream, seed);
                float4 o;
                o.x = p_step(xv.x, ev.x, zv.x, cr, crm1, a1, a2, sg);
                o.y = p_step(xv.y, ev.y, zv.y, cr, crm1, a1, a2, sg);
                o.z = p_step(xv.z, ev.z, zv.z, cr, crm1, a1, a2, sg);
                o.w = p_step(xv.w, ev.w, zv.w, cr, crm1, a1, a2, sg);
                x[i] = o;
            }
        }
    }
}

// ---- DDNM restoration (Wang, Yu, Zhang, ICLR 2023, Algorithm 1 and section 3.3; DESIGN.md sections 3.6, 3.8 - 3.11) -------------
// One step for the five restore kinds: the clipped x0 of p_step (rst_x0), its projection onto the measurement x0' = x0 + A+ (y - A x0)
// (rst_x0p, not re-clamped), then the rule's update on x0' (rst_finish).  A = mask o pool_n [o grey_w]: m is A x0 of the element's n x n
// block (rst_block_mean) or n x n x 3 group (gry_group), summed in row-major order.  What a kind adds is a compile-time flag:
//   kind              MASK      HIST  NOISY  GRAY  n = 1
//   Restore           absent    -     -      -     -
//   RestoreMasked     required  -     -      -     pointwise
//   RestoreMultistep  optional  yes   -      -     pointwise
//   RestoreNoisy      optional  -     yes    -     pointwise
//   RestoreGray       optional  -     yes    yes   a group of three
//   RestoreBlur       PLANE: no block at all -- A is a separable blur, x0' = (x0 - P_h x0 P_w^T) + Yp, the kernels in separable.hip
//   RestoreHadamard   PLANE: A is the first m rows of a plane's permuted Walsh-Hadamard transform, the kernels in hadamard.hip
//   RestoreFFT        PLANE: A is a circular convolution with a 2-D point-spread function, the kernels in fft_conv.hip
//   RestoreFFTNoisy   PLANE: RestoreFFT's operator, DDNM+ per frequency, the kernels in fft_conv.hip
// MASK: the block's (n = 1: the pixel's) mask value, 1 where no mask was given, selects between x0' and x0 -- a select, never a blend,
// so whatever an unmeasured y holds (NaN included) reaches no result.  HIST: DPM-Solver++(2M)'s history term in the place of the draw,
// the history then holding x0'.  NOISY (DDNM+): the correction scaled by the row's lam and the draw of a measured element by the row's
// sgm instead of sigma.  GRAY: the correction also scaled by A+'s factor a_c of the element's channel.  Pointwise n = 1: the block is
// the element, so x0' = y where measured with no arithmetic (known pixels come back bit for bit at row 0), under NOISY x0 + lam (y - x0).
// These functions are the arithmetic of both tails, every operation rounded on its own, so given the same eps_hat the tails are
// bit-identical.
// (RestoreTraits, rst_x0, rst_finish, comp4, rst_prologue and the Philox draws live in diffusion_step.h, shared with separable.hip.)
// x0_at(i, j): the clipped x0 at row i, column j of the element's block (same image, same channel)
template <class F>
__device__ __forceinline__ float rst_block_mean(F&& x0_at, int n) {
    float s = 0.0f;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) s = __fadd_rn(s, x0_at(i, j));
    return __fmul_rn(s, 1.0f / (float)(n * n));                           // n a power of two: exact
}

// m: A x0 of the element's block or group (POINT: not read); mk: its mask value; lam: NOISY; ac: GRAY
template <StepKind K, bool POINT = false>
__device__ __forceinline__ float rst_x0p(float x0, float m, float y, float mk, float lam, float ac) {
    using T = RestoreTraits<K>;
    float x0p = y;
    if constexpr (!POINT || T::NOISY) {
        float d = __fsub_rn(y, POINT ? x0 : m);
        if constexpr (T::GRAY) d = __fmul_rn(ac, d);
        if constexpr (T::NOISY) d = __fmul_rn(lam, d);
        x0p = __fadd_rn(x0, d);
    }
    if constexpr (T::MASK) return mk != 0.0f ? x0p : x0;
    return x0p;
}

// the pointwise step (n = 1) of one element
template <StepKind K>
__device__ __forceinline__ float rst_point(float x, float e, float y, float mk, float& zh, float cr, float crm1, float c1, float c2, float a5,
                                           float lam, float sgm) {
    const float x0 = rst_x0(x, e, cr, crm1);
    return rst_finish<K>(x, rst_x0p<K, true>(x0, x0, y, mk, lam, 1.0f), mk, zh, c1, c2, a5, sgm);
}

// the n = 1 mask values of elements e0 .. e0 + 3 (e0 % 4 == 0) of an NHWC map with C channels, mk pointing at the map's first pixel:
// one pixel when 4 divides C, else up to three (a 3-channel pixel model)
__device__ __forceinline__ float4 rstm_mask4(const float* __restrict__ mk, unsigned e0, unsigned C) {
    if ((C & 3u) == 0u) {
        const float m = mk[e0 / C];
        return make_float4(m, m, m, m);
    }
    return make_float4(mk[e0 / C], mk[(e0 + 1u) / C], mk[(e0 + 2u) / C], mk[(e0 + 3u) / C]);
}

// the row's coefficients of a restore step: c_recip, c_recipm1, c1, c2, the fifth (sigma with its t > 0 mask, or HIST: c3), NOISY: lam, sgm
struct RestoreCoef {
    float cr, crm1, a1, a2, a5, lam, sgm;
};
template <StepKind K>
__device__ __forceinline__ RestoreCoef rst_coef(const StepRule& r, int64_t tb) {
    RestoreCoef k{r.c_recip[tb], r.c_recipm1[tb], r.c1[tb], r.c2[tb], 0.0f, 0.0f, 0.0f};
    if constexpr (RestoreTraits<K>::HIST) k.a5 = r.c3[tb];
    else k.a5 = tb > 0 ? r.sigma[tb] : 0.0f;
    if constexpr (RestoreTraits<K>::NOISY) { k.lam = r.nsy.lam[tb]; k.sgm = r.nsy.sgm[tb]; }
    return k;
}

// The last kernel of an unfused restore step with n >= 2 (Restore, RestoreMasked, RestoreMultistep, RestoreNoisy).  p_update_kernel's flat
// float4 loop cannot see an element's neighbours, so here a thread owns one (image, block, channel): it sums the block's n x n clipped
// x0 from x and eps_hat, then updates those n x n elements of x (HIST: and of the history) in place; nobody else reads them.  Any
// n_out, any H, W that n divides.  y is [B][H/n][W/n][n_out], the mask [B][H/n][W/n].  Element e of the NHWC latent takes component
// e & 3 of the Philox draw of float4 e >> 2, the Ancestral kind's keying.
template <StepKind K>
__global__ __launch_bounds__(256) void p_update_restore_kernel(const StepRule r, const float* __restrict__ eps_hat,
                                                               const int64_t* __restrict__ t, int B, int n_out, uint64_t seed,
                                                               uint32_t stream, const int64_t* __restrict__ chain_state,
                                                               int64_t* dec_counter) {
    using T = RestoreTraits<K>;
    rst_prologue(dec_counter, chain_state, seed, stream);
    const int n = r.rst.n, H = r.rst.H, W = r.rst.W, Hn = H / n, Wn = W / n;
    const long long total = (long long)B * Hn * Wn * n_out;
    float* __restrict__ x = r.x;
    float* __restrict__ hist = r.x0_hist;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % n_out);
        long long q = i / n_out;
        const int bc = (int)(q % Wn);
        q /= Wn;
        const int br = (int)(q % Hn), b = (int)(q / Hn);
        const int64_t tb = t[b];
        const RestoreCoef k = rst_coef<K>(r, tb);
        const long long e0 = (((long long)b * H + br * n) * W + bc * n) * n_out + c;       // the block's first element
        const float m = rst_block_mean(
            [&](int bi, int bj) {
                const long long e = e0 + ((long long)bi * W + bj) * n_out;
                return rst_x0(x[e], eps_hat[e], k.cr, k.crm1);
            },
            n);
        const float yv = r.rst.y[i];                                      // this thread's index
        float mk = 1.0f;
        if constexpr (T::MASK) mk = T::MASK_REQUIRED || r.rst.mask ? r.rst.mask[i / n_out] : 1.0f;
        for (int bi = 0; bi < n; ++bi)
            for (int bj = 0; bj < n; ++bj) {
                const long long e = e0 + ((long long)bi * W + bj) * n_out;
                const float xv = x[e];
                float zh;
                if constexpr (T::HIST) zh = hist[e];
                else zh = comp4(philox_normal4((unsigned long long)(e >> 2), (uint32_t)tb, stream, seed), (int)(e & 3));
                x[e] = rst_finish<K>(xv, rst_x0p<K>(rst_x0(xv, eps_hat[e], k.cr, k.crm1), m, yv, mk, k.lam, 1.0f), mk, zh, k.a1, k.a2, k.a5, k.sgm);
                if constexpr (T::HIST) hist[e] = zh;
            }
    }
}

// ... and with n = 1 (RestoreMasked, RestoreMultistep, RestoreNoisy; the mask is required): pointwise, so p_update_kernel's flat float4
// loop with one Philox call (HIST: one history float4, read and rewritten) per float4; y has x's layout, the mask is [B][H][W] and the
// float4's elements look up their own pixels (rstm_mask4).
template <StepKind K>
__global__ __launch_bounds__(256) void p_update_restore_point_kernel(const StepRule r, const float* __restrict__ eps_hat,
                                                                     const int64_t* __restrict__ t, long long per4, long long total4,
                                                                     int n_out, uint64_t seed, uint32_t stream,
                                                                     const int64_t* __restrict__ chain_state, int64_t* dec_counter) {
    using T = RestoreTraits<K>;
    static_assert(T::POINT, "the kinds whose n = 1 is pointwise");
    rst_prologue(dec_counter, chain_state, seed, stream);
    float4* __restrict__ x = reinterpret_cast<float4*>(r.x);
    float4* __restrict__ hist = reinterpret_cast<float4*>(r.x0_hist);
    const long long hw = (long long)r.rst.H * r.rst.W;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const long long b = i / per4;
        const int64_t tb = t[b];
        const RestoreCoef k = rst_coef<K>(r, tb);
        const float4 xv = x[i], ev = reinterpret_cast<const float4*>(eps_hat)[i], yv = reinterpret_cast<const float4*>(r.rst.y)[i];
        const float4 mv = rstm_mask4(r.rst.mask + b * hw, (unsigned)(i - b * per4) * 4u, (unsigned)n_out);      // host: per < 2^31
        float4 zh;
        if constexpr (T::HIST) zh = hist[i];
        else zh = philox_normal4((unsigned long long)i, (uint32_t)tb, stream, seed);
        x[i] = each4([&](float xe, float e, float y, float mk, float& z) { return rst_point<K>(xe, e, y, mk, z, k.cr, k.crm1, k.a1, k.a2, k.a5, k.lam, k.sgm); },
                     xv, ev, yv, mv, zh);
        if constexpr (T::HIST) hist[i] = zh;
    }
}

// The grey measurement of a 3-channel map: the group of an element is its n x n block over all three channels;
// the group value is the weighted sum in row-major order, channel innermost, times NORM.  mean: w = a = 1 and NORM = 1 / (3 n n) (the
// products by 1 are exact); luma (BT.601): w_c, NORM = 1 / (n n), a_c = w_c / (w . w) formed in double.
struct GrayCoef {
    float w0, w1, w2, a0, a1, a2, norm;
};
__device__ __forceinline__ GrayCoef gry_coef(int gray, int n) {
    constexpr double w0 = 0.299, w1 = 0.587, w2 = 0.114, ww = (w0 * w0 + w1 * w1) + w2 * w2;
    const bool luma = gray == GRAY_LUMA;
    GrayCoef k;
    k.w0 = luma ? (float)w0 : 1.0f; k.w1 = luma ? (float)w1 : 1.0f; k.w2 = luma ? (float)w2 : 1.0f;
    k.a0 = luma ? (float)(w0 / ww) : 1.0f; k.a1 = luma ? (float)(w1 / ww) : 1.0f; k.a2 = luma ? (float)(w2 / ww) : 1.0f;
    k.norm = __fmul_rn(luma ? 1.0f : (float)(1.0 / 3.0), 1.0f / (float)(n * n));      // n a power of two: (float)(1.0 / (3 n n)) exactly
    return k;
}

// x0_at(i, j, c): the clipped x0 at row i, column j, channel c of the element's group (same image)
template <class F>
__device__ __forceinline__ float gry_group(F&& x0_at, int n, const GrayCoef& k) {
    float g = 0.0f;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            g = __fadd_rn(g, __fmul_rn(k.w0, x0_at(i, j, 0)));
            g = __fadd_rn(g, __fmul_rn(k.w1, x0_at(i, j, 1)));
            g = __fadd_rn(g, __fmul_rn(k.w2, x0_at(i, j, 2)));
        }
    return __fmul_rn(g, k.norm);
}

// The last kernel of an unfused RestoreGray step, n in {1, 2, 4, 8}: a thread owns one (image, block) with all three channels, forms the
// group value from x and eps_hat, then updates the block's n n 3 elements in place (no other thread touches them).  r.rst.y and
// r.rst.mask are [B][H/n][W/n]; the mask may be null (every block measured).  The draw as p_update_restore_kernel's.
__global__ __launch_bounds__(256) void p_update_restore_gray_kernel(const StepRule r, const float* __restrict__ eps_hat,
                                                                    const int64_t* __restrict__ t, int B, uint64_t seed, uint32_t stream,
                                                                    const int64_t* __restrict__ chain_state, int64_t* dec_counter) {
    constexpr StepKind K = StepKind::RestoreGray;
    rst_prologue(dec_counter, chain_state, seed, stream);
    const int n = r.rst.n, H = r.rst.H, W = r.rst.W, Hn = H / n, Wn = W / n;
    const long long total = (long long)B * Hn * Wn;
    const GrayCoef g = gry_coef(r.rst.gray, n);
    float* __restrict__ x = r.x;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int bc = (int)(i % Wn);
        const long long q = i / Wn;
        const int br = (int)(q % Hn), b = (int)(q / Hn);
        const int64_t tb = t[b];
        const RestoreCoef k = rst_coef<K>(r, tb);
        const long long e0 = (((long long)b * H + br * n) * W + bc * n) * 3;       // the group's first element
        const float m = gry_group(
            [&](int bi, int bj, int c) {
                const long long e = e0 + ((long long)bi * W + bj) * 3 + c;
                return rst_x0(x[e], eps_hat[e], k.cr, k.crm1);
            },
            n, g);
        const float mk = r.rst.mask ? r.rst.mask[i] : 1.0f;
        const float yv = r.rst.y[i];
        for (int bi = 0; bi < n; ++bi)
            for (int bj = 0; bj < n; ++bj)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const long long e = e0 + ((long long)bi * W + bj) * 3 + c;
                    const float xv = x[e];
                    float z = comp4(philox_normal4((unsigned long long)(e >> 2), (uint32_t)tb, stream, seed), (int)(e & 3));
                    const float ac = c == 0 ? g.a0 : c == 1 ? g.a1 : g.a2;
                    x[e] = rst_finish<K>(xv, rst_x0p<K>(rst_x0(xv, eps_hat[e], k.cr, k.crm1), m, yv, mk, k.lam, ac), mk, z, k.a1, k.a2, k.a5, k.sgm);
                }
    }
}

// ---- the VLB term of one element (reference models/diffusion/ddpm.py:317-366, models/utils/losses.py:17-109) --------------------
// Shared by vlb_terms_kernel and the likelihood sweep's epilogues (final_tail_kernel<.., StepKind::Vlb>, vlb_sweep_terms_kernel).
__device__ __forceinline__ float std_normal_cdf_approx(float v) {
    return 0.5f * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * (v * v * v))));      // sqrt(2/pi)
}

struct VlbCoef {
    float cr, crm1, a1, a2, inv_var, inv_std, kl0;
    bool t0;
};

__device__ __forceinline__ VlbCoef vlb_coef(int64_t tb, const float* c_recip, const float* c_recipm1, const float* c1, const float* c2,
                                            const float* logvar) {
    VlbCoef k;
    const float lv = logvar[tb];
    k.cr = c_recip[tb]; k.crm1 = c_recipm1[tb]; k.a1 = c1[tb]; k.a2 = c2[tb];
    k.inv_var = expf(-lv); k.inv_std = expf(-(0.5f * lv));
    k.kl0 = (lv - lv - 1.0f) + expf(lv - lv);
    k.t0 = tb == 0;
    return k;
}

// t > 0: KL(q(x_{t-1} | x_t, x) || p(x_{t-1} | x_t)) in nats; t == 0: the discretised-Gaussian NLL of x
__device__ __forceinline__ float vlb_elem(float xv, float xt, float eh, const VlbCoef& k) {
    float x0 = __fsub_rn(__fmul_rn(k.cr, xt), __fmul_rn(k.crm1, eh));
    x0 = clamp_pm1(x0);
    const float pred = __fadd_rn(__fmul_rn(k.a1, x0), __fmul_rn(k.a2, xt));
    if (k.t0) {
        const float c = xv - pred;
        const float cdf_plus = std_normal_cdf_approx(k.inv_std * (c + 1.0f / 255.0f));
        const float cdf_min = std_normal_cdf_approx(k.inv_std * (c - 1.0f / 255.0f));
        const float lp = xv < -0.999f ? logf(clamp_min_nan(cdf_plus, 1e-12f))
                                      : (xv > 0.999f ? logf(clamp_min_nan(1.0f - cdf_min, 1e-12f))
                                                     : logf(clamp_min_nan(cdf_plus - cdf_min, 1e-12f)));
        return -lp;
    }
    const float tm = __fadd_rn(__fmul_rn(k.a1, xv), __fmul_rn(k.a2, xt));
    const float d = tm - pred;
    return 0.5f * (k.kl0 + (d * d) * k.inv_var);
}

// ------------------------------------------------------------------------------------------------
// The end of a forward in ONE launch (reference models/unet/unet.py:69-72 after the final Block's conv, blocks.py:79-80;
// in the sampler also models/diffusion/ddpm.py:149-158,177-185,216-227): GroupNorm (statistics from the final conv's per-tile
// partials) -> Mish -> 1x1 projection to n_out <= 8 channels -> eps_hat, and -- when x is given -- the reverse-step update of x
// in place.  Replaces gn_apply_parts_kernel + conv1x1_n8_kernel + p_update_kernel: the normalised activation (16.8 MB at
// cfg4) and eps_hat never go to memory.
//   workgroup (16 waves) = one 128-pixel tile of one image; phase 1: LPP lanes share a pixel (conv1x1_n8_kernel's butterfly), eps_hat of
//   the tile goes to LDS; phase 2: the tile's 128 * n_out latent elements are updated with p_update_kernel's exact arithmetic
//   and Philox indexing (bit-identical given the same eps_hat).
struct TailParams {
    const float* raw;          // [B][HW][C] output of the final Block's conv
    const float2* part;        // [B*np][G] {mean, M2} per (128-pixel tile, group)
    const float* gamma;
    const float* beta;
    const float* w;            // [n_out][C]
    const float* bias;         // [n_out] or nullptr
    float* eps_out;            // [B][HW][n_out] or nullptr
    float* x;                  // [B][HW][n_out] or nullptr: updated in place
    const float* noise;
    long long noise_step_stride;
    int t_first;
    const int64_t* t;
    const float *c_recip, *c_recipm1, *c1, *c2, *sigma;
    const int64_t* chain_state;   // sampler: {counter, Philox seed, stream id} in device memory; else seed / stream below
    uint64_t seed;
    uint32_t stream;
    int np, HW, C, cpg, n_out;
    float eps;
    int64_t* dec_counter;         // the step counter, decremented HERE (the step's last kernel) when the first kernel left it alone, or null
    // StepKind::Vlb: x is the clean sample (read only), c_recip .. c2 as above
    const float* xt;              // q_sample(x, t, eps): what the forward ran on
    const float* logvar;          // posterior_log_variance_clipped [T]
    float2* vlb_part;             // [T][B][np] {sum of the VLB terms, sum of (eps - eps_hat)^2} per 128-pixel tile
    int B;
    // StepKind::Multistep: the previous step's clipped x0, same layout as x, read and rewritten
    float* x0_hist;
    const float* c3;
    // StepKind::Inpaint: the known latent, its mask and the per-row tables; StepKind::RestoreNoisy: the per-row scale of the correction and
    // of the draw on measured elements, in the same storage (as in StepRule: the struct keeps its size, and the older kernels the offsets
    // of what follows their arguments)
    union {
        InpaintOps inp;
        NoisyTables nsy;
    };
    // StepKind::Restore / RestoreMasked: the low-resolution image, the block, the map's height and width and (RestoreMasked) the mask;
    // StepKind::RestoreGray: the grey image, and the weights in rst.gray
    RestoreOps rst;
};

// K says how the launch ends (StepRule).  Eps and Ancestral are ONE instantiation, <.., StepKind::Ancestral>: eps_hat out and / or
// the reverse-step update of x, whichever of p.eps_out / p.x is given.  The other kinds exist for C <= 128 only (final_tail_ok).
// Vlb (ddk_vlb_sweep_run): phase 2 evaluates, per element, vlb_terms_kernel's term and (eps - eps_hat)^2 with eps the step-input
// kernel's draw (the same Philox call or injected array), and the workgroup stores the two block sums to its own slot of vlb_part
// (plain stores, no atomics: the kernel boundary publishes them).
// Multistep (ddk_sampler_run_multistep, x given): the DPM-Solver++(2M) update of p_update_kernel; the history float4 is requested
// where the other kinds draw their noise (no Philox rounds), and the thread that read it writes it back.
// Inpaint (ddk_sampler_run_inpaint, x given, Philox only): RePaint's op of p_update_kernel; the known float4, the mask float4 and
// the two extra draws are requested in the same prologue, and x_kn is formed there (4 registers live, not 8).
// The restore kinds (ddk_sampler_run_restore*, x given, Philox only or -- RestoreMultistep -- no draw; flags as RestoreTraits): the y
// and, where the kind has one, the mask value of the block of each of the thread's four elements are requested in the prologue; in
// phase 2 the owners write their clipped x0 over eps_hat in LDS, and one barrier later every owner forms its elements' block values
// from LDS (rst_block_mean; GRAY: gry_group) and finishes with rst_x0p / rst_finish: neither x0 nor eps_hat goes through memory.  The
// 128-pixel tile must hold whole rows of blocks, 128 % (W n) == 0.  Per kind:
//   MASK, n = 1 (uniform per launch; RestoreMasked, RestoreMultistep, RestoreNoisy): pointwise, so no whole blocks needed: the y float4
//     and the mask are requested where Inpaint requests known and mask, and phase 2 is rst_point, with no second barrier
//   HIST: the history float4 is requested where Multistep requests it, and the owner writes x0' back to it
//   NOISY: the row's lam and sgm are loaded with its other coefficients
//   GRAY (n_out == 3): y and the mask have one value per block; the exchange and the second barrier at every n, n = 1 included (a
//     pixel's three channels straddle float4s)
template <int LPP, int VPL, StepKind K>
__global__ __launch_bounds__(1024) void final_tail_kernel(const TailParams p) {
    static_assert(K != StepKind::Eps, "the plain forward runs the Ancestral instantiation with p.x null");
    using RT = RestoreTraits<K>;
    constexpr bool VLB = K == StepKind::Vlb, MS = K == StepKind::Multistep, INP = K == StepKind::Inpaint, HIST = MS || RT::HIST;
    constexpr int PPW = 64 / LPP;                    // pixels per wave and iteration
    constexpr int PPI = 16 * PPW;                    // ... per iteration of the 16-wave workgroup
    constexpr int NIT = 128 / PPI;                   // 4 at C = 128 / 256, 2 at C = 64, 1 at C = 32
    __shared__ float2 mr[64];
    __shared__ float2 sp[1024];
    __shared__ __attribute__((aligned(16))) float es[128 * 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane % LPP, pl = lane / LPP;
    const int b = blockIdx.x / p.np, tile = blockIdx.x - b * p.np;
    const int G = p.C / p.cpg;
    const long long pix0 = (long long)b * p.HW + tile * 128;
    if (p.dec_counter && blockIdx.x == 0 && tid == 0) *p.dec_counter -= 1;     // nobody reads the counter in this kernel (t comes from t_cur)
    // every pixel this wave will touch is requested up front, before the statistics are merged: one latency, not NIT
    float4 v[NIT][VPL];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
#pragma unroll
        for (int i = 0; i < VPL; ++i)
            v[it][i] = *reinterpret_cast<const float4*>(p.raw + (pix0 + it * PPI + wave * PPW + pl) * p.C + (sub + i * LPP) * 4);
    const float2* pb = p.part + (long long)b * p.np * G;
    for (int i = tid; i < p.np * G; i += 1024) sp[i] = pb[i];
    // ... and so is everything else that does not depend on the statistics
    float4 ga[VPL], be[VPL], ww[8][VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c0 = (sub + i * LPP) * 4;
        ga[i] = *reinterpret_cast<const float4*>(p.gamma + c0);
        be[i] = *reinterpret_cast<const float4*>(p.beta + c0);
#pragma unroll
        for (int co = 0; co < 8; ++co)
            ww[co][i] = co < p.n_out ? *reinterpret_cast<const float4*>(p.w + (long long)co * p.C + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const bool h2 = sub & (LPP / 2), h4 = sub & (LPP / 4), h8 = sub & (LPP / 8);
    const int my_co = (h2 ? 4 : 0) + (h4 ? 2 : 0) + (h8 ? 1 : 0);
    const float my_bias = (p.bias && my_co < p.n_out) ? p.bias[my_co] : 0.f;
    // ... including phase 2's operands of the threads that have one (128 * n_out / 4 <= 256 float4 per tile): the latent, the schedule
    // scalars and the noise draw depend on nothing computed here -- one memory latency and the Philox rounds less behind the last barrier
    const int cnt4 = 128 * p.n_out / 4;
    const long long e4 = pix0 * p.n_out / 4;          // host: (128 * n_out) % 4 == 0
    float4 xv0 = make_float4(0.f, 0.f, 0.f, 0.f), zv0 = xv0;
    float cr = 0.f, crm1 = 0.f, a1 = 0.f, a2 = 0.f, sg = 0.f, a3 = 0.f;
    float lam = 0.f, sgm = 0.f;                       // restore, NOISY
    int64_t tb = 0;
    float4 xt0 = xv0;
    float4 xk0 = xv0, mk0 = xv0, z30 = xv0;           // INP: x_kn, the mask, the jump's draw
    float ja = 0.f, jb = 0.f;
    bool jump = false;
    float yv0[4] = {0.f, 0.f, 0.f, 0.f};              // restore: y of the block of each of the thread's four elements
    float mv0[4] = {0.f, 0.f, 0.f, 0.f};              // restore, MASK: ... and its mask value
    VlbCoef kc{};
    if ((VLB || p.x) && tid < cnt4) {
        const uint64_t seed = p.chain_state ? (uint64_t)p.chain_state[1] : p.seed;
        const uint32_t stream = p.chain_state ? (uint32_t)p.chain_state[2] : p.stream;
        tb = p.t[b];
        if constexpr (VLB) {
            kc = vlb_coef(tb, p.c_recip, p.c_recipm1, p.c1, p.c2, p.logvar);
        } else {
            cr = p.c_recip[tb]; crm1 = p.c_recipm1[tb]; a1 = p.c1[tb]; a2 = p.c2[tb];
            if constexpr (HIST) a3 = p.c3[tb];
            else sg = tb > 0 ? p.sigma[tb] : 0.0f;
            if constexpr (RT::NOISY) { lam = p.nsy.lam[tb]; sgm = p.nsy.sgm[tb]; }
        }
        const long long i = e4 + tid;
        xv0 = reinterpret_cast<const float4*>(p.x)[i];
        if constexpr (VLB) xt0 = reinterpret_cast<const float4*>(p.xt)[i];
        if constexpr (HIST) zv0 = reinterpret_cast<const float4*>(p.x0_hist)[i];      // zv0 holds the history, not a draw
        else zv0 = p.noise ? reinterpret_cast<const float4*>(p.noise + (long long)(p.t_first - tb) * p.noise_step_stride)[i]
                           : philox_normal4((unsigned long long)i, (uint32_t)tb, stream, seed);
        if constexpr (INP) {
            const float ka = p.inp.ka[tb], kb = p.inp.kb[tb];
            ja = p.inp.ja[tb]; jb = p.inp.jb[tb];
            jump = jb != 0.0f;                         // one row per launch: uniform
            mk0 = reinterpret_cast<const float4*>(p.inp.mask)[i];
            xk0 = inp_known4(reinterpret_cast<const float4*>(p.inp.known)[i],
                             philox_normal4((unsigned long long)i, (uint32_t)tb, stream | INPAINT_Z2_BIT, seed), ka, kb);
            if (jump) z30 = philox_normal4((unsigned long long)i, (uint32_t)tb, stream | INPAINT_Z3_BIT, seed);
        }
        if constexpr (RT::RESTORE) {
            if (RT::POINT && p.rst.n == 1) {           // one block per launch: uniform
                const float4 yv = reinterpret_cast<const float4*>(p.rst.y)[i];
                const float4 mv = rstm_mask4(p.rst.mask + pix0, (unsigned)tid * 4u, (unsigned)p.n_out);
                yv0[0] = yv.x; yv0[1] = yv.y; yv0[2] = yv.z; yv0[3] = yv.w;
                mv0[0] = mv.x; mv0[1] = mv.y; mv0[2] = mv.z; mv0[3] = mv.w;
            } else {
                const int W = p.rst.W, n = p.rst.n, Wn = W / n, no = RT::GRAY ? 3 : p.n_out;      // GRAY: n_out == 3 (final_tail_ok)
                const long long yrow0 = pix0 / (W * n);          // the tile's first row of blocks, over all images (GRAY, n = 1: not used)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int lp = (tid * 4 + j) / no, c = tid * 4 + j - lp * no, row = lp / W, col = lp - row * W;
                    const long long blk = RT::GRAY && n == 1 ? pix0 + lp : (yrow0 + row / n) * Wn + col / n;
                    yv0[j] = p.rst.y[RT::GRAY ? blk : blk * no + c];      // GRAY: one value per block, shared by the three channels
                    if constexpr (RT::MASK) mv0[j] = RT::MASK_REQUIRED || p.rst.mask ? p.rst.mask[blk] : 1.0f;
                }
            }
        }
    }
    __syncthreads();
    if (tid < G) {          // the same fixed-order merge as gn_apply_parts_kernel
        float ms = 0.f;
        for (int i = 0; i < p.np; ++i) ms += sp[i * G + tid].x;
        const float mean = ms / (float)p.np;
        float m2 = 0.f, d2 = 0.f;
        for (int i = 0; i < p.np; ++i) {
            const float2 t = sp[i * G + tid];
            m2 += t.y;
            d2 += (t.x - mean) * (t.x - mean);
        }
        const float n_i = 128.0f * (float)p.cpg;
        const float var = (m2 + n_i * d2) / ((float)p.np * n_i);
        mr[tid] = make_float2(mean, 1.0f / sqrtf(var + p.eps));
    }
    __syncthreads();
    float2 st[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) st[i] = mr[((sub + i * LPP) * 4) / p.cpg];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int lp = it * PPI + wave * PPW + pl;   // pixel within the tile
        float s[8];
#pragma unroll
        for (int co = 0; co < 8; ++co) s[co] = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            float4 y;
            y.x = mish_f((v[it][i].x - st[i].x) * st[i].y * ga[i].x + be[i].x);
            y.y = mish_f((v[it][i].y - st[i].x) * st[i].y * ga[i].y + be[i].y);
            y.z = mish_f((v[it][i].z - st[i].x) * st[i].y * ga[i].z + be[i].z);
            y.w = mish_f((v[it][i].w - st[i].x) * st[i].y * ga[i].w + be[i].w);
#pragma unroll
            for (int co = 0; co < 8; ++co) s[co] += (y.x * ww[co][i].x + y.y * ww[co][i].y) + (y.z * ww[co][i].z + y.w * ww[co][i].w);
        }
        // conv1x1_n8_kernel's packed butterfly: lane l ends with output my_co summed over the pixel's LPP lanes
        float t4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float keep = h2 ? s[4 + i] : s[i], send = h2 ? s[i] : s[4 + i];
            t4[i] = keep + __shfl_xor(send, LPP / 2, 64);
        }
        float t2[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float keep = h4 ? t4[2 + i] : t4[i], send = h4 ? t4[i] : t4[2 + i];
            t2[i] = keep + __shfl_xor(send, LPP / 4, 64);
        }
        float r = (h8 ? t2[1] : t2[0]) + __shfl_xor(h8 ? t2[0] : t2[1], LPP / 8, 64);
#pragma unroll
        for (int o = LPP / 16; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
        if ((sub & (LPP / 8 - 1)) == 0 && my_co < p.n_out) es[lp * p.n_out + my_co] = r + my_bias;
    }
    __syncthreads();
    // phase 2: the tile's 128 * n_out elements, contiguous in the NHWC latent (cnt4 <= 256: at most one float4 per thread)
    if constexpr (VLB) {
        __shared__ float red[32];
        float acc = 0.f, sq = 0.f;
        if (tid < cnt4) {
            const float4 ev = reinterpret_cast<const float4*>(es)[tid];
            acc = (vlb_elem(xv0.x, xt0.x, ev.x, kc) + vlb_elem(xv0.y, xt0.y, ev.y, kc)) +
                  (vlb_elem(xv0.z, xt0.z, ev.z, kc) + vlb_elem(xv0.w, xt0.w, ev.w, kc));
            const float d0 = zv0.x - ev.x, d1 = zv0.y - ev.y, d2 = zv0.z - ev.z, d3 = zv0.w - ev.w;
            sq = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
        acc = block_sum(acc, red);
        sq = block_sum(sq, red);
        if (tid == 0) p.vlb_part[((long long)tb * p.B + b) * p.np + tile] = make_float2(acc, sq);
        return;
    }
    if constexpr (RT::RESTORE) {
        const float a5 = RT::HIST ? a3 : sg;             // zv0: the draw, HIST: the history, which rst_finish rewrites
        if (RT::POINT && p.rst.n == 1) {
            if (tid < cnt4) {
                const float4 ev = reinterpret_cast<const float4*>(es)[tid];
                if (p.eps_out) reinterpret_cast<float4*>(p.eps_out)[e4 + tid] = ev;
                reinterpret_cast<float4*>(p.x)[e4 + tid] =
                    each4([&](float x, float e, float y, float mk, float& z) { return rst_point<K>(x, e, y, mk, z, cr, crm1, a1, a2, a5, lam, sgm); },
                          xv0, ev, make_float4(yv0[0], yv0[1], yv0[2], yv0[3]), make_float4(mv0[0], mv0[1], mv0[2], mv0[3]), zv0);
                if constexpr (RT::HIST) reinterpret_cast<float4*>(p.x0_hist)[e4 + tid] = zv0;
            }
            return;
        }
        float x0v[4] = {0.f, 0.f, 0.f, 0.f};
        if (tid < cnt4) {
            const float4 ev = reinterpret_cast<const float4*>(es)[tid];
            if (p.eps_out) reinterpret_cast<float4*>(p.eps_out)[e4 + tid] = ev;
            x0v[0] = rst_x0(xv0.x, ev.x, cr, crm1); x0v[1] = rst_x0(xv0.y, ev.y, cr, crm1);
            x0v[2] = rst_x0(xv0.z, ev.z, cr, crm1); x0v[3] = rst_x0(xv0.w, ev.w, cr, crm1);
            reinterpret_cast<float4*>(es)[tid] = make_float4(x0v[0], x0v[1], x0v[2], x0v[3]);      // only its owner read this eps_hat
        }
        __syncthreads();
        if (tid < cnt4) {
            const int W = p.rst.W, n = p.rst.n, no = RT::GRAY ? 3 : p.n_out;
            const float xa[4] = {xv0.x, xv0.y, xv0.z, xv0.w};
            float za[4] = {zv0.x, zv0.y, zv0.z, zv0.w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int lp = (tid * 4 + j) / p.n_out, c = tid * 4 + j - lp * p.n_out, row = lp / W, col = lp - row * W;
                const float* blk = es + ((row & ~(n - 1)) * W + (col & ~(n - 1))) * no;      // the block's first pixel
                float m, ac = 1.0f;
                if constexpr (RT::GRAY) {
                    const GrayCoef k = gry_coef(p.rst.gray, n);
                    m = gry_group([&](int bi, int bj, int ch) { return blk[(bi * W + bj) * 3 + ch]; }, n, k);
                    ac = c == 0 ? k.a0 : c == 1 ? k.a1 : k.a2;
                } else {
                    m = rst_block_mean([&](int bi, int bj) { return blk[(bi * W + bj) * p.n_out + c]; }, n);
                }
                o[j] = rst_finish<K>(xa[j], rst_x0p<K>(x0v[j], m, yv0[j], mv0[j], lam, ac), mv0[j], za[j], a1, a2, a5, sgm);
            }
            reinterpret_cast<float4*>(p.x)[e4 + tid] = make_float4(o[0], o[1], o[2], o[3]);
            if constexpr (RT::HIST) reinterpret_cast<float4*>(p.x0_hist)[e4 + tid] = make_float4(za[0], za[1], za[2], za[3]);
        }
        return;
    }
    if (tid < cnt4) {
        const float4 ev = reinterpret_cast<const float4*>(es)[tid];
        if (p.eps_out) reinterpret_cast<float4*>(p.eps_out)[e4 + tid] = ev;
        if constexpr (MS) {
            reinterpret_cast<float4*>(p.x)[e4 + tid] = ms_step4(xv0, ev, zv0, cr, crm1, a1, a2, a3);
            reinterpret_cast<float4*>(p.x0_hist)[e4 + tid] = zv0;
        } else if constexpr (INP) {
            reinterpret_cast<float4*>(p.x)[e4 + tid] = inp_step4(xv0, ev, zv0, xk0, mk0, z30, cr, crm1, a1, a2, sg, ja, jb, jump);
        } else if (p.x) {
            float4 o;
            o.x = p_step(xv0.x, ev.x, zv0.x, cr, crm1, a1, a2, sg);
            o.y = p_step(xv0.y, ev.y, zv0.y, cr, crm1, a1, a2, sg);
            o.z = p_step(xv0.z, ev.z, zv0.z, cr, crm1, a1, a2, sg);
            o.w = p_step(xv0.w, ev.w, zv0.w, cr, crm1, a1, a2, sg);
            reinterpret_cast<float4*>(p.x)[e4 + tid] = o;
        }
    }
}

// What restore_rule_fault asks of one plane-wide kind beyond the part they share: its operands besides rst.y (all required), its
// scratch (required when one_launch declines the shape), its shape rule and the two texts
struct PlaneRule {
    const void* ops[4];
    int n_ops;
    const void* tmp;
    bool (*shape_ok)(int H, int W, int channels);
    bool (*one_launch)(int H, int W, int channels);
    const char *shape_text, *scratch_text;
};
static PlaneRule plane_rule(const StepRule& r) {
    const auto cs_form = [](int H, int W, int) { return restore_cs_plane_form(H, W); };
    const auto fft_form = [](int H, int W, int) { return restore_fft_plane_form(H, W); };
    const char* fft_text = "the deconvolution step needs H and W powers of two in [16, 256] and 1 to 8 channels";
    switch (r.kind) {
        case StepKind::RestoreBlur:       // rst.y is Yp in x's layout, the projections and the scratch in blr
            return {{r.blr.ph, r.blr.pw}, 2, r.blr.tmp, restore_blur_shape_ok, restore_blur_one_launch,
                    "the blur step needs H and W multiples of 16 in [16, 256] and 1 to 8 channels", "an image above 64 KB needs the scratch for T"};
        case StepKind::RestoreHadamard:   // rst.y is [B][C][m], the permutation, the scratch and m in had
            return {{r.had.perm}, 1, r.had.tmp, restore_cs_shape_ok, cs_form,
                    "the compressed-sensing step needs H and W powers of two in [16, 256] and 1 to 8 channels", "a 256 x 256 plane needs the scratch for T"};
        case StepKind::RestoreFFT:        // rst.y is Yp in x's layout, the mask, the twiddles and the scratch in fft
            return {{r.fft.mask, r.fft.tw}, 2, r.fft.tmp, restore_fft_shape_ok, fft_form, fft_text, "a plane above 16384 pixels needs the scratch for T"};
        default:                          // RestoreFFTNoisy: rst.y is the spectrum of A+ y, the mask, the twiddles, the scratch, gain and nsc in fnz
            return {{r.fnz.mask, r.fnz.tw, r.fnz.gain, r.fnz.nsc}, 4, r.fnz.tmp, restore_fft_shape_ok, fft_form, fft_text,
                    "a plane above 16384 pixels needs the scratch for T and T2"};
    }
}

// What both tails ask of a restore kind's rule beyond x, t and the four common tables, `per` being the elements of one image: null
// when the rule is sound, else what is wrong with it.  By kind (RestoreTraits): Restore has no n = 1; RestoreMasked needs its mask, the
// other pointwise kinds need one at n = 1 only (nothing would be constrained), where y is read as float4s.
static const char* restore_rule_fault(const StepRule& r, long long per) {
    const RestoreOps& o = r.rst;
    if (plane_kind(r.kind)) {      // no block: rst.H x rst.W planes, rst.y and the kind's own operands
        const PlaneRule k = plane_rule(r);
        bool there = o.y && r.sigma, aligned = aligned16(o.y) && aligned16(k.tmp);
        for (int i = 0; i < k.n_ops; ++i) { there = there && k.ops[i]; aligned = aligned && aligned16(k.ops[i]); }
        if (!there) return "null pointer";
        if (r.noise) return "no injected noise (Philox only)";
        if (!(o.H > 0 && o.W > 0) || per % ((long long)o.H * o.W)) return "per must be H * W * channels";
        const long long ch = per / ((long long)o.H * o.W);
        if (ch > 8 || !k.shape_ok(o.H, o.W, (int)ch)) return k.shape_text;
        if (r.kind == StepKind::RestoreHadamard && !restore_cs_rows_ok(o.H, o.W, r.had.m)) return "m must be a multiple of 4 in [4, H W]";
        if (!k.one_launch(o.H, o.W, (int)ch) && !k.tmp) return k.scratch_text;
        return aligned ? nullptr : "alignment";
    }
    const bool hist = r.kind == StepKind::RestoreMultistep, gray = r.kind == StepKind::RestoreGray,
               noisy = gray || r.kind == StepKind::RestoreNoisy, n1 = r.kind != StepKind::Restore;
    if (!(o.y && (hist ? r.c3 && r.x0_hist : r.sigma != nullptr) && (!noisy || (r.nsy.lam && r.nsy.sgm)) &&
          (r.kind != StepKind::RestoreMasked || o.mask)))
        return "null pointer";
    if (hist && (r.noise || !aligned16(r.x0_hist))) return "no injected noise, an aligned history";
    if (r.noise) return "no injected noise (Philox only)";
    if (!((o.n == 2 || o.n == 4 || o.n == 8 || (n1 && o.n == 1)) && o.H > 0 && o.W > 0 && o.H % o.n == 0 && o.W % o.n == 0))
        return n1 ? "n must be 1, 2, 4 or 8 and divide H and W" : "n must be 2, 4 or 8 and divide H and W";
    if (o.n == 1 && !o.mask && !gray) return "n = 1 needs a mask (nothing would be constrained)";
    if (gray && !(o.gray == GRAY_MEAN || o.gray == GRAY_LUMA)) return "weights must be 1 (mean) or 2 (luma)";
    const long long hw = (long long)o.H * o.W;
    if (gray && (per != hw * 3 || per > INT_MAX)) return "per must be H * W * 3, below 2^31";
    if (per % hw || per / hw > INT_MAX || (n1 && per > INT_MAX)) return n1 ? "per must be H * W * channels, below 2^31" : "per must be H * W * channels";
    if (o.n == 1 && !gray && !aligned16(o.y)) return "alignment";
    return nullptr;
}

template <StepKind K>
static int launch_tail(const TailParams& p, int B, hipStream_t st) {
    const dim3 grid((unsigned)(B * p.np));
    if (p.C == 32) hipLaunchKernelGGL((final_tail_kernel<8, 1, K>), grid, dim3(1024), 0, st, p);
    else if (p.C == 64) hipLaunchKernelGGL((final_tail_kernel<16, 1, K>), grid, dim3(1024), 0, st, p);
    else if (p.C == 128) hipLaunchKernelGGL((final_tail_kernel<32, 1, K>), grid, dim3(1024), 0, st, p);
    else if constexpr (K == StepKind::Ancestral) hipLaunchKernelGGL((final_tail_kernel<32, 2, K>), grid, dim3(1024), 0, st, p);
    else DDK_REQUIRE(false, "final_tail: C = 256 takes the unfused epilogue in the VLB, multistep, inpainting and restore kinds (final_tail_ok)");
    return check_launch("final_tail_kernel");
}

bool final_tail_ok(int HW, int C, int groups, int n_out, int np, StepKind kind, int restore_w, int restore_n) {
    if (!(C == 32 || C == 64 || C == 128 || C == 256)) return false;
    // the 256-channel instantiation spills registers already in the plain kinds; the others hold more in the prologue
    if (C > 128 && kind != StepKind::Eps && kind != StepKind::Ancestral) return false;
    if (groups <= 0 || groups > 64 || C % groups || (C / groups) % 4) return false;
    if (n_out < 1 || n_out > 8 || (128 * n_out) % 4) return false;
    if (plane_kind(kind)) return false;      // a 128-pixel tile cannot form P_h x0 P_w^T, nor a plane's Walsh-Hadamard or Fourier transform
    if (kind == StepKind::RestoreGray && n_out != 3) return false;       // the grey operator is over a pixel's three colours
    // the restore tail forms block means from the tile's x0 in LDS: the 128-pixel tile must hold whole rows of n x n blocks
    // (the masked kind the same for n >= 2; its n = 1 is pointwise)
    const bool blocks = kind == StepKind::Restore || (restore_kind(kind) && restore_n != 1);
    if (blocks && !(restore_w > 0 && restore_n > 0 && 128 % (restore_w * restore_n) == 0)) return false;
    return np > 0 && HW == np * 128 && np * groups <= 1024;
}

int final_tail(const TailIn& in, const StepRule& r, const int64_t* t, const ChainHooks& h, hipStream_t st) {
    DDK_REQUIRE(in.raw && in.part && in.gamma && in.beta && in.w && in.B > 0, "final_tail: null pointer");
    DDK_REQUIRE(final_tail_ok(in.HW, in.C, in.groups, in.n_out, in.np, r.kind, r.rst.W, r.rst.n),
                "final_tail: needs C in {32,64,128,256} (the VLB, multistep, inpainting and restore kinds: C <= 128), n_out <= 8, "
                "H*W == tiles * 128 (restore with n >= 2: 128 % (W n) == 0)");
    DDK_REQUIRE(aligned16(in.raw) && aligned16(in.gamma) && aligned16(in.beta) && aligned16(in.w) && aligned16(r.eps_out) && aligned16(r.x) &&
                    aligned16(r.noise) && r.noise_step_stride % 4 == 0, "final_tail: alignment");
    const bool tables = r.x && t && r.c_recip && r.c_recipm1 && r.c1 && r.c2;     // what every kind but Eps reads
    TailParams p{};
    p.raw = in.raw; p.part = reinterpret_cast<const float2*>(in.part); p.gamma = in.gamma; p.beta = in.beta; p.w = in.w; p.bias = in.bias;
    p.eps_out = r.eps_out; p.x = r.x; p.noise = r.noise; p.noise_step_stride = r.noise_step_stride; p.t_first = r.t_first; p.t = t;
    p.c_recip = r.c_recip; p.c_recipm1 = r.c_recipm1; p.c1 = r.c1; p.c2 = r.c2; p.sigma = r.sigma;
    p.chain_state = h.chain_state; p.seed = h.seed; p.stream = h.stream_id; p.dec_counter = h.dec_counter;
    p.np = in.np; p.HW = in.HW; p.C = in.C; p.cpg = in.C / in.groups; p.n_out = in.n_out; p.eps = in.eps;
    if (restore_kind(r.kind)) {      // the operands of every restore kind; the null ones are those its instantiation does not read
        const char* fault = tables ? restore_rule_fault(r, (long long)in.HW * in.n_out) : "needs x, t and the schedule tables";
        if (!fault && (long long)r.rst.H * r.rst.W != in.HW) fault = "H * W must be the map's";
        if (fault) {
            set_error("bad argument: final_tail: the restore step: %s", fault);
            return DDK_ERR_ARG;
        }
        p.rst = r.rst; p.x0_hist = r.x0_hist; p.c3 = r.c3;
        if (r.kind == StepKind::RestoreNoisy || r.kind == StepKind::RestoreGray) p.nsy = r.nsy;
    }
    switch (r.kind) {
        case StepKind::Eps:
            DDK_REQUIRE(r.eps_out && !r.x, "final_tail: the plain forward needs eps_out and takes no x");
            return launch_tail<StepKind::Ancestral>(p, in.B, st);
        case StepKind::Ancestral:
            DDK_REQUIRE(tables && r.sigma, "final_tail: the update needs x, t and the schedule tables");
            return launch_tail<StepKind::Ancestral>(p, in.B, st);
        case StepKind::Multistep:
            DDK_REQUIRE(tables && r.c3 && r.x0_hist && !r.noise && aligned16(r.x0_hist),
                        "final_tail: the multistep update needs x, t, the tables with c3, no injected noise and an aligned history");
            p.x0_hist = r.x0_hist; p.c3 = r.c3;
            return launch_tail<StepKind::Multistep>(p, in.B, st);
        case StepKind::Inpaint:
            DDK_REQUIRE(tables && r.sigma && !r.noise && r.inp.known && r.inp.mask && r.inp.ka && r.inp.kb && r.inp.ja && r.inp.jb &&
                            aligned16(r.inp.known) && aligned16(r.inp.mask),
                        "final_tail: the inpainting op needs x, t, the tables, its operands, no injected noise and aligned known / mask");
            p.inp = r.inp;
            return launch_tail<StepKind::Inpaint>(p, in.B, st);
        case StepKind::Restore:
            return launch_tail<StepKind::Restore>(p, in.B, st);
        case StepKind::RestoreMasked:
            return launch_tail<StepKind::RestoreMasked>(p, in.B, st);
        case StepKind::RestoreMultistep:
            return launch_tail<StepKind::RestoreMultistep>(p, in.B, st);
        case StepKind::RestoreNoisy:
            return launch_tail<StepKind::RestoreNoisy>(p, in.B, st);
        case StepKind::RestoreGray:
            return launch_tail<StepKind::RestoreGray>(p, in.B, st);
        case StepKind::RestoreBlur:
            return fail_arg("final_tail: the blur step has no fused tail (final_tail_ok)");
        case StepKind::RestoreHadamard:
            return fail_arg("final_tail: the compressed-sensing step has no fused tail (final_tail_ok)");
        case StepKind::RestoreFFT:
        case StepKind::RestoreFFTNoisy:
            return fail_arg("final_tail: the deconvolution step has no fused tail (final_tail_ok)");
        case StepKind::Vlb: {
            DDK_REQUIRE(r.vlb && tables && !r.eps_out && h.chain_state, "final_tail: the VLB epilogue needs the sweep's step, x, t, the tables and the chain state");
            const VlbStep& v = *r.vlb;
            DDK_REQUIRE(v.xt && v.logvar && v.partials && v.nslot == in.np && aligned16(v.xt) && aligned16(v.partials),
                        "final_tail: the VLB epilogue needs aligned x_t and partials, logvar and one slot per tile");
            p.xt = v.xt; p.logvar = v.logvar; p.vlb_part = reinterpret_cast<float2*>(v.partials); p.B = in.B;
            return launch_tail<StepKind::Vlb>(p, in.B, st);
        }
    }
    return fail_arg("final_tail: unknown step kind");
}

// one workgroup per sample: fixed summation tree -> run-to-run deterministic
__global__ __launch_bounds__(1024) void sq_err_sum_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ per_sample, long long per4) {
    __shared__ float red[32];
    const float4* ap = reinterpret_cast<const float4*>(a) + blockIdx.x * per4;
    const float4* bp = reinterpret_cast<const float4*>(b) + blockIdx.x * per4;
    float s = 0.f;
    for (long long i = threadIdx.x; i < per4; i += blockDim.x) {
        const float4 u = ap[i], v = bp[i];
        const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
        s += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) per_sample[blockIdx.x] = s;
}

// Evaluation-time variational bound, one term per sample (reference models/diffusion/ddpm.py:317-366 after the UNet call,
// models/utils/losses.py:17-109, utils/utils.py:43-48), fused into ONE pass over x, x_t, eps_hat (and eps for L_simple):
//   x0 = clamp(c_recip x_t - c_recipm1 eps_hat); pred_mean = c1 x0 + c2 x_t; true_mean = c1 x + c2 x_t      (q_posterior twice)
//   t > 0:  kl  = 0.5 (lv - lv - 1 + exp(lv - lv) + (true_mean - pred_mean)^2 exp(-lv))                      (normal_kl)
//   t == 0: nll = -log p(x | pred_mean, exp(0.5 lv)) of the discretised Gaussian (tanh CDF approximation)
//   vlb[b] = mean_chw(.) / ln 2 (flat_bits);  sqerr[b] = sum_chw (eps - eps_hat)^2.
// The reference evaluates ~25 elementwise torch ops + 2 reductions per timestep (and runs the UNet twice on identical
// inputs); this is one launch, 16 B read per element, one workgroup per sample with a fixed summation tree.

// Each sample is split over `ns` workgroups (a batch of 8 full-resolution images would otherwise occupy 8 of 256 CUs); a slice
// leaves {sum of terms, sum of squared errors} in the workspace (sc1 stores), adds to the sample's arrival counter, and the
// workgroup whose add came last sums the ns partials IN SLICE ORDER -- deterministic whatever the arrival order -- writes the
// outputs and re-arms the counter (MI355X_MICROARCH.md, sc1 table, first row: "the workgroup whose add came last").
__global__ __launch_bounds__(1024) void vlb_terms_kernel(const float* __restrict__ x, const float* __restrict__ x_t,
                                                         const float* __restrict__ eps_hat, const float* __restrict__ eps,
                                                         const int64_t* __restrict__ t, const float* __restrict__ c_recip,
                                                         const float* __restrict__ c_recipm1, const float* __restrict__ c1,
                                                         const float* __restrict__ c2, const float* __restrict__ logvar,
                                                         float* __restrict__ vlb, float* __restrict__ sqerr, long long per, int ns,
                                                         unsigned* __restrict__ counters, float* __restrict__ partials) {
    __shared__ float red[32];
    __shared__ unsigned last;
    const int b = blockIdx.y, sl = blockIdx.x;
    const VlbCoef k = vlb_coef(t[b], c_recip, c_recipm1, c1, c2, logvar);
    const long long base = (long long)b * per;
    const long long chunk = (per + ns - 1) / ns, i0 = sl * chunk, i1 = i0 + chunk < per ? i0 + chunk : per;
    float acc = 0.f, sq = 0.f;
    for (long long i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const float xv = x[base + i], xt = x_t[base + i], eh = eps_hat[base + i];
        const float term = vlb_elem(xv, xt, eh, k);
        acc += term;
        if (eps) { const float e = eps[base + i] - eh; sq += e * e; }
    }
    acc = block_sum(acc, red);
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) {
        float* part = partials + ((long long)b * ns + sl) * 2;
        __hip_atomic_store(part, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + 1, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned old = __hip_atomic_fetch_add(counters + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = old == (unsigned)ns - 1u;
        if (last) {
            float a = 0.f, s2 = 0.f;
            for (int k = 0; k < ns; ++k) {
                a += __hip_atomic_load(partials + ((long long)b * ns + k) * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s2 += __hip_atomic_load(partials + ((long long)b * ns + k) * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            vlb[b] = (a / (float)per) / 0.6931471805599453f;
            if (sqerr) sqerr[b] = s2;
            __hip_atomic_store(counters + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

static int vlb_slices(int B, long long per) {
    int ns = (int)((256 + B - 1) / B);                    // fill the chip ...
    const long long cap = (per + 4095) / 4096;            // ... but keep at least ~4 elements per thread and slice
    if (ns > cap) ns = (int)cap;
    if (ns > 64) ns = 64;
    return ns < 1 ? 1 : ns;
}

// ---- likelihood sweep (ddk_vlb_sweep_run): test_losses_ of reference models/diffusion/ddpm.py:392-446 as a chain of steps -------
// A step: vlb_step_input_kernel (x_t = q_sample(x, t, eps)), the UNet forward on x_t, and an epilogue that leaves the step's
// {sum of VLB terms, sum of (eps - eps_hat)^2} per (t, image, slice) in partials[t][b][slice] -- final_tail_kernel<.., StepKind::Vlb> where
// the fused tail takes the shape, else vlb_sweep_terms_kernel behind conv + GroupNorm + 1x1.  t, the Philox seed and stream come
// from the chain state in device memory, like the sampler's.  vlb_sweep_finalize_kernel sums the partials once, after the last step.

// x_t = sqrt_acp[t] x + sqrt_1m_acp[t] eps (q_sample_kernel's arithmetic), eps = the injected draw k = t_first - t or the Philox draw
// of (float4 index, t, stream, seed) -- the call final_tail_kernel<.., StepKind::Vlb> / vlb_sweep_terms_kernel repeat.  Leaves the counter alone.
__global__ __launch_bounds__(256) void vlb_step_input_kernel(const float* __restrict__ x, float* __restrict__ xt,
                                                             const float* __restrict__ noise, long long noise_step_stride, int t_first,
                                                             const float* __restrict__ ca, const float* __restrict__ cb,
                                                             const int64_t* __restrict__ chain_state, long long total4) {
    const int64_t tb = chain_state[0];
    const uint64_t seed = (uint64_t)chain_state[1];
    const uint32_t stream = (uint32_t)chain_state[2];
    const float a = ca[tb], b = cb[tb];
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const float4 ev = noise ? reinterpret_cast<const float4*>(noise + (long long)(t_first - tb) * noise_step_stride)[i]
                                : philox_normal4((unsigned long long)i, (uint32_t)tb, stream, seed);
        float4 o;
        o.x = __fadd_rn(__fmul_rn(a, xv.x), __fmul_rn(b, ev.x));
        o.y = __fadd_rn(__fmul_rn(a, xv.y), __fmul_rn(b, ev.y));
        o.z = __fadd_rn(__fmul_rn(a, xv.z), __fmul_rn(b, ev.z));
        o.w = __fadd_rn(__fmul_rn(a, xv.w), __fmul_rn(b, ev.w));
        reinterpret_cast<float4*>(xt)[i] = o;
    }
}

// the unfused epilogue: eps_hat from conv + GroupNorm + 1x1 in memory; slice sl of image b sums its share of the float4s
__global__ __launch_bounds__(256) void vlb_sweep_terms_kernel(const VlbStep v, const int64_t* __restrict__ t,
                                                              const float* __restrict__ eps_hat, long long per4, int B,
                                                              const int64_t* __restrict__ chain_state, int64_t* dec_counter) {
    __shared__ float red[32];
    if (dec_counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *dec_counter -= 1;   // nobody reads it here
    const int b = blockIdx.y, sl = blockIdx.x;
    const int64_t tb = t[b];
    const VlbCoef k = vlb_coef(tb, v.c_recip, v.c_recipm1, v.c1, v.c2, v.logvar);
    const uint64_t seed = (uint64_t)chain_state[1];
    const uint32_t stream = (uint32_t)chain_state[2];
    const long long chunk = (per4 + gridDim.x - 1) / gridDim.x, i0 = sl * chunk, i1 = i0 + chunk < per4 ? i0 + chunk : per4;
    const float4* nz = v.noise ? reinterpret_cast<const float4*>(v.noise + (long long)(v.t_first - tb) * v.noise_step_stride) : nullptr;
    float acc = 0.f, sq = 0.f;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        const long long g = (long long)b * per4 + i;
        const float4 xv = reinterpret_cast<const float4*>(v.x)[g], xt = reinterpret_cast<const float4*>(v.xt)[g];
        const float4 eh = reinterpret_cast<const float4*>(eps_hat)[g];
        const float4 z = nz ? nz[g] : philox_normal4((unsigned long long)g, (uint32_t)tb, stream, seed);
        acc += (vlb_elem(xv.x, xt.x, eh.x, k) + vlb_elem(xv.y, xt.y, eh.y, k)) + (vlb_elem(xv.z, xt.z, eh.z, k) + vlb_elem(xv.w, xt.w, eh.w, k));
        const float d0 = z.x - eh.x, d1 = z.y - eh.y, d2 = z.z - eh.z, d3 = z.w - eh.w;
        sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    acc = block_sum(acc, red);
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) reinterpret_cast<float2*>(v.partials)[((long long)tb * B + b) * gridDim.x + sl] = make_float2(acc, sq);
}

// once per sweep, one workgroup per timestep, fixed summation order: vlb_t[b][k] = sum of terms / per / ln 2 (vlb_terms_kernel's
// flat_bits), L_simple_t[k] = sum over b, slices of sq / (B per); k = T-1-t, the reference's column order
__global__ __launch_bounds__(256) void vlb_sweep_finalize_kernel(const float2* __restrict__ part, float* __restrict__ vlb_t,
                                                                 float* __restrict__ l_simple_t, int T, int B, int nslot, long long per) {
    __shared__ float red[32];
    const int t = blockIdx.x, k = T - 1 - t;
    float sq = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float2* pb = part + ((long long)t * B + b) * nslot;
        float a = 0.f, s2 = 0.f;
        for (int j = 0; j < nslot; ++j) {
            const float2 q = pb[j];
            a += q.x;
            s2 += q.y;
        }
        vlb_t[(long long)b * T + k] = (a / (float)per) / 0.6931471805599453f;
        sq += s2;
    }
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) l_simple_t[k] = sq / (float)((long long)B * per);
}

int vlb_sweep_slots_unfused(int B, long long per) { return vlb_slices(B, per); }

int vlb_step_input(const VlbStep& v, const float* sqrt_acp, const float* sqrt_1m_acp, const int64_t* chain_state, int B, long long per,
                   hipStream_t st) {
    DDK_REQUIRE(v.x && v.xt && sqrt_acp && sqrt_1m_acp && chain_state && B > 0 && per % 4 == 0, "vlb_step_input: arguments");
    const long long total4 = B * per / 4;
    hipLaunchKernelGGL(vlb_step_input_kernel, dim3(grid1d(total4)), dim3(256), 0, st, v.x, v.xt, v.noise, v.noise_step_stride, v.t_first,
                       sqrt_acp, sqrt_1m_acp, chain_state, total4);
    return check_launch("vlb_step_input_kernel");
}

static int vlb_sweep_terms(const VlbStep& v, const int64_t* t, const float* eps_hat, int B, long long per, const int64_t* chain_state,
                           hipStream_t st, int64_t* dec_counter) {
    DDK_REQUIRE(v.x && v.xt && v.partials && t && eps_hat && chain_state && B > 0 && per % 4 == 0, "vlb_sweep_terms: arguments");
    DDK_REQUIRE(v.nslot == vlb_slices(B, per), "vlb_sweep_terms: slot count");
    hipLaunchKernelGGL(vlb_sweep_terms_kernel, dim3(v.nslot, B), dim3(256), 0, st, v, t, eps_hat, per / 4, B, chain_state, dec_counter);
    return check_launch("vlb_sweep_terms_kernel");
}

int vlb_sweep_finalize(const float* partials, int nslot, float* vlb_t, float* l_simple_t, int T, int B, long long per, hipStream_t st) {
    DDK_REQUIRE(partials && vlb_t && l_simple_t && T > 0 && B > 0 && nslot > 0, "vlb_sweep_finalize: arguments");
    hipLaunchKernelGGL(vlb_sweep_finalize_kernel, dim3(T), dim3(256), 0, st, reinterpret_cast<const float2*>(partials), vlb_t, l_simple_t,
                       T, B, nslot, per);
    return check_launch("vlb_sweep_finalize_kernel");
}

// the unfused restore step's one kernel: blocks (GRAY: groups) of n x n elements per thread, or float4s where n = 1 is pointwise
template <StepKind K>
static int launch_restore(const StepRule& r, const float* eps_hat, const int64_t* t, int B, long long per, const ChainHooks& h, hipStream_t st) {
    const long long hw = (long long)r.rst.H * r.rst.W, nn = r.rst.n * r.rst.n;
    if constexpr (K == StepKind::RestoreGray) {
        hipLaunchKernelGGL(p_update_restore_gray_kernel, dim3(grid1d(B * hw / nn)), dim3(256), 0, st, r, eps_hat, t, B, h.seed, h.stream_id,
                           h.chain_state, h.dec_counter);
        return check_launch("p_update_restore_gray_kernel");
    } else {
        const int n_out = (int)(per / hw);
        if constexpr (RestoreTraits<K>::POINT)
            if (r.rst.n == 1) {
                hipLaunchKernelGGL(p_update_restore_point_kernel<K>, dim3(grid1d(B * per / 4)), dim3(256), 0, st, r, eps_hat, t, per / 4,
                                   B * per / 4, n_out, h.seed, h.stream_id, h.chain_state, h.dec_counter);
                return check_launch("p_update_restore_point_kernel");
            }
        hipLaunchKernelGGL(p_update_restore_kernel<K>, dim3(grid1d(B * per / nn)), dim3(256), 0, st, r, eps_hat, t, B, n_out, h.seed,
                           h.stream_id, h.chain_state, h.dec_counter);
        return check_launch("p_update_restore_kernel");
    }
}

int p_update(const StepRule& r, const float* eps_hat, const int64_t* t, int B, long long per, const ChainHooks& h, hipStream_t st,
             const char* who) {
    auto bad = [who](const char* what) {
        set_error("bad argument: %s: %s", who, what);
        return DDK_ERR_ARG;
    };
    if (!(r.x && eps_hat && t && r.c_recip && r.c_recipm1 && r.c1 && r.c2)) return bad("null pointer");
    if (!(B > 0 && per > 0 && per % 4 == 0)) return bad("per-sample element count must be a multiple of 4");
    if (!(aligned16(r.x) && aligned16(eps_hat) && aligned16(r.noise) && r.noise_step_stride % 4 == 0)) return bad("alignment");
    if (restore_kind(r.kind))
        if (const char* fault = restore_rule_fault(r, per)) return bad(fault);
    const long long total4 = B * per / 4;
    const dim3 grid(grid1d(total4));
    switch (r.kind) {
        case StepKind::Ancestral:
            if (!r.sigma) return bad("null pointer");
            hipLaunchKernelGGL(p_update_kernel<StepKind::Ancestral>, grid, dim3(256), 0, st, r, eps_hat, t, per / 4, total4, h.seed, h.stream_id, h.chain_state, h.dec_counter);
            break;
        case StepKind::Multistep:
            if (!(r.x0_hist && r.c3)) return bad("null pointer");
            if (r.noise || !aligned16(r.x0_hist)) return bad("no injected noise, an aligned history");
            hipLaunchKernelGGL(p_update_kernel<StepKind::Multistep>, grid, dim3(256), 0, st, r, eps_hat, t, per / 4, total4, h.seed, h.stream_id, h.chain_state, h.dec_counter);
            break;
        case StepKind::Inpaint:
            if (!(r.sigma && r.inp.known && r.inp.mask && r.inp.ka && r.inp.kb && r.inp.ja && r.inp.jb)) return bad("null pointer");
            if (r.noise || !(aligned16(r.inp.known) && aligned16(r.inp.mask))) return bad("no injected noise, aligned known / mask");
            if (!(h.chain_state || h.stream_id < INPAINT_Z3_BIT)) return bad("stream_id must be < 2^29 (bits 29, 30 key the extra draws)");
            hipLaunchKernelGGL(p_update_kernel<StepKind::Inpaint>, grid, dim3(256), 0, st, r, eps_hat, t, per / 4, total4, h.seed, h.stream_id, h.chain_state, h.dec_counter);
            break;
        case StepKind::Restore:
            return launch_restore<StepKind::Restore>(r, eps_hat, t, B, per, h, st);
        case StepKind::RestoreMasked:
            return launch_restore<StepKind::RestoreMasked>(r, eps_hat, t, B, per, h, st);
        case StepKind::RestoreMultistep:
            return launch_restore<StepKind::RestoreMultistep>(r, eps_hat, t, B, per, h, st);
        case StepKind::RestoreNoisy:
            return launch_restore<StepKind::RestoreNoisy>(r, eps_hat, t, B, per, h, st);
        case StepKind::RestoreGray:
            return launch_restore<StepKind::RestoreGray>(r, eps_hat, t, B, per, h, st);
        case StepKind::RestoreBlur:       // separable.hip: one launch, or two through blr.tmp
        case StepKind::RestoreHadamard:   // hadamard.hip: one launch, or three through had.tmp
        case StepKind::RestoreFFT:        // fft_conv.hip: one launch, or three through fft.tmp
        case StepKind::RestoreFFTNoisy: { // fft_conv.hip: one launch, or three through fnz.tmp
            const long long channels = per / ((long long)r.rst.H * r.rst.W);
            if (r.kind == StepKind::RestoreBlur) {
                if (B > 65535) return bad("at most 65535 images");
                return p_update_restore_blur(r, eps_hat, t, B, (int)channels, h, st);
            }
            if (B * channels > 65535) return bad("at most 65535 planes");
            return r.kind == StepKind::RestoreHadamard ? p_update_restore_cs(r, eps_hat, t, B, (int)channels, h, st)
                   : r.kind == StepKind::RestoreFFT    ? p_update_restore_fft(r, eps_hat, t, B, (int)channels, h, st)
                                                       : p_update_restore_fft_noisy(r, eps_hat, t, B, (int)channels, h, st);
        }
        case StepKind::Vlb:       // no update: the sweep's reduction of the step's terms, a kernel of its own
            if (!r.vlb) return bad("null pointer");
            return vlb_sweep_terms(*r.vlb, t, eps_hat, B, per, h.chain_state, st, h.dec_counter);
        case StepKind::Eps:
            return bad("a plain forward has no update of x");
    }
    return check_launch("p_update_kernel");
}

int randn(float* out, long long n, uint64_t seed, uint32_t step, uint32_t stream_id, hipStream_t st) {
    DDK_REQUIRE(out && n > 0 && aligned16(out), "randn: arguments");
    const long long n4 = (n + 3) / 4;
    hipLaunchKernelGGL(randn_kernel, dim3(grid1d(n4)), dim3(256), 0, st, out, n4, n, seed, step, stream_id);
    return check_launch("randn_kernel");
}

}  // namespace ddk

using namespace ddk;


// Sampler output stage (utils/eval_helpers.py:37-41 + utils/utils.py:16-24): per-image min / max over C*H*W, then
// out[b][h][w][c] = ((x[b][c][h][w] - lo) / (hi - lo)) * 255 -- the same three fp32 operations, in the same order, as
// the reference's torch expression (this file is compiled with -ffp-contract=off), written NHWC like its np.moveaxis.
// One workgroup per image: pass 1 reduces, pass 2 normalises and transposes.
__global__ __launch_bounds__(1024) void fix_samples_kernel(const float* __restrict__ x, float* __restrict__ out, int C, long long HW) {
    __shared__ float red[32];
    const long long per = (long long)C * HW;
    const float* xb = x + (long long)blockIdx.x * per;
    float* ob = out + (long long)blockIdx.x * per;
    float lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    for (long long i = threadIdx.x; i < per; i += 1024) {
        const float v = xb[i];
        bad |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    hi = block_max(hi, red);
    lo = -block_max(-lo, red);
    // x.min() / x.max() of an image that holds a NaN are NaN (fminf / fmaxf skip it): the whole image comes out NaN
    if (block_max(bad ? 1.0f : 0.0f, red) != 0.0f) lo = hi = __builtin_nanf("");
    const float range = hi - lo;
    for (long long p = threadIdx.x; p < HW; p += 1024)
        for (int c = 0; c < C; ++c) ob[p * C + c] = ((xb[c * HW + p] - lo) / range) * 255.0f;
}

extern "C" {

int ddk_q_sample(const float* x, const float* eps, const int64_t* t, const float* sqrt_acp, const float* sqrt_1m_acp, float* out,
                 int B, long long per, ddk_stream_t s) {
    DDK_REQUIRE(x && eps && t && sqrt_acp && sqrt_1m_acp && out, "q_sample: null pointer");
    DDK_REQUIRE(B > 0 && per > 0 && per % 4 == 0, "q_sample: per-sample element count must be a multiple of 4");
    DDK_REQUIRE(aligned16(x) && aligned16(eps) && aligned16(out), "q_sample: alignment");
    const long long total4 = B * per / 4;
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid1d(total4)), dim3(256), 0, as_stream(s), x, eps, t, sqrt_acp, sqrt_1m_acp, out,
                       per / 4, total4);
    return check_launch("q_sample_kernel");
}

int ddk_p_sample_update(float* x, const float* eps_hat, const float* noise, const int64_t* t, const float* c_recip,
                        const float* c_recipm1, const float* c1, const float* c2, const float* sigma, int B, long long per,
                        uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    const StepRule r{StepKind::Ancestral, nullptr, x, noise, 0, 0, c_recip, c_recipm1, c1, c2, sigma};
    return p_update(r, eps_hat, t, B, per, ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s), "p_sample_update");
}

int ddk_p_sample_update_multistep(float* x, const float* eps_hat, float* x0_hist, const int64_t* t, const float* c_recip,
                                  const float* c_recipm1, const float* c1, const float* c2, const float* c3, int B, long long per,
                                  ddk_stream_t s) {
    const StepRule r{StepKind::Multistep, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, nullptr, x0_hist, c3};
    return p_update(r, eps_hat, t, B, per, ChainHooks{}, as_stream(s), "p_sample_update_multistep");
}

int ddk_p_sample_update_inpaint(float* x, const float* eps_hat, const float* known, const float* mask, const int64_t* t,
                                const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* sigma,
                                const float* ka, const float* kb, const float* ja, const float* jb, int B, long long per, uint64_t seed,
                                uint32_t stream_id, ddk_stream_t s) {
    const StepRule r{StepKind::Inpaint, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, sigma, nullptr, nullptr,
                     {InpaintOps{known, mask, ka, kb, ja, jb}}};
    return p_update(r, eps_hat, t, B, per, ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s), "p_sample_update_inpaint");
}

}  // extern "C"

// What the restore ops share: the shape check in the entry's name, the rule of its kind and p_update.  c5: sigma, or the solver's c3.
static int restore_op(const char* who, StepKind kind, float* x, const float* eps_hat, float* x0_hist, const RestoreOps& rst, const int64_t* t,
                      const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* c5, const float* lam,
                      const float* sgm, int B, int channels, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    if (!(B > 0 && rst.H > 0 && rst.W > 0 && channels > 0)) {
        set_error("bad argument: %s: B / H / W / channels must be positive", who);
        return DDK_ERR_ARG;
    }
    if (!(rst.mask || rst.n != 1 || kind == StepKind::Restore || kind == StepKind::RestoreGray)) {      // Restore: p_update rejects n = 1
        set_error("bad argument: %s: n = 1 needs a mask (nothing would be constrained)", who);
        return DDK_ERR_ARG;
    }
    const bool hist = kind == StepKind::RestoreMultistep;
    StepRule r{kind, nullptr, x, nullptr, 0, 0, c_recip, c_recipm1, c1, c2, hist ? nullptr : c5, x0_hist, hist ? c5 : nullptr};
    r.rst = rst;
    if (lam || sgm) r.nsy = NoisyTables{lam, sgm};
    return p_update(r, eps_hat, t, B, (long long)rst.H * rst.W * channels, hist ? ChainHooks{} : ChainHooks{nullptr, nullptr, seed, stream_id},
                    as_stream(s), who);
}

extern "C" {

int ddk_p_sample_update_restore(float* x, const float* eps_hat, const float* y, int n, const int64_t* t, const float* c_recip,
                                const float* c_recipm1, const float* c1, const float* c2, const float* sigma, int B, int H, int W,
                                int channels, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    return restore_op("p_sample_update_restore", StepKind::Restore, x, eps_hat, nullptr, RestoreOps{y, n, H, W, 0, nullptr}, t, c_recip,
                      c_recipm1, c1, c2, sigma, nullptr, nullptr, B, channels, seed, stream_id, s);
}

int ddk_p_sample_update_restore_masked(float* x, const float* eps_hat, const float* y, const float* mask, int n, const int64_t* t,
                                       const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* sigma,
                                       int B, int H, int W, int channels, uint64_t seed, uint32_t stream_id, ddk_stream_t s) {
    // no mask (n >= 2): every block is measured, which is the Restore kind, its kernel and its bits
    return restore_op("p_sample_update_restore_masked", mask || n == 1 ? StepKind::RestoreMasked : StepKind::Restore, x, eps_hat, nullptr,
                      RestoreOps{y, n, H, W, 0, mask}, t, c_recip, c_recipm1, c1, c2, sigma, nullptr, nullptr, B, channels, seed, stream_id, s);
}

int ddk_p_sample_update_restore_multistep(float* x, const float* eps_hat, float* x0_hist, const float* y, const float* mask, int n,
                                          const int64_t* t, const float* c_recip, const float* c_recipm1, const float* c1, const float* c2,
                                          const float* c3, int B, int H, int W, int channels, ddk_stream_t s) {
    return restore_op("p_sample_update_restore_multistep", StepKind::RestoreMultistep, x, eps_hat, x0_hist, RestoreOps{y, n, H, W, 0, mask}, t,
                      c_recip, c_recipm1, c1, c2, c3, nullptr, nullptr, B, channels, 0, 0, s);
}

int ddk_p_sample_update_restore_noisy(float* x, const float* eps_hat, const float* y, const float* mask, int n, const int64_t* t,
                                      const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* sigma,
                                      const float* lam, const float* sgm, int B, int H, int W, int channels, uint64_t seed, uint32_t stream_id,
                                      ddk_stream_t s) {
    return restore_op("p_sample_update_restore_noisy", StepKind::RestoreNoisy, x, eps_hat, nullptr, RestoreOps{y, n, H, W, 0, mask}, t, c_recip,
                      c_recipm1, c1, c2, sigma, lam, sgm, B, channels, seed, stream_id, s);
}

int ddk_p_sample_update_restore_gray(float* x, const float* eps_hat, const float* y, const float* mask, int n, int weights, const int64_t* t,
                                     const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* sigma,
                                     const float* lam, const float* sgm, int B, int H, int W, int channels, uint64_t seed, uint32_t stream_id,
                                     ddk_stream_t s) {
    DDK_REQUIRE(B > 0 && H > 0 && W > 0, "p_sample_update_restore_gray: B / H / W must be positive");
    DDK_REQUIRE(channels == 3, "p_sample_update_restore_gray: the grey operator needs a 3-channel map");
    DDK_REQUIRE(weights == GRAY_MEAN || weights == GRAY_LUMA, "p_sample_update_restore_gray: weights must be 1 (mean) or 2 (luma)");
    return restore_op("p_sample_update_restore_gray", StepKind::RestoreGray, x, eps_hat, nullptr, RestoreOps{y, n, H, W, weights, mask}, t,
                      c_recip, c_recipm1, c1, c2, sigma, lam, sgm, B, 3, seed, stream_id, s);
}

int ddk_final_tail(const float* raw, const float* partials, int tiles_per_image, const float* gamma, const float* beta, float eps,
                   const float* w, const float* bias, int n_out, float* eps_out, float* x, const float* noise, const int64_t* t,
                   const float* c_recip, const float* c_recipm1, const float* c1, const float* c2, const float* sigma, uint64_t seed,
                   uint32_t stream_id, int B, int HW, int C, int groups, ddk_stream_t s) {
    const StepRule r{x ? StepKind::Ancestral : StepKind::Eps, eps_out, x, noise, 0, 0, c_recip, c_recipm1, c1, c2, sigma};
    return final_tail(TailIn{raw, partials, tiles_per_image, gamma, beta, eps, w, bias, n_out, B, HW, C, groups}, r, t,
                      ChainHooks{nullptr, nullptr, seed, stream_id}, as_stream(s));
}

int ddk_randn(float* out, long long n, uint64_t seed, uint32_t step, uint32_t stream_id, ddk_stream_t s) {
    return randn(out, n, seed, step, stream_id, as_stream(s));
}

int ddk_fix_samples(const float* x_nchw, float* out_nhwc, int B, int C, int H, int W, ddk_stream_t s) {
    DDK_REQUIRE(x_nchw && out_nhwc && B > 0 && C > 0 && H > 0 && W > 0, "fix_samples: arguments");
    hipLaunchKernelGGL(fix_samples_kernel, dim3(B), dim3(1024), 0, as_stream(s), x_nchw, out_nhwc, C, (long long)H * W);
    return check_launch("fix_samples_kernel");
}

size_t ddk_vlb_terms_workspace_bytes(int B, long long per) {
    if (B <= 0 || per <= 0) return 0;
    return ((size_t)B + (size_t)B * vlb_slices(B, per) * 2) * sizeof(float);
}

int ddk_vlb_terms(const float* x, const float* x_t, const float* eps_hat, const float* eps, const int64_t* t, const float* c_recip,
                  const float* c_recipm1, const float* c1, const float* c2, const float* post_logvar, float* vlb, float* sqerr, int B,
                  long long per, void* workspace, size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(x && x_t && eps_hat && t && c_recip && c_recipm1 && c1 && c2 && post_logvar && vlb, "vlb_terms: null pointer");
    DDK_REQUIRE((eps == nullptr) == (sqerr == nullptr), "vlb_terms: eps and sqerr go together");
    DDK_REQUIRE(B > 0 && per > 0, "vlb_terms: B / per");
    DDK_REQUIRE(workspace && workspace_bytes >= ddk_vlb_terms_workspace_bytes(B, per) && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
                "vlb_terms: workspace (ddk_vlb_terms_workspace_bytes)");
    const int ns = vlb_slices(B, per);
    unsigned* counters = static_cast<unsigned*>(workspace);
    float* partials = static_cast<float*>(workspace) + B;
    DDK_HIP(hipMemsetAsync(counters, 0, (size_t)B * sizeof(unsigned), as_stream(s)));      // they re-arm themselves; a fresh workspace starts at 0
    hipLaunchKernelGGL(vlb_terms_kernel, dim3(ns, B), dim3(1024), 0, as_stream(s), x, x_t, eps_hat, eps, t, c_recip, c_recipm1, c1, c2,
                       post_logvar, vlb, sqerr, per, ns, counters, partials);
    return check_launch("vlb_terms_kernel");
}

int ddk_sq_err_sum(const float* a, const float* b, float* per_sample, int B, long long per, ddk_stream_t s) {
    DDK_REQUIRE(a && b && per_sample && B > 0 && per > 0 && per % 4 == 0, "sq_err_sum: arguments (per % 4 == 0)");
    DDK_REQUIRE(aligned16(a) && aligned16(b), "sq_err_sum: alignment");
    hipLaunchKernelGGL(sq_err_sum_kernel, dim3(B), dim3(1024), 0, as_stream(s), a, b, per_sample, per / 4);
    return check_launch("sq_err_sum_kernel");
}
}
