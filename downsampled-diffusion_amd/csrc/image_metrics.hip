// image_metrics.hip -- full-reference image quality of uint8 NHWC images: per-image squared-error sums (for PSNR) and SSIM
// (Wang, Bovik, Sheikh, Simoncelli, "Image quality assessment: from error visibility to structural similarity", IEEE TIP 2004).
// DESIGN.md section 3.7.
//
// Squared error: exact.  (a - b)^2 <= 255^2 and a 256 x 256 x 3 image already overflows 32 bits, so every sum is an unsigned 64-bit
// integer, and the per-image {sum, count} pair is accumulated with integer atomics: any arrival order gives the same bits.
//
// SSIM: 11 x 11 Gaussian window (sigma 1.5, the outer product of the normalised 1-D window), valid windows only, population moments.
// A workgroup owns TILE x TILE windows of one channel of one image: it stages the TILE + 10 square of both images in LDS as
// (value - 128), runs the 11 horizontal taps for the five maps a, b, a^2, b^2, ab into LDS, then the 11 vertical taps per window, and
// leaves the sum of its windows' SSIM in the workspace.  ssim_finish_kernel adds an image's partials in a fixed order.  The window
// values are fp32; their sums are carried in double (a few thousand additions per image, free next to the taps), so the mean adds one
// rounding to fp32 and nothing else.
//   * the shift by 128 is exact in fp32 and leaves variance and covariance unchanged; it quarters the magnitude of E[x^2] and mu^2,
//     whose difference is the variance, for bright images and removes it for mid-grey ones.  The luminance term gets the shift back.
//   * taps run in index order 0..10 and every product and sum is rounded on its own (this file is compiled with -ffp-contract=off,
//     see Makefile), so a window's value is the one the same expression gives in any fp32 arithmetic without FMA.
//   * no atomics and no arrival order anywhere in the SSIM path: the result is the same bits from run to run and for any batch.
#include "ddk_internal.h"

#include <cmath>

namespace ddk {

constexpr int SSIM_WIN = 11, SSIM_HALO = SSIM_WIN - 1, SSIM_TILE = 32, SSIM_IN = SSIM_TILE + SSIM_HALO;
constexpr int SSIM_THREADS = 256;                            // four waves: ssim_tile_kernel adds their sums by name
constexpr float SSIM_SHIFT = 128.0f;
constexpr float SSIM_C1 = (float)((0.01 * 255) * (0.01 * 255)), SSIM_C2 = (float)((0.03 * 255) * (0.03 * 255));

struct SsimWindow { float w[SSIM_WIN]; };

static SsimWindow ssim_window() {
    double g[SSIM_WIN], sum = 0.0;
    for (int i = 0; i < SSIM_WIN; ++i) {
        const double d = i - SSIM_WIN / 2;
        g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    SsimWindow o;
    for (int i = 0; i < SSIM_WIN; ++i) o.w[i] = (float)(g[i] / sum);
    return o;
}

static int sq_err_slices(long long pixels) {
    const long long ns = ceil_div(pixels, 256 * 16);          // ~16 pixels per thread
    return (int)(ns < 1 ? 1 : ns > 64 ? 64 : ns);
}

// slice sl of image n: out[n] += {sum (a - b)^2, number of elements} over its pixels (all C channels of a pixel whose mask is nonzero)
__global__ __launch_bounds__(256) void image_sq_err_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                           const uint8_t* __restrict__ mask, long long pixels, int C, int ns,
                                                           unsigned long long* __restrict__ out) {
    const int n = blockIdx.x / ns, sl = blockIdx.x % ns;
    const uint8_t* ap = a + (size_t)n * pixels * C;
    const uint8_t* bp = b + (size_t)n * pixels * C;
    const uint8_t* mp = mask ? mask + (size_t)n * pixels : nullptr;
    unsigned long long sum = 0, cnt = 0;
    for (long long p = sl * 256LL + threadIdx.x; p < pixels; p += ns * 256LL) {
        if (mp && mp[p] == 0) continue;
        for (int c = 0; c < C; ++c) {
            const int d = (int)ap[p * C + c] - (int)bp[p * C + c];
            sum += (unsigned)(d * d);
        }
        cnt += (unsigned)C;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt != 0) {
        atomicAdd(out + 2 * (size_t)n, sum);
        atomicAdd(out + 2 * (size_t)n + 1, cnt);
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workgroup = tile (ty, tx) of channel c of image n, blockIdx.x = ((n * C + c) * tiles_y + ty) * tiles_x + tx = its slot in partials
__global__ __launch_bounds__(SSIM_THREADS) void ssim_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W,
                                                                 int C, int tiles_y, int tiles_x, const SsimWindow g,
                                                                 double* __restrict__ partials) {
    __shared__ float sa[SSIM_IN][SSIM_IN], sb[SSIM_IN][SSIM_IN];
    __shared__ float hz[5][SSIM_IN][SSIM_TILE];
    __shared__ double red[SSIM_THREADS / 64];
    int q = blockIdx.x;
    const int tx = q % tiles_x;
    q /= tiles_x;
    const int ty = q % tiles_y;
    q /= tiles_y;
    const int c = q % C, n = q / C;
    const int y0 = ty * SSIM_TILE, x0 = tx * SSIM_TILE;
    const size_t img = (size_t)n * H * W * C;

    // the tile's windows read rows y0 .. y0 + TILE + 9 and as many columns; what lies outside the image is 0 and feeds no valid window
    for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += SSIM_THREADS) {
        const int r = i / SSIM_IN, col = i % SSIM_IN, y = y0 + r, x = x0 + col;
        float va = 0.0f, vb = 0.0f;
        if (y < H && x < W) {
            const size_t e = img + ((size_t)y * W + x) * C + c;
            va = (float)a[e] - SSIM_SHIFT;
            vb = (float)b[e] - SSIM_SHIFT;
        }
        sa[r][col] = va;
        sb[r][col] = vb;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SSIM_IN * SSIM_TILE; i += SSIM_THREADS) {
        const int r = i / SSIM_TILE, x = i % SSIM_TILE;
        float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float w = g.w[k], u = sa[r][x + k], v = sb[r][x + k];
            m[0] += w * u;
            m[1] += w * v;
            m[2] += w * (u * u);
            m[3] += w * (v * v);
            m[4] += w * (u * v);
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) hz[j][r][x] = m[j];
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = threadIdx.x; i < SSIM_TILE * SSIM_TILE; i += SSIM_THREADS) {
        const int y = i / SSIM_TILE, x = i % SSIM_TILE;
        if (y0 + y >= H - SSIM_HALO || x0 + x >= W - SSIM_HALO) continue;
        float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float w = g.w[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] += w * hz[j][y + k][x];
        }
        const float var_a = m[2] - m[0] * m[0], var_b = m[3] - m[1] * m[1], cov = m[4] - m[0] * m[1];
        const float mu_a = m[0] + SSIM_SHIFT, mu_b = m[1] + SSIM_SHIFT;
        const float num = (2.0f * (mu_a * mu_b) + SSIM_C1) * (2.0f * cov + SSIM_C2);
        const float den = ((mu_a * mu_a + mu_b * mu_b) + SSIM_C1) * ((var_a + var_b) + SSIM_C2);
        acc += (double)(num / den);
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per image: lane l adds partials l, l + 64, ... in that order, then the butterfly; ssim[n] = sum / windows
__global__ __launch_bounds__(64) void ssim_finish_kernel(const double* __restrict__ partials, int per_image, double windows,
                                                         float* __restrict__ ssim) {
    const double* p = partials + (size_t)blockIdx.x * per_image;
    double s = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 64) s += p[i];
    s = wave_sum_f64(s);
    if (threadIdx.x == 0) ssim[blockIdx.x] = (float)(s / windows);
}

static long long ssim_tiles(int H, int W, int* tiles_y, int* tiles_x) {
    *tiles_y = (int)ceil_div(H - SSIM_HALO, SSIM_TILE);
    *tiles_x = (int)ceil_div(W - SSIM_HALO, SSIM_TILE);
    return (long long)*tiles_y * *tiles_x;
}

}  // namespace ddk

using namespace ddk;

extern "C" {

size_t ddk_image_metrics_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || C < 1 || C > 4 || H < SSIM_WIN || W < SSIM_WIN) return 0;
    int ty, tx;
    return (size_t)N * C * (size_t)ssim_tiles(H, W, &ty, &tx) * sizeof(double);
}

int ddk_image_metrics(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int N, int H, int W, int C,
                      unsigned long long* sq_sum_count, float* ssim, void* workspace, size_t workspace_bytes, ddk_stream_t s) {
    DDK_REQUIRE(a && b && sq_sum_count && ssim, "image_metrics: null pointer");
    DDK_REQUIRE(N > 0 && C >= 1 && C <= 4, "image_metrics: N must be positive and C in 1..4");
    DDK_REQUIRE(H >= SSIM_WIN && W >= SSIM_WIN, "image_metrics: H and W must be at least 11 (one SSIM window)");
    DDK_REQUIRE((reinterpret_cast<uintptr_t>(sq_sum_count) & 7u) == 0, "image_metrics: sq_sum_count alignment");
    DDK_REQUIRE(workspace && workspace_bytes >= ddk_image_metrics_workspace_bytes(N, H, W, C) &&
                    (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
                "image_metrics: workspace (ddk_image_metrics_workspace_bytes)");
    int tiles_y, tiles_x;
    const long long tiles = ssim_tiles(H, W, &tiles_y, &tiles_x), pixels = (long long)H * W;
    const int ns = sq_err_slices(pixels);
    DDK_REQUIRE((long long)N * C * tiles <= INT32_MAX && (long long)N * ns <= INT32_MAX && (long long)C * tiles <= INT32_MAX,
                "image_metrics: too many tiles for one launch");
    double* partials = static_cast<double*>(workspace);
    DDK_HIP(hipMemsetAsync(sq_sum_count, 0, (size_t)N * 2 * sizeof(unsigned long long), as_stream(s)));
    hipLaunchKernelGGL(image_sq_err_kernel, dim3((unsigned)(N * ns)), dim3(256), 0, as_stream(s), a, b, mask, pixels, C, ns, sq_sum_count);
    DDK_TRY(check_launch("image_sq_err_kernel"));
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)((long long)N * C * tiles)), dim3(SSIM_THREADS), 0, as_stream(s), a, b, H, W, C,
                       tiles_y, tiles_x, ssim_window(), partials);
    DDK_TRY(check_launch("ssim_tile_kernel"));
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(N), dim3(64), 0, as_stream(s), (const double*)partials, (int)(C * tiles),
                       (double)C * (double)(H - SSIM_HALO) * (double)(W - SSIM_HALO), ssim);
    return check_launch("ssim_finish_kernel");
}
}
