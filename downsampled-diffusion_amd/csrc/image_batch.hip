// image_batch.hip -- a training batch from a resident uint8 image array in one launch.
//
// out[b] = the reference's transform chain (utils/data.py:48-84: ToTensor -> Resize(S) -> CenterCrop(S) -> t * 2 - 1 -> RandomHorizontalFlip)
// of images[index[b]], fp32 NCHW.  The resize is separable and the crop selects rows of its two matrices, so the host hands over two tap
// tables (utils/image_batch.py): S rows of `taps` weights from a start index, along H and along W.
//
// A workgroup takes one image and a band of output rows (ddk_image_batch_rows_per_group), in chunks of source rows that fit its LDS:
//   A  the chunk's source rows are ONE contiguous byte span of the image: it is copied to LDS with aligned 4-byte loads, at the
//      span's own phase mod 4; a word that straddles an end of the IMAGE is assembled from the bytes inside it, so nothing outside
//      the image is read (an image's base, index Hs Ws C bytes, is in general not aligned: 7 x 5 x 3 = 105);
//   B  every source row is resampled along W into LDS as fp32, T[row][c][x] = sum_k col_w[x][k] * unit[byte], unit[] the 256 correctly
//      rounded quotients i / 255 (one IEEE division per thread, in LDS);
//   C  the band's output rows are combined along H out of T, four x per thread: v * 2 - 1, one 16-byte store, mirrored in x when the
//      image's flip bit is set.
// Taps are summed in increasing index, each with one fmaf, W first and then H: the bits of an image depend on nothing but the image,
// the tables and its flip bit.  A single chunk is the rule: the host sizes the band from the scale so that its source rows fit; the
// chunk loop is what makes ANY table safe (starts are clamped as well), not a second code path with other results.
#include "ddk_internal.h"
#include "diffusion_step.h"

namespace ddk {

constexpr int IB_THREADS = 256;
constexpr int IB_LDS_BUDGET = 64 * 1024;          // per workgroup, the unit table included
constexpr int IB_UNIT_BYTES = 256 * 4;
constexpr uint32_t IB_FLIP_WORD = 0x464c4950u;    // 'FLIP': counter word 3 of the flip draw

struct ImageBatch {
    const uint8_t* images;
    long long n_images;
    const int64_t* index;
    const int32_t* row_start;
    const float* row_w;
    const int32_t* col_start;
    const float* col_w;
    float* out;
    uint64_t seed;
    uint32_t epoch;
    int Hs, Ws, C, S, row_taps, col_taps, flip, rows_per_group, cap_rows, raw_bytes;
};

__device__ __forceinline__ int ib_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int C>
__global__ __launch_bounds__(IB_THREADS) void image_batch_kernel(const ImageBatch p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ib_lds[];
    float* unit = reinterpret_cast<float*>(ib_lds);
    uint32_t* raw_w = reinterpret_cast<uint32_t*>(ib_lds + IB_UNIT_BYTES);
    const unsigned char* raw_b = ib_lds + IB_UNIT_BYTES;
    float* T = reinterpret_cast<float*>(ib_lds + IB_UNIT_BYTES + p.raw_bytes);

    const int S = p.S, Hs = p.Hs, Ws = p.Ws, rt = p.row_taps, ct = p.col_taps, tid = threadIdx.x;
    const int b = blockIdx.y, y_begin = blockIdx.x * p.rows_per_group, y_end = min(S, y_begin + p.rows_per_group);
    const int S4 = S >> 2;
    float* __restrict__ out = p.out + (size_t)b * C * S * S;
    const long long id = p.index[b];
    if (id < 0 || id >= p.n_images) {             // nothing of `images` is read: the band is NaN
        const float nan = __int_as_float(0x7fc00000);
        const float4 n4 = make_float4(nan, nan, nan, nan);
        for (int i = tid; i < (y_end - y_begin) * C * S4; i += IB_THREADS) {
            const int x4 = i % S4, yc = i / S4, c = yc % C, y = y_begin + yc / C;
            reinterpret_cast<float4*>(out + ((size_t)c * S + y) * S)[x4] = n4;
        }
        return;
    }
    unit[tid] = (float)tid / 255.0f;              // IB_THREADS == 256; read after the first barrier below
    const size_t row_bytes = (size_t)Ws * C, img_bytes = (size_t)Hs * row_bytes;
    const uint8_t* img_lo = p.images + (size_t)id * img_bytes;
    const uint8_t* img_hi = img_lo + img_bytes;
    bool mirror = false;
    if (p.flip)
        mirror = philox4x32_10(U4{(uint32_t)id, (uint32_t)((unsigned long long)id >> 32), p.epoch, IB_FLIP_WORD}, (uint32_t)p.seed,
                               (uint32_t)(p.seed >> 32)).x & 1u;

    for (int y0 = y_begin; y0 < y_end;) {
        // the chunk: output rows [y0, y1) whose source rows [lo, hi) fit the LDS (cap_rows >= row_taps: one row always fits)
        int lo = ib_clamp(p.row_start[y0], Hs - rt), hi = lo + rt, y1 = y0 + 1;
        for (; y1 < y_end; ++y1) {
            const int st = ib_clamp(p.row_start[y1], Hs - rt);
            const int nlo = min(lo, st), nhi = max(hi, st + rt);
            if (nhi - nlo > p.cap_rows) break;
            lo = nlo; hi = nhi;
        }
        const int nsrc = hi - lo;
        // A: the span's bytes at LDS byte offset head + i
        const uint8_t* span = img_lo + (size_t)lo * row_bytes;
        const int head = (int)(reinterpret_cast<uintptr_t>(span) & 3u);
        const uint8_t* a4 = span - head;
        const int nwords = (int)((head + (size_t)nsrc * row_bytes + 3) >> 2);
        for (int d = tid; d < nwords; d += IB_THREADS) {
            const uint8_t* q = a4 + 4 * (size_t)d;
            uint32_t v = 0;
            if (q >= img_lo && q + 4 <= img_hi) {
                v = *reinterpret_cast<const uint32_t*>(q);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q + j >= img_lo && q + j < img_hi) v |= (uint32_t)q[j] << (8 * j);
            }
            raw_w[d] = v;
        }
        __syncthreads();
        // B: T[r][c][x], x fastest over the threads
        for (int i = tid; i < nsrc * S; i += IB_THREADS) {
            const int x = i % S, r = i / S;
            const int cs = ib_clamp(p.col_start[x], Ws - ct);
            const float* __restrict__ w = p.col_w + (size_t)x * ct;
            const unsigned char* src = raw_b + head + (size_t)r * row_bytes + (size_t)cs * C;
            float acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.f;
            for (int k = 0; k < ct; ++k) {
                const float wk = w[k];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = fmaf(wk, unit[src[k * C + c]], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) T[((size_t)r * C + c) * S + x] = acc[c];
        }
        __syncthreads();
        // C: four x of one (y, c) per thread
        for (int i = tid; i < (y1 - y0) * C * S4; i += IB_THREADS) {
            const int x4 = i % S4, yc = i / S4, c = yc % C, y = y0 + yc / C;
            const int st = ib_clamp(p.row_start[y], Hs - rt) - lo;
            const float* __restrict__ w = p.row_w + (size_t)y * rt;
            const float4* t4 = reinterpret_cast<const float4*>(T + ((size_t)st * C + c) * S) + x4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < rt; ++k) {
                const float wk = w[k];
                const float4 v = t4[(size_t)k * C * S4];
                acc.x = fmaf(wk, v.x, acc.x); acc.y = fmaf(wk, v.y, acc.y); acc.z = fmaf(wk, v.z, acc.z); acc.w = fmaf(wk, v.w, acc.w);
            }
            float4 o = make_float4(fmaf(acc.x, 2.0f, -1.0f), fmaf(acc.y, 2.0f, -1.0f), fmaf(acc.z, 2.0f, -1.0f), fmaf(acc.w, 2.0f, -1.0f));
            int xo = x4;
            if (mirror) {
                o = make_float4(o.w, o.z, o.y, o.x);
                xo = S4 - 1 - x4;
            }
            reinterpret_cast<float4*>(out + ((size_t)c * S + y) * S)[xo] = o;
        }
        y0 = y1;
        // the next chunk's A writes raw, last read in B (a barrier ago); its B writes T only after A's barrier, which every wave reaches after C
    }
}

// the band and its LDS: everything the launch derives from the shape, host arithmetic only
struct ImageBatchGeometry {
    int rows_per_group;       // 0: the shape is not taken
    int cap_rows;             // source rows a chunk may hold
    int raw_bytes;            // the byte span's part of the LDS (a multiple of 16)
    size_t lds_bytes;
};

static ImageBatchGeometry image_batch_geometry(int Hs, int Ws, int C, int S, int row_taps, int col_taps) {
    ImageBatchGeometry g{0, 0, 0, 0};
    if (Hs < 1 || Ws < 1 || Hs > 16384 || Ws > 16384 || C < 1 || C > 4 || S < 4 || S > 1024 || S % 4 != 0) return g;
    if (row_taps < 1 || row_taps > 32 || col_taps < 1 || col_taps > 32 || row_taps > Hs || col_taps > Ws) return g;
    const long long row_bytes = (long long)Ws * C, t_row = (long long)S * C * 4;
    // unit table + (cap row_bytes + 3 head bytes, rounded up to 16) + cap t_row <= the budget
    const long long cap = (IB_LDS_BUDGET - IB_UNIT_BYTES - 3 - 15) / (row_bytes + t_row);
    if (cap < row_taps) return g;
    // the resized height is torchvision's Resize(S): the short side becomes S, the long side int(S long / short); an output row's taps
    // start within one source row of scale (y + 0.5) - support, so R rows span at most (R - 1) scale + taps + 1 source rows
    const int Ho = Hs <= Ws ? S : (int)((double)((long long)S * Hs) / (double)Ws);
    const double scale = (double)Hs / (double)(Ho > 0 ? Ho : 1);
    long long r = cap > row_taps ? 1 + (long long)((double)(cap - row_taps - 1) / scale) : 1;
    const long long want = S / 4 > 4 ? S / 4 : 4;           // at least four bands of an image once S >= 16: B images fill the device
    if (r > want) r = want;
    if (r > S) r = S;
    if (r < 1) r = 1;
    g.rows_per_group = (int)r;
    g.cap_rows = (int)(cap < Hs ? cap : Hs);
    g.raw_bytes = (int)((g.cap_rows * row_bytes + 3 + 15) / 16 * 16);
    g.lds_bytes = (size_t)IB_UNIT_BYTES + g.raw_bytes + (size_t)g.cap_rows * t_row;
    return g;
}

}  // namespace ddk

using namespace ddk;

extern "C" {

int ddk_image_batch_rows_per_group(int Hs, int Ws, int C, int S, int row_taps, int col_taps) {
    return image_batch_geometry(Hs, Ws, C, S, row_taps, col_taps).rows_per_group;
}

int ddk_image_batch(const uint8_t* images, long long n_images, int Hs, int Ws, int C, const int64_t* index, int B, const int32_t* row_start,
                    const float* row_w, int row_taps, const int32_t* col_start, const float* col_w, int col_taps, int S, int flip,
                    uint64_t seed, uint32_t epoch, float* out, ddk_stream_t s) {
    DDK_REQUIRE(images && index && row_start && row_w && col_start && col_w && out, "image_batch: null pointer");
    DDK_REQUIRE(C >= 1 && C <= 4, "image_batch: C must be in 1..4");
    DDK_REQUIRE(S >= 4 && S <= 1024 && S % 4 == 0, "image_batch: S must be a multiple of 4 in [4, 1024]");
    DDK_REQUIRE(row_taps >= 1 && row_taps <= 32 && col_taps >= 1 && col_taps <= 32, "image_batch: taps must be in 1..32");
    DDK_REQUIRE(B >= 1 && B <= 65535 && n_images >= 1, "image_batch: B must be in 1..65535 and n_images positive");
    DDK_REQUIRE(aligned16(out), "image_batch: out must be 16-byte aligned");
    DDK_REQUIRE((reinterpret_cast<uintptr_t>(index) & 7u) == 0 && (reinterpret_cast<uintptr_t>(row_start) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(row_w) & 3u) == 0 && (reinterpret_cast<uintptr_t>(col_start) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(col_w) & 3u) == 0, "image_batch: index and the tables must be aligned to their elements");
    const ImageBatchGeometry g = image_batch_geometry(Hs, Ws, C, S, row_taps, col_taps);
    DDK_REQUIRE(g.rows_per_group > 0,
                "image_batch: the source must be 1..16384 a side with no fewer rows / columns than taps, and one output row's source rows "
                "must fit 64 KB of LDS");
    const ImageBatch p{images, n_images, index, row_start, row_w, col_start, col_w, out, seed, epoch, Hs, Ws, C, S, row_taps, col_taps,
                       flip != 0, g.rows_per_group, g.cap_rows, g.raw_bytes};
    const dim3 grid((S + g.rows_per_group - 1) / g.rows_per_group, B);
    hipStream_t st = as_stream(s);
    switch (C) {
        case 1: hipLaunchKernelGGL(image_batch_kernel<1>, grid, dim3(IB_THREADS), g.lds_bytes, st, p); break;
        case 2: hipLaunchKernelGGL(image_batch_kernel<2>, grid, dim3(IB_THREADS), g.lds_bytes, st, p); break;
        case 3: hipLaunchKernelGGL(image_batch_kernel<3>, grid, dim3(IB_THREADS), g.lds_bytes, st, p); break;
        default: hipLaunchKernelGGL(image_batch_kernel<4>, grid, dim3(IB_THREADS), g.lds_bytes, st, p); break;
    }
    return check_launch("image_batch_kernel");
}

}  // extern "C"
