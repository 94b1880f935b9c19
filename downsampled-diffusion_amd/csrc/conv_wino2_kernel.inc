// conv_wino2_kernel.inc -- included by conv_wino.hip (shares WinoParams, make_srd, buf_load16, the fragment conventions).
//
// Round 4: the Winograd conv with EIGHT matrix waves (two per SIMD) and four loader waves, 768 threads, <= 168 registers.
// Why (DESIGN.md section 3.1g; profiles/r03_wino_clock.txt): the 4 + 4 kernel above runs 2654 cycles per 2048-cycle stage --
// ~230 of the excess are the loader wave's VALU / issue slots taken out of the SIMD it shares with a matrix wave (the fp32 MFMA
// runs on the vector lanes), ~280 the matrix wave's own non-MFMA instructions (DMA issue, LDS reads, waits) with nobody to fill
// the pipe meanwhile, ~100 the barrier; and at 32x32 (512 workgroups, one per CU) every workgroup pays its prologue and epilogue
// twice per CU.  Here
//   * two matrix waves share a SIMD and fill each other's issue gaps (16 MFMAs per wave and stage on ONE accumulator each);
//   * variant F (P = 2): a workgroup covers 32 tiles x 128 output channels, so the input transform V -- the loader's VALU work
//     and its patch loads -- is shared by two n tiles: half the VALU per MFMA, and the 32x32 maps are ONE dispatch round of 256
//     workgroups; a stage = 2 positions (V 8 KB + U 32 KB = 40 KB, 3 stages = 120 KB), wave (pp, nb) keeps 8 accumulators
//     (position 2s + pp of every stage s of a chunk, n block nb);
//   * variant D (P = 4): 32 tiles x 64 output channels as before for the shapes with too few tiles for F (16x16, 8x8 at batch
//     32: 256 workgroups only exist at 64 channels per workgroup); a stage = 4 positions as above, wave (pp, nb) keeps 4;
//   * the loader holds ONE 4x4 patch (64 registers, was two): patch row r of the next chunk is requested as soon as the last V
//     row that needs row r of this chunk has been written (V row i needs patch rows {0,2}, {1,2}, {1,2}, {1,3}).
// U is the same packed tensor ([cin/32][16][N][32]); the epilogue, the GroupNorm statistics and the in-launch GroupNorm exchange
// are those of the kernel above, generalised to the tile width.

template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }    // f(integral_constant<int, i>) for i = 0 .. N-1

#ifndef DDK_WINO2_LP_F
#define DDK_WINO2_LP_F 8
#endif
#ifndef DDK_WINO2_LP_D
#define DDK_WINO2_LP_D 4
#endif
template <int P>
struct W2 {
    static constexpr int NT = 256 / P;              // output channels per workgroup: 128 (P = 2) or 64 (P = 4)
    static constexpr int NB = NT / 32;              // 32-channel blocks; matrix waves = P * NB = 8
    static constexpr int SPC = 16 / P;              // stages per 32-channel chunk
    static constexpr int SPR = 4 / P;               // stages per V row (the 4 positions 4i .. 4i+3)
    static constexpr int V_FL = P * WBT * 32;       // floats of a stage's V images
    static constexpr int U_FL = P * NT * 32;        // ... and U images (8192 either way)
    static constexpr int STAGE = V_FL + U_FL;
    static constexpr int PPI = NT / 8;              // 1-KiB DMA pieces per U image
    static constexpr int TP = NT + 4;               // epilogue staging pitch
    static constexpr int T_FL = 4 * 2 * WBT * TP;   // 4 blocks of 64 rows: D the 4 position columns, F (wave pp, output column b)
    static constexpr int LDS_FL = (3 * STAGE > T_FL + 320) ? 3 * STAGE : T_FL + 320;
    static constexpr int QUADS = NT / 4;            // channel quads per pixel row of the tile
    static constexpr int ITEMS = 2 * WBT * QUADS / 512;   // float4 pairs per thread of the 512 finishing threads
    // of a stage's 32 U pieces each loader wave issues LPL, each matrix wave LPM.  F's loaders have the slack to issue them all
    // (they arrive at the stage barrier ~1500 cycles early: profiles/r04_wino_clock.txt); D's do twice the V work per stage and split
    static constexpr int LPL = P == 2 ? DDK_WINO2_LP_F : DDK_WINO2_LP_D;
    static constexpr int LPM = (32 - 4 * LPL) / 8;
    static_assert(4 * LPL + 8 * LPM == 32 && LPL % 2 == 0 && LPM % 2 == 0, "piece split: (8,0), (4,2) or (0,4)");
};
#ifndef DDK_WINO2_STAGGER
#define DDK_WINO2_STAGGER 1
#endif
constexpr bool W2_STAGGER = DDK_WINO2_STAGGER != 0;  // waves 4..7 run one quarter-stage behind their SIMD partners (see the matrix loop)

// DBG (tuning build only; anything but 0 / 1 gives wrong results): 1 summary stamps per workgroup, 2 loaders issue no U pieces,
// 4 matrix waves issue none, 8 loaders do no V work (no patch loads, no transform, no LDS writes), 16 per-wave barrier timeline of
// workgroup 0 (stages 8..15) into g_wino_timeline
__device__ unsigned long long g_wino_timeline[12 * 8 * 2];

// SK (variant D only): the ResnetBlock's 1x1 skip conv of the SAME input rides along (DESIGN.md 3.1l).  The four
// inner positions 5, 6, 9, 10 of V = B^T d B are a 2x2 Hadamard transform of the patch centre -- the tile's own four pixels -- so
// S_p = (W1 / 4) . V_p for those p, combined with the transform's signs, is the 1x1 conv at those pixels.  The waves that own these
// positions (pp = 1, 2; stages 1, 2) multiply their A fragments a second time, against W1 fragments streamed from L2 into registers.
template <int P, int DBG, bool CL, bool SK = false>
__global__ __launch_bounds__(768) void conv3x3_wino2_kernel(const WinoParams p) {
    using G = W2<P>;
    static_assert(!SK || (P == 4 && DBG == 0), "the skip fold exists on variant D");
    static_assert(!SK || G::T_FL + 320 + 2 * 2 * WBT * G::TP <= G::LDS_FL, "the skip tile is staged behind the conv's");
    constexpr int NT = G::NT, SPC = G::SPC, SPR = G::SPR, STAGE = G::STAGE, V_FL = G::V_FL;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned long long r_entry = 0;
    if (DBG) r_entry = __builtin_amdgcn_s_memrealtime();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tile_m, tile_n, split;
    {   // XCD-aware order: every XCD gets a contiguous run of (n fastest, then m, then split) tiles
        const int nwg = gridDim.x * gridDim.y * gridDim.z;
        const int bid = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        const int logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        tile_n = logical % gridDim.y;
        const int rest = logical / gridDim.y;
        tile_m = rest % gridDim.x;
        split = rest / gridDim.x;
    }
    const int t0 = tile_m * WBT, n0 = tile_n * NT;
    const int c_begin = split * p.chunks_per_split;
    const int n_chunks = min(p.chunks, c_begin + p.chunks_per_split) - c_begin;
    const int n_stages = n_chunks * SPC;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;
    // per-lane part of a U piece's source offset: 8 rows x 128 B, k-chunk position XOR-swizzled by (row >> 1) & 7; the row block
    // rb of a piece only enters through its parity (4 * rb & 7), everything else of the address is wave-uniform
    const int prow = lane >> 3, ppos = lane & 7;
    const unsigned uv_even = (unsigned)((prow * 32 + ((ppos ^ (prow >> 1)) << 2)) * 4);
    const unsigned uv_odd = (unsigned)((prow * 32 + ((ppos ^ (4 + (prow >> 1))) << 2)) * 4);
    // U pieces of stage T (relative to this workgroup's first): piece g in [0, 32) = image g / PPI (position P * st + image),
    // row block g % PPI; issued into stage buffer `buf`
    auto issue_u = [&](int T, int buf, int g_first, auto count) {
        const int chunk = c_begin + T / SPC, st = T % SPC;
        const float* base = p.wu + (((long long)chunk * 16 + P * st) * p.N + n0) * 32;
        const unsigned dst = lds_base + (unsigned)((buf * STAGE + V_FL) * 4);
#pragma unroll
        for (int j = 0; j < decltype(count)::value; ++j) {
            const int g = g_first + j;                       // g_first is even: parity of the row block = parity of j
            const int image = g / G::PPI, rb = g % G::PPI;
            lds_dma16_s(base + ((long long)image * p.N + rb * 8) * 32, (j & 1) ? uv_odd : uv_even, dst + (unsigned)(g * 1024));
        }
    };

    if (wid >= 8) {
        // ================================================================ loader wave
        const int lw = wid - 8;
        const int lt = lw * 64 + lane;
        const int t = lt >> 3, cq = lt & 7;
        __builtin_amdgcn_s_setprio(3);
        const int g = t0 + t;
        const bool tile_ok = g < p.tiles;
        const unsigned gg = tile_ok ? (unsigned)g : 0u;
        const unsigned tmp = fdiv_u(gg, p.dTW);
        const int tx = (int)(gg - tmp * (unsigned)p.TW);
        const unsigned bq = fdiv_u(tmp, p.dTH);
        const int ty = (int)(tmp - bq * (unsigned)p.TH), b = (int)bq;
        const int py0 = 2 * ty - 1, px0 = 2 * tx - 1;
        const int pix0 = (b * p.H + py0) * p.W + px0;          // may be "negative": only used where the mask says valid
        unsigned mask = 0;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx)
                if (tile_ok && (unsigned)(py0 + dy) < (unsigned)p.H && (unsigned)(px0 + dx) < (unsigned)p.W) mask |= 1u << (dy * 4 + dx);
        const i32x4 srd0 = make_srd(p.src0, (unsigned)((long long)p.B * p.H * p.W * p.c0 * 4));
        const i32x4 srd1 = make_srd(p.src1 ? p.src1 : p.src0, (unsigned)((long long)p.B * p.H * p.W * (p.src1 ? p.c1 : p.c0) * 4));
        unsigned voff[16];
        int cur_src = -1;
        auto set_source = [&](int which) {
            const int cs = which == 0 ? p.c0 : p.c1;
#pragma unroll
            for (int dy = 0; dy < 4; ++dy)
#pragma unroll
                for (int dx = 0; dx < 4; ++dx)
                    voff[dy * 4 + dx] = ((mask >> (dy * 4 + dx)) & 1u) ? (unsigned)(((pix0 + dy * p.W + dx) * cs + cq * 4) * 4) : WINO_OOB;
            cur_src = which;
        };
        const int v_off = t * 32 + ((cq ^ ((t >> 1) & 7)) << 2);     // float offset of this thread's float4 inside a V image
        f32x4 d[16];                                                   // the 4x4 patch (4 channels): ONE buffer, rows refilled as they retire
        // NOTE the two sources (concat-free skip) have different pixel strides: a patch row loaded from source 1 while rows of
        // source 0 are still live is fine -- voff is only read by the loads themselves, and set_source runs in front of them.
        auto load_row = [&](int chunk, int row) {
            const int cc = chunk << 5;
            const bool first = cc < p.c0;                              // wave-uniform
            if ((first ? 0 : 1) != cur_src) set_source(first ? 0 : 1);
            const unsigned soff = (unsigned)((first ? cc : cc - p.c0) * 4);
            i32x4 srd;
            srd.x = first ? srd0.x : srd1.x; srd.y = first ? srd0.y : srd1.y; srd.z = first ? srd0.z : srd1.z; srd.w = srd0.w;
#pragma unroll
            for (int dy = 0; dy < 4; ++dy)
                if (dy == row) {
#pragma unroll
                    for (int dx = 0; dx < 4; ++dx) buf_load16(d[dy * 4 + dx], voff[dy * 4 + dx], srd, soff);
                }
        };
        auto pin = [&]() {        // no use of the patch registers may move above this point (their loads are invisible to the compiler)
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(d[i]));
        };
        // half (h) of V row k = B^T d B row k, into the V images of stage buffer `buf`: B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]
        auto write_v = [&](auto kc, auto hc, int buf) {
            constexpr int k = decltype(kc)::value, h = decltype(hc)::value;
            auto rowc = [&](auto xc) -> f32x4 {
                constexpr int x = decltype(xc)::value;
                if constexpr (k == 0) return d[0 * 4 + x] - d[2 * 4 + x];
                else if constexpr (k == 1) return d[1 * 4 + x] + d[2 * 4 + x];
                else if constexpr (k == 2) return d[2 * 4 + x] - d[1 * 4 + x];
                else return d[1 * 4 + x] - d[3 * 4 + x];
            };
            using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
            float* base = smem + buf * STAGE + v_off;
            if constexpr (P == 4) {
                const f32x4 r0 = rowc(I0{}), r1 = rowc(I1{}), r2 = rowc(I2{}), r3 = rowc(I3{});
                *reinterpret_cast<f32x4*>(base + 0 * (WBT * 32)) = r0 - r2;
                *reinterpret_cast<f32x4*>(base + 1 * (WBT * 32)) = r1 + r2;
                *reinterpret_cast<f32x4*>(base + 2 * (WBT * 32)) = r2 - r1;
                *reinterpret_cast<f32x4*>(base + 3 * (WBT * 32)) = r1 - r3;
            } else if constexpr (h == 0) {
                const f32x4 r0 = rowc(I0{}), r1 = rowc(I1{}), r2 = rowc(I2{});
                *reinterpret_cast<f32x4*>(base + 0 * (WBT * 32)) = r0 - r2;      // position 4k + 0 -> image 0
                *reinterpret_cast<f32x4*>(base + 1 * (WBT * 32)) = r1 + r2;      // position 4k + 1 -> image 1
            } else {
                const f32x4 r1 = rowc(I1{}), r2 = rowc(I2{}), r3 = rowc(I3{});
                *reinterpret_cast<f32x4*>(base + 0 * (WBT * 32)) = r2 - r1;      // position 4k + 2
                *reinterpret_cast<f32x4*>(base + 1 * (WBT * 32)) = r1 - r3;      // position 4k + 3
            }
        };
        // Everything a loader does for stage T (ts = T % SPC, a compile-time value in the unrolled loop; tc = chunk of T relative to
        // c_begin): the V images, then -- when ts closes a V row -- the patch row that this retires (k = 0: row 0 of the NEXT chunk;
        // k = 1: row 3 of THIS chunk, first needed by its V row 3; k = 2: row 2 of the next chunk; k = 3: row 1 of the next chunk),
        // then its share of the U pieces.  Returns the number of vector-memory operations issued (for the counted wait).
        auto produce = [&](auto tsc, int T, int tc, int buf) -> bool {
            constexpr int ts = decltype(tsc)::value, k = ts / SPR, h = ts % SPR;
            if (!(DBG & 8)) write_v(std::integral_constant<int, k>{}, std::integral_constant<int, h>{}, buf);
            bool loaded = false;
            if constexpr (h == SPR - 1 && !(DBG & 8)) {
                if (k == 1) { load_row(c_begin + tc, 3); loaded = true; }
                else if (tc + 1 < n_chunks) { load_row(c_begin + tc + 1, k == 0 ? 0 : k == 2 ? 2 : 1); loaded = true; }
            }
            if (!(DBG & 2)) issue_u(T, buf, lw * G::LPL, std::integral_constant<int, G::LPL>{});
            return loaded;
        };
        // prologue: the first barrier only needs stage 0's operands and V of stage 1 (the matrix waves prefetch their next A fragment
        // across a barrier): U(1) -- and for F, whose first two stages are both halves of V row 0, patch row 1 -- stay in flight
        // behind it.  Issue order = completion order: rows 0 and 2, [row 1 if D], U(0), [row 1 if F], U(1).
        load_row(c_begin, 0);
        load_row(c_begin, 2);
        if (P == 4) load_row(c_begin, 1);
        if (!(DBG & 2)) issue_u(0, 0, lw * G::LPL, std::integral_constant<int, G::LPL>{});
        if (P == 2) load_row(c_begin, 1);
        constexpr int NPL0 = (DBG & 2) ? 0 : G::LPL;
        wait_vmcnt<NPL0 + (P == 2 ? 4 : 0)>();                             // the rows V(0) and V(1) are built from
        pin();
        using K0 = std::integral_constant<int, 0>;
        if (!(DBG & 8)) {
            write_v(K0{}, K0{}, 0);                                         // V(0)
            if (P == 2) write_v(K0{}, std::integral_constant<int, SPR - 1>{}, 1);               // V(1): F the other half of row 0
            else write_v(std::integral_constant<int, 1 / SPR>{}, K0{}, 1);                      //       D row 1
            // what these two stages retire (the rule of produce() below): row 0 of the next chunk, and for D row 3 of this one
            if (1 < n_chunks) load_row(c_begin + 1, 0);
            if (P == 4) load_row(c_begin, 3);
        }
        if (!(DBG & 2)) issue_u(1, 1, lw * G::LPL, std::integral_constant<int, G::LPL>{});
        // outstanding behind this wait at most: [row 1 (F)], [next row 0], [row 3 (D)], U(1) -- all younger than U(0)
        if (DBG & 8) wait_vmcnt<NPL0>();
        else if (P == 2) { if (1 < n_chunks) wait_vmcnt<NPL0 + 8>(); else wait_vmcnt<NPL0 + 4>(); }
        else { if (1 < n_chunks) wait_vmcnt<NPL0 + 8>(); else wait_vmcnt<NPL0 + 4>(); }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                       // B0: stage 0 complete, V(1) written; U(1) lands before B(1)
        // Iteration S (after barrier B(S)): stage S - 1's buffer is free -> produce stage S + 2 into it.  Nothing waits for what it has
        // just issued: in front of B(S + 1) a loader waits only for what it issued BEFORE this iteration (counted vmcnt), so a patch
        // row requested in iteration X is guaranteed in registers from iteration X + 2 on -- the schedule above never reads one earlier.
        int b0 = 0;
        for (int qi = 0; qi < n_chunks; ++qi) {
            static_for<SPC>([&](auto sc) {
                constexpr int s = decltype(sc)::value;
                const int S = qi * SPC + s;
                const int buf2 = b0 == 0 ? 2 : b0 - 1;                      // (S + 2) % 3 == (S - 1) % 3
                const bool more = S + 2 < n_stages;
                if (s == 0 && qi == 0) wait_vmcnt<((DBG & 2) ? 0 : G::LPL)>();   // the prologue's late loads (only U(1) may still be in flight)
                pin();
                bool loaded = false;
                if (more) {
                    constexpr int ts = (s + 2) % SPC;
                    loaded = produce(std::integral_constant<int, ts>{}, S + 2, qi + (s + 2 >= SPC ? 1 : 0), buf2);
                }
                constexpr int NPL = (DBG & 2) ? 0 : G::LPL;
                if (more) { if (loaded) wait_vmcnt<NPL + 4>(); else wait_vmcnt<NPL>(); }
                else wait_vmcnt<0>();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                unsigned long long tlA = 0;
                const bool tl = (DBG & 16) && blockIdx.x + blockIdx.y + blockIdx.z == 0 && S >= 8 && S < 16;
                if (tl) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlA)::"memory");
                __builtin_amdgcn_s_barrier();                               // B(S+1)
                if (tl) {
                    unsigned long long tlB;
                    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlB)::"memory");
                    if (lane == 0) { g_wino_timeline[(wid * 8 + (S - 8)) * 2] = tlA; g_wino_timeline[(wid * 8 + (S - 8)) * 2 + 1] = tlB; }
                }
                b0 = b0 == 2 ? 0 : b0 + 1;
            });
        }
        return;                                                             // (terminated waves leave the barrier count)
    }

    // ================================================================ matrix wave (pp, nb)
    // SK: waves w and w + 4 share a SIMD; the extra multiplies belong to pp = 1, 2, so waves 4..7 swap pp pairwise and every SIMD
    // carries exactly one such wave (pp only names the position a wave owns: a_img, b_img and its staging block below follow it)
    const int pp = (SK && wid >= 4) ? ((wid % P) ^ 1) : wid % P, nb = wid / P;
    const bool skw = SK && (pp == 1 || pp == 2);                        // wave-uniform
    f32x16 sk[2];                                                       // SK: S_(4 + pp) (stage 1), S_(8 + pp) (stage 2)
    f32x4 w1[4];                                                        // SK: this chunk's W1 / 4 fragments of n block nb, one per quarter
    if constexpr (SK) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sk[i][r] = 0.f;
    }
    f32x16 acc[SPC];
#pragma unroll
    for (int i = 0; i < SPC; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    {
        const int fsw = ((lane & 31) >> 1) & 7, fh = lane >> 5;
        int foff[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) foff[q] = (lane & 31) * 32 + (((2 * q + fh) ^ fsw) << 2);
        const int a_img = pp * (WBT * 32), b_img = V_FL + (pp * NT + nb * 32) * 32;
        // W1 / 4 in MFMA operand order, [chunk][N / 32][quarter][lane] float4 (ddk_pack_conv_skip_weight_wino): 4 loads of 1 KiB per chunk
        // and wave.  Chunk 0 here, chunk c + 1 in stage 3 of chunk c in FRONT of that stage's U pieces: the counted waits below
        // (wait_vmcnt<LPM> = "all but my last LPM operations") then cover these loads too -- they are older than the pieces the count
        // leaves in flight -- so the existing counts hold unchanged, and the registers are complete one stage before their first use.
        const float* w1p = nullptr;
        auto load_w1 = [&](int chunk) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(w1[q]) : "v"(w1p + ((long long)chunk * (p.N >> 5) * 4 + q) * 256) : "memory");
        };
        auto pin_w1 = [&] {
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(w1[q]));
        };
        if constexpr (SK) {
            w1p = p.sk_w + ((long long)((n0 >> 5) + nb) * 4 * 64 + lane) * 4;
            load_w1(c_begin);
        }
        if (G::LPM > 0 && !(DBG & 4)) {
            issue_u(0, 0, 4 * G::LPL + wid * G::LPM, std::integral_constant<int, G::LPM>{});
            issue_u(1, 1, 4 * G::LPL + wid * G::LPM, std::integral_constant<int, G::LPM>{});
            wait_vmcnt<G::LPM>();                                           // U(0); its pieces of U(1) land before B(1)
        }
        if constexpr (SK) { if (G::LPM == 0) wait_vmcnt<0>(); pin_w1(); }
        __builtin_amdgcn_s_barrier();                                       // B0: stages 0, 1 complete
        unsigned long long r_loop0 = 0, c_wait = 0, c_mma = 0;
        if (DBG) r_loop0 = __builtin_amdgcn_s_memrealtime();
        // One stage = 16 MFMAs on acc[s] in 4 quarters of 4 (one ds_read_b128 of A and of B each).  Fragments are double-buffered:
        // while a quarter multiplies, the next quarter's are read.
        //   waves 0..3 (STG = false) run the quarters of stage S between B(S) and B(S+1); U(S) is only guaranteed by B(S), so their
        //     first B fragment is read behind the barrier -- an LDS round trip with nothing of their own to multiply;
        //   waves 4..7 (STG = true), their SIMD partners, are staggered by ONE quarter: they keep the fragments of (S-1, q3) in
        //     registers across B(S), multiply them right behind it -- while the (S, q0) fragments are in flight -- and end the interval
        //     with (S, q2).  The two waves of a SIMD so never reach their LDS bursts, their exposed waits and the barrier in lockstep,
        //     and the pipe has the deferred quarter to run while waves 0..3 wait for their first fragments (profiles/r04_wino_clock.txt:
        //     unstaggered, waves 0..3 arrived at the barrier 700 cycles before their partners, with the pipe 26 % idle before that).
        auto mloop = [&](auto stgc, auto skc) {
            constexpr bool STG = decltype(stgc)::value, SKW = decltype(skc)::value;
            float4 a[2], b[2];
            int buf = 0, S = 0;
            auto frag = [&](float4& av, float4& bv, const float* As, const float* Bs, int q) {
                av = *reinterpret_cast<const float4*>(As + foff[q]);
                bv = *reinterpret_cast<const float4*>(Bs + foff[q]);
            };
            auto mma4 = [&](f32x16& c, const float4& av, const float4& bv) {
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, c, 0, 0, 0);
            };
            if (STG) frag(a[1], b[1], smem + a_img, smem + b_img, 0);                  // (0, q0): the one exposed read of these waves
            else a[0] = *reinterpret_cast<const float4*>(smem + a_img + foff[0]);
            for (int c = 0; c < n_chunks; ++c) {
                static_for<SPC>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    // SKW: quarter q of stage st in {1, 2} also goes into sk[st - 1], against W1 fragment q
                    auto skq = [&](auto stc, auto qc, const float4& av) {
                        constexpr int st = decltype(stc)::value, q = decltype(qc)::value;
                        if constexpr (SKW && (st == 1 || st == 2))
                            mma4(sk[st - 1], av, make_float4(w1[q].x, w1[q].y, w1[q].z, w1[q].w));
                    };
                    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
                    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
                    using IS = std::integral_constant<int, s>; using IP = std::integral_constant<int, (s + SPC - 1) % SPC>;
                    auto next_w1 = [&] {        // next chunk's fragments (the last chunk reloads its own: no branch joins the registers)
                        if constexpr (SKW && s == SPC - 1) {
                            __builtin_amdgcn_sched_barrier(0);
                            load_w1(c_begin + (c + 1 < n_chunks ? c + 1 : c));
                        }
                    };
                    const float* As = smem + buf * STAGE + a_img;
                    const float* Bs = smem + buf * STAGE + b_img;
                    const int nbuf = buf == 2 ? 0 : buf + 1, pbuf = buf == 0 ? 2 : buf - 1;
                    const bool more = S + 2 < n_stages;                          // wave-uniform
                    auto dma = [&] {                                             // its U pieces of stage S + 2, behind a quarter's first MFMAs
                        if (more && G::LPM > 0 && !(DBG & 4)) {
                            __builtin_amdgcn_sched_barrier(0);
                            issue_u(S + 2, pbuf, 4 * G::LPL + wid * G::LPM, std::integral_constant<int, G::LPM>{});
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    };
                    if constexpr (!STG) {
                        b[0] = *reinterpret_cast<const float4*>(Bs + foff[0]);
                        frag(a[1], b[1], As, Bs, 1);
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[0], b[0]);
                        skq(IS{}, I0{}, a[0]);
                        frag(a[0], b[0], As, Bs, 2);
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[1], b[1]);
                        skq(IS{}, I1{}, a[1]);
                        next_w1();
                        dma();
                        frag(a[1], b[1], As, Bs, 3);
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[0], b[0]);
                        skq(IS{}, I2{}, a[0]);
                        a[0] = *reinterpret_cast<const float4*>(smem + nbuf * STAGE + a_img + foff[0]);     // V of stage S+1: complete since B(S)
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[1], b[1]);
                        skq(IS{}, I3{}, a[1]);
                    } else {
                        if (s > 0 || c > 0) {                                    // the deferred quarter (S-1, q3); [1] <- (S, q0)
                            frag(a[1], b[1], As, Bs, 0);
                            __builtin_amdgcn_sched_barrier(0);
                            mma4(acc[(s + SPC - 1) % SPC], a[0], b[0]);
                            skq(IP{}, I3{}, a[0]);
                        }
                        frag(a[0], b[0], As, Bs, 1);
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[1], b[1]);
                        skq(IS{}, I0{}, a[1]);
                        next_w1();                                               // (behind the deferred quarter, the last reader of w1[3])
                        dma();
                        frag(a[1], b[1], As, Bs, 2);
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[0], b[0]);
                        skq(IS{}, I1{}, a[0]);
                        frag(a[0], b[0], As, Bs, 3);                             // kept across the barrier
                        __builtin_amdgcn_sched_barrier(0);
                        mma4(acc[s], a[1], b[1]);
                        skq(IS{}, I2{}, a[1]);
                    }
                    if (more && !(DBG & 4)) wait_vmcnt<G::LPM>(); else wait_vmcnt<0>();       // my pieces of U(S+1), issued during stage S-1, have landed
                    if constexpr (SKW && s == SPC - 1) pin_w1();                // ... and the W1 fragments requested in front of this stage's pieces
                    unsigned long long tA = 0, tB = 0;
                    if (DBG) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tA)::"memory"); }
                    __builtin_amdgcn_s_barrier();                               // B(S+1): stage S released; V <= S+2, U <= S+1 complete
                    if (DBG) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tB)::"memory"); c_wait += tB - tA; if (c_mma == 0) c_mma = tA; }
                    if ((DBG & 16) && blockIdx.x + blockIdx.y + blockIdx.z == 0 && S >= 8 && S < 16 && lane == 0) {
                        g_wino_timeline[(wid * 8 + (S - 8)) * 2] = tA;
                        g_wino_timeline[(wid * 8 + (S - 8)) * 2 + 1] = tB;
                    }
                    buf = nbuf;
                    ++S;
                });
            }
            if (STG) mma4(acc[SPC - 1], a[0], b[0]);                             // the last stage's deferred quarter
        };
        if constexpr (SK) {
            if (skw) { if (W2_STAGGER && wid >= 4) mloop(std::true_type{}, std::true_type{}); else mloop(std::false_type{}, std::true_type{}); }
            else { if (W2_STAGGER && wid >= 4) mloop(std::true_type{}, std::false_type{}); else mloop(std::false_type{}, std::false_type{}); }
        } else {
            if (W2_STAGGER && wid >= 4) mloop(std::true_type{}, std::false_type{}); else mloop(std::false_type{}, std::false_type{});
        }
        if (DBG && lane == 0 && wid == 0) {
            const int wg = (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) & 1023;
            unsigned long long tE;
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tE)::"memory");
            g_wino_stamps[wg * 8 + 0] = r_entry;
            g_wino_stamps[wg * 8 + 1] = r_loop0;
            g_wino_stamps[wg * 8 + 2] = __builtin_amdgcn_s_memrealtime();
            g_wino_stamps[wg * 8 + 3] = c_wait;                 // shader cycles parked at the stage barriers
            g_wino_stamps[wg * 8 + 4] = tE - c_mma;             // shader cycles from the end of stage 0's multiply to the end of the loop
            g_wino_stamps[wg * 8 + 5] = (unsigned long long)n_stages;
        }
    }
    // ---- output transform.  Rows first, in registers: T[a] = sum_i A^T[a][i] M[4i + j],  A^T = [[1,1,1,0],[0,1,-1,-1]].
    //      D: the wave holds column j = pp (acc[i]); its two T blocks go to column block j.  F: the wave holds columns j = pp and
    //      pp + 2 (acc[2i + h], j = 2h + pp) and also folds what it can of the column transform Y[a][0] = T0 + T1 + T2,
    //      Y[a][1] = T1 - T2 - T3:  pp = 0 contributes {T0 + T2, -T2}, pp = 1 contributes {T1, T1 - T3}; block (pp, b).
    {
        constexpr int TP = G::TP;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int col = nb * 32 + (lane & 31);
            if constexpr (P == 4) {
                float* Ts = smem + pp * (2 * WBT * TP);
                const float m0 = acc[0][r], m1 = acc[1][r], m2 = acc[2][r], m3 = acc[3][r];
                Ts[row * TP + col] = (m0 + m1) + m2;
                Ts[(WBT + row) * TP + col] = (m1 - m2) - m3;
                if constexpr (SK) {
                    // rows of the Hadamard transform back: pp = 1 holds S5, S9, pp = 2 holds S6, S10; output row a = 0: S(4 + pp) - S(8 + pp),
                    // a = 1: their sum.  Two blocks behind the conv's staging area and its GroupNorm scratch.
                    if (skw) {
                        float* Ks = smem + G::T_FL + 320 + (pp - 1) * (2 * WBT * TP);
                        Ks[row * TP + col] = sk[0][r] - sk[1][r];
                        Ks[(WBT + row) * TP + col] = sk[0][r] + sk[1][r];
                    }
                }
            } else {
                const float l0 = acc[0][r], l1 = acc[2][r], l2 = acc[4][r], l3 = acc[6][r];      // column pp     (h = 0)
                const float h0 = acc[1][r], h1 = acc[3][r], h2 = acc[5][r], h3 = acc[7][r];      // column pp + 2 (h = 1)
                const float tl0 = (l0 + l1) + l2, tl1 = (l1 - l2) - l3;                          // T[a = 0], T[a = 1] of column pp
                const float th0 = (h0 + h1) + h2, th1 = (h1 - h2) - h3;                          // ... of column pp + 2
                float* B0 = smem + (pp * 2 + 0) * (2 * WBT * TP);                                // contribution to Y[a][0]
                float* B1 = smem + (pp * 2 + 1) * (2 * WBT * TP);                                // ... to Y[a][1]
                if (pp == 0) {
                    B0[row * TP + col] = tl0 + th0;          B0[(WBT + row) * TP + col] = tl1 + th1;
                    B1[row * TP + col] = -th0;               B1[(WBT + row) * TP + col] = -th1;
                } else {
                    B0[row * TP + col] = tl0;                B0[(WBT + row) * TP + col] = tl1;
                    B1[row * TP + col] = tl0 - th0;          B1[(WBT + row) * TP + col] = tl1 - th1;
                }
            }
        }
    }
    __syncthreads();   // the 8 matrix waves (the loaders have exited): every block is in LDS

    // ---- finish: 512 threads, item = (tile, output row a, channel quad) -> the two pixels (2ty + a, 2tx), (2ty + a, 2tx + 1)
    constexpr int TP = G::TP, QUADS = G::QUADS, ITEMS = G::ITEMS;
    // CL with a channel-chunk split: workgroup `split == 0` of a tile finishes it -- its partners hand their partial tiles over through
    // p.cl_slab (sc1 stores, drained, one arrival on the tile's pair counter) and leave; everything is one dispatch round (host)
    // (only the 64-channel tile has such shapes: the host admits the split form on variant D alone)
    constexpr bool CLS = CL && P == 4;
    const bool partner = CLS && split > 0;
    const bool direct = p.splits == 1 || (CLS && !partner);
    float* outp = p.splits == 1 ? p.out : CLS ? p.cl_slab + (long long)(split - 1) * p.slab_stride : p.out + (long long)split * p.slab_stride;
    float4 keep[ITEMS][2];
    float4 sz[ITEMS][2];                   // SK: the skip tile (only the hand-off's finishing workgroup reads it again)
    long long oo[ITEMS];
    int opix[ITEMS];                       // pixel index of an item's first output (the second is the next pixel of the row)
    const int cq = tid & (QUADS - 1);
    const int gn = n0 + cq * 4;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = tid + it * 512;
        const int t = item / (2 * QUADS), a = (item / QUADS) & 1;
        const int g = t0 + t;
        keep[it][0] = keep[it][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        oo[it] = -1;
        opix[it] = 0;
        if (g >= p.tiles || gn >= p.N) continue;
        const float* tp = smem + (a * WBT + t) * TP + cq * 4;
        const float4 q0 = *reinterpret_cast<const float4*>(tp);
        const float4 q1 = *reinterpret_cast<const float4*>(tp + 1 * (2 * WBT * TP));
        const float4 q2 = *reinterpret_cast<const float4*>(tp + 2 * (2 * WBT * TP));
        const float4 q3 = *reinterpret_cast<const float4*>(tp + 3 * (2 * WBT * TP));
        float4 y0, y1;
        if constexpr (P == 4) {
            y0 = f4add(f4add(q0, q1), q2);
            y1 = f4sub(f4sub(q1, q2), q3);
        } else {
            y0 = f4add(q0, q2);           // blocks (0,0) + (1,0)
            y1 = f4add(q1, q3);           // blocks (0,1) + (1,1)
        }
        const unsigned tmp = fdiv_u((unsigned)g, p.dTW);
        const int tx = g - (int)tmp * p.TW;
        const unsigned bq = fdiv_u(tmp, p.dTH);
        const int ty = (int)tmp - (int)bq * p.TH;
        const long long o0 = ((((long long)bq * p.H + 2 * ty + a) * p.W) + 2 * tx) * p.N + gn;
        oo[it] = o0;
        opix[it] = ((int)bq * p.H + 2 * ty + a) * p.W + 2 * tx;
        if constexpr (SK) {
            // the skip conv's two pixels of this item: columns of the Hadamard transform back, y(a, 0) = R1 - R2, y(a, 1) = R1 + R2
            const float* kp = smem + G::T_FL + 320 + (a * WBT + t) * TP + cq * 4;
            const float4 k1 = *reinterpret_cast<const float4*>(kp);
            const float4 k2 = *reinterpret_cast<const float4*>(kp + 2 * WBT * TP);
            float4 z0 = f4sub(k1, k2), z1 = f4add(k1, k2);
            if (direct && p.sk_bias) {
                const float4 bb = *reinterpret_cast<const float4*>(p.sk_bias + gn);
                z0 = f4add(z0, bb);
                z1 = f4add(z1, bb);
            }
            // like the conv tile: the result, a slab of partial sums (host: sk_out is then the skip slab area), or -- partner hand-off --
            // a partial tile behind the conv partials of cl_slab, summed by the tile's first workgroup below
            if (!CLS || p.splits == 1) {
                float* so = p.splits == 1 ? p.sk_out : p.sk_out + (long long)split * p.sk_stride;
                *reinterpret_cast<float4*>(so + o0) = z0;
                *reinterpret_cast<float4*>(so + o0 + p.N) = z1;
            } else if (partner) {
                float* so = p.cl_slab + (long long)(p.splits - 1 + split - 1) * p.slab_stride;
                st_sc1_f4(so + o0, z0);
                st_sc1_f4(so + o0 + p.N, z1);
            }
            sz[it][0] = z0;
            sz[it][1] = z1;
        }
        if (direct) {
            if (p.bias) {
                const float4 bb = *reinterpret_cast<const float4*>(p.bias + gn);
                y0 = f4add(y0, bb);
                y1 = f4add(y1, bb);
            }
            if (!CL && p.resid) {
                y0 = f4add(y0, *reinterpret_cast<const float4*>(p.resid + o0));
                y1 = f4add(y1, *reinterpret_cast<const float4*>(p.resid + o0 + p.N));
            }
            if (p.post_mish) {
                y0 = make_float4(mish_f(y0.x), mish_f(y0.y), mish_f(y0.z), mish_f(y0.w));
                y1 = make_float4(mish_f(y1.x), mish_f(y1.y), mish_f(y1.z), mish_f(y1.w));
            }
        }
        if (!CL) {
            *reinterpret_cast<float4*>(outp + o0) = y0;
            *reinterpret_cast<float4*>(outp + o0 + p.N) = y1;
        } else if (CLS && partner) {
            st_sc1_f4(outp + o0, y0);
            st_sc1_f4(outp + o0 + p.N, y1);
        }
        keep[it][0] = y0;
        keep[it][1] = y1;
    }
    if (CLS && p.splits > 1) {
        unsigned* pair = p.cl_pair + ((long long)tile_m * gridDim.y + tile_n) * 16;
        if (partner) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // every wave's sc1 stores have left before the one arrival
            __syncthreads();
            if (tid == 0) __hip_atomic_fetch_add(pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        int* pair_gave_up = reinterpret_cast<int*>(smem + G::T_FL + 258);
        if (tid == 0) {
            *pair_gave_up = 0;
            const unsigned want = (unsigned)p.splits - 1u;
            if (cl_wait_ge<2>(pair, want, p.cl_fail)) *pair_gave_up = 1;
            __hip_atomic_store(pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // its only reader: re-armed for the next launch
        }
        __syncthreads();                 // (also: every thread is done with the staging area the partial tiles came from)
        const bool pair_poisoned = *pair_gave_up != 0;
        for (int s = 1; s < p.splits; ++s) {
            const float* sl = p.cl_slab + (long long)(s - 1) * p.slab_stride;
            static_assert(ITEMS % 2 == 0, "two items per load group");
#pragma unroll
            for (int it = 0; it < ITEMS; it += 2) {        // (host: every tile of a CL shape is full, so every oo[] is a real offset)
                float4 a0, a1, b0, b1;
                ld_sc1_f4x4(a0, a1, b0, b1, sl + oo[it], sl + oo[it] + p.N, sl + oo[it + 1], sl + oo[it + 1] + p.N);
                keep[it][0] = f4add(keep[it][0], a0);
                keep[it][1] = f4add(keep[it][1], a1);
                keep[it + 1][0] = f4add(keep[it + 1][0], b0);
                keep[it + 1][1] = f4add(keep[it + 1][1], b1);
            }
        }
        if (pair_poisoned) {
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) keep[it][0].x = __builtin_nanf("");
        }
        if constexpr (SK) {
            // the partners' skip partials, in split order like the conv's; a give-up poisons this tile too
            for (int s = 1; s < p.splits; ++s) {
                const float* sl = p.cl_slab + (long long)(p.splits - 1 + s - 1) * p.slab_stride;
#pragma unroll
                for (int it = 0; it < ITEMS; it += 2) {
                    float4 a0, a1, b0, b1;
                    ld_sc1_f4x4(a0, a1, b0, b1, sl + oo[it], sl + oo[it] + p.N, sl + oo[it + 1], sl + oo[it + 1] + p.N);
                    sz[it][0] = f4add(sz[it][0], a0);
                    sz[it][1] = f4add(sz[it][1], a1);
                    sz[it + 1][0] = f4add(sz[it + 1][0], b0);
                    sz[it + 1][1] = f4add(sz[it + 1][1], b1);
                }
            }
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                if (pair_poisoned) sz[it][0].x = __builtin_nanf("");
                *reinterpret_cast<float4*>(p.sk_out + oo[it]) = sz[it][0];
                *reinterpret_cast<float4*>(p.sk_out + oo[it] + p.N) = sz[it][1];
            }
        }
    }
    // ---- optional GroupNorm statistics of this tile (host: every m tile full and inside one image): per group {mean, M2 about that
    //      mean} over the tile's 128 pixels x cpg channels, two passes over the registers
    if (CL || p.gn_part) {
        const int qpg = p.cpg >> 2;                    // quads per group
        const int gl = cq / qpg;                       // group within the tile's channels (< 8)
        float* red = smem + G::T_FL;                   // behind the staging area; one 128-float region per pass
        auto group_sum = [&](float v, float* rd) {
            for (int o = 1; o < qpg; o <<= 1) v += __shfl_xor(v, o, 64);
#pragma unroll
            for (int o = QUADS; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            if (lane < QUADS && (cq & (qpg - 1)) == 0) rd[wid * 16 + gl] = v;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS traffic only: not the output stores above
            float t = rd[gl];
#pragma unroll
            for (int w = 1; w < 8; ++w) t += rd[w * 16 + gl];
            return t;
        };
        auto sum4 = [](float4 v) { return (v.x + v.y) + (v.z + v.w); };
        const float inv = 1.0f / (float)(4 * WBT * p.cpg);
        float s1 = 0.f;
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) s1 += sum4(keep[it][0]) + sum4(keep[it][1]);
        const float mean = group_sum(s1, red) * inv;
        auto sq4 = [&](float4 v) {
            const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
            return (a * a + b * b) + (c * c + d * d);
        };
        float s2 = 0.f;
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) s2 += sq4(keep[it][0]) + sq4(keep[it][1]);
        const float m2 = group_sum(s2, red + 128);
        if (!CL) {
            if (tid < QUADS && (cq & (qpg - 1)) == 0) p.gn_part[(long long)tile_m * p.groups + n0 / p.cpg + gl] = make_float2(mean, m2);
        } else {
            // ---- cluster exchange (cluster_sync.h), as in the kernel above (one workgroup per CU: >= 120 KB of LDS)
            const int image = tile_m / p.cl_np;
            unsigned long long* rec = reinterpret_cast<unsigned long long*>(p.cl_rec) + ((long long)tile_m * gridDim.y + tile_n) * 16;
            unsigned* cnt = p.cl_cnt + ((long long)image * gridDim.y + tile_n) * 16;
            int* gave_up = reinterpret_cast<int*>(red + 256);
            if (tid == 0) *gave_up = 0;
            if (tid < QUADS && (cq & (qpg - 1)) == 0) cl_store_stats(rec + gl, mean, m2);
            float4 ga, be, ts = make_float4(0.f, 0.f, 0.f, 0.f);
            auto load_affine = [&] {
                ga = *reinterpret_cast<const float4*>(p.gn_gamma + gn);
                be = *reinterpret_cast<const float4*>(p.gn_beta + gn);
                if (p.gn_temb) {
                    const int b_img = (int)((long long)t0 / ((long long)p.TH * p.TW));
                    const long long tr = p.gn_temb_rows ? p.gn_temb_rows[b_img] : b_img;
                    ts = *reinterpret_cast<const float4*>(p.gn_temb + tr * p.gn_temb_stride + gn);
                }
            };
            float4 rs[ITEMS][2];
            auto load_resid = [&] {
#pragma unroll
                for (int it = 0; it < ITEMS; ++it) {
                    rs[it][0] = rs[it][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p.resid) {
                        rs[it][0] = *reinterpret_cast<const float4*>(p.resid + oo[it]);
                        rs[it][1] = *reinterpret_cast<const float4*>(p.resid + oo[it] + p.N);
                    }
                }
                if (p.r1_x) {
                    // the addend is a 1x1 conv of a narrow tensor (the first ResnetBlock's res_conv of the <= 8-channel input): this lane's
                    // four weight rows, then <= 8 MACs per output -- instead of a GroupNorm-apply launch that computes it (15 us at cfg4)
                    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p.r1_b) bb = *reinterpret_cast<const float4*>(p.r1_b + gn);
#pragma unroll
                    for (int it = 0; it < ITEMS; ++it) rs[it][0] = rs[it][1] = bb;
                    if (p.r1_cin == 8 && (p.r1_ld & 3) == 0) {
                        // 8 input channels: this lane's four weight rows as 8 float4, a pixel's 8 inputs as 2 float4 (24 vector loads
                        // per lane; as scalar loads -- 96, every one strided over the lanes -- the epilogue took 13 us longer)
                        float4 wv[4][2];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            wv[j][0] = *reinterpret_cast<const float4*>(p.r1_w + (long long)(gn + j) * p.r1_ld);
                            wv[j][1] = *reinterpret_cast<const float4*>(p.r1_w + (long long)(gn + j) * p.r1_ld + 4);
                        }
                        auto dot8 = [](float4 a0, float4 a1, float4 b0, float4 b1) {
                            return ((a0.x * b0.x + a0.y * b0.y) + (a0.z * b0.z + a0.w * b0.w)) + ((a1.x * b1.x + a1.y * b1.y) + (a1.z * b1.z + a1.w * b1.w));
                        };
#pragma unroll
                        for (int it = 0; it < ITEMS; ++it) {
                            if (oo[it] < 0) continue;
                            const float* xp = p.r1_x + (long long)opix[it] * 8;   // the item's two pixels (y, x), (y, x + 1): 16 contiguous floats
                            const float4 xa0 = *reinterpret_cast<const float4*>(xp), xa1 = *reinterpret_cast<const float4*>(xp + 4);
                            const float4 xb0 = *reinterpret_cast<const float4*>(xp + 8), xb1 = *reinterpret_cast<const float4*>(xp + 12);
                            rs[it][0].x += dot8(xa0, xa1, wv[0][0], wv[0][1]); rs[it][0].y += dot8(xa0, xa1, wv[1][0], wv[1][1]);
                            rs[it][0].z += dot8(xa0, xa1, wv[2][0], wv[2][1]); rs[it][0].w += dot8(xa0, xa1, wv[3][0], wv[3][1]);
                            rs[it][1].x += dot8(xb0, xb1, wv[0][0], wv[0][1]); rs[it][1].y += dot8(xb0, xb1, wv[1][0], wv[1][1]);
                            rs[it][1].z += dot8(xb0, xb1, wv[2][0], wv[2][1]); rs[it][1].w += dot8(xb0, xb1, wv[3][0], wv[3][1]);
                        }
                    } else {
                        for (int k = 0; k < p.r1_cin; ++k) {
                            const float w0 = p.r1_w[(long long)(gn + 0) * p.r1_ld + k], w1 = p.r1_w[(long long)(gn + 1) * p.r1_ld + k];
                            const float w2 = p.r1_w[(long long)(gn + 2) * p.r1_ld + k], w3 = p.r1_w[(long long)(gn + 3) * p.r1_ld + k];
#pragma unroll
                            for (int it = 0; it < ITEMS; ++it) {
                                if (oo[it] < 0) continue;
                                const long long pix = opix[it];                  // the item's two pixels: (y, x) and (y, x + 1)
                                const float x0 = p.r1_x[pix * p.r1_cin + k], x1 = p.r1_x[(pix + 1) * p.r1_cin + k];
                                rs[it][0].x += x0 * w0; rs[it][0].y += x0 * w1; rs[it][0].z += x0 * w2; rs[it][0].w += x0 * w3;
                                rs[it][1].x += x1 * w0; rs[it][1].y += x1 * w1; rs[it][1].z += x1 * w2; rs[it][1].w += x1 * w3;
                            }
                        }
                    }
                }
            };
            if (wid != 0) { load_affine(); load_resid(); }
            if (wid == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                load_affine();
                load_resid();
                if (lane == 0 && cl_wait_ge<4>(cnt, (unsigned)p.cl_np, p.cl_fail)) *gave_up = 1;
            }
            __syncthreads();
            const unsigned long long* r0 = reinterpret_cast<const unsigned long long*>(p.cl_rec) +
                                           ((long long)image * p.cl_np * gridDim.y + tile_n) * 16 + gl;
            const bool poisoned = *gave_up != 0;
            float rm[8], rq[8];
            cl_load_stats(r0, (long long)gridDim.y * 16, p.cl_np, rm, rq);
            if (tid == 0) cl_depart(cnt, cnt + 1, (unsigned)p.cl_np);
            const float2 st = cl_merge_stats(rm, rq, p.cl_np, 128.0f * (float)p.cpg, p.gn_eps, poisoned);
            const float gmean = st.x, rstd = st.y;
            auto fin = [&](float4 v) {
                return make_float4(mish_f((v.x - gmean) * rstd * ga.x + be.x) + ts.x, mish_f((v.y - gmean) * rstd * ga.y + be.y) + ts.y,
                                   mish_f((v.z - gmean) * rstd * ga.z + be.z) + ts.z, mish_f((v.w - gmean) * rstd * ga.w + be.w) + ts.w);
            };
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                *reinterpret_cast<float4*>(p.out + oo[it]) = f4add(fin(keep[it][0]), rs[it][0]);
                *reinterpret_cast<float4*>(p.out + oo[it] + p.N) = f4add(fin(keep[it][1]), rs[it][1]);
            }
        }
    }
    if (DBG && tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int wg = (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) & 1023;
        g_wino_stamps[wg * 8 + 6] = __builtin_amdgcn_s_memrealtime();
        g_wino_stamps[wg * 8 + 7] = 1;
    }
}
