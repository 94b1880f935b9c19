// unet_plan.hip -- native sequencing of the eval-mode UNet forward and of the T-step sampler loop.
//
// Reference: models/unet/unet.py:10-72 (module tree), :74-104 (forward), models/unet/blocks.py:105-115
// (ResnetBlock), :8-14,63-71,126-134 (Residual(PreNorm(LinearAttention))), models/diffusion/ddpm.py:203-249
// (p_sample, p_sample_loop).
//
// The plan owns (a) the list of weight slots -- one per state_dict tensor, with the packed layout each
// kernel wants -- and (b) the order of kernel launches for one forward.  Nothing here computes: every
// arithmetic step is a HIP kernel from the other translation units.  The sampler captures one reverse step
// (t bookkeeping + UNet + x update) into a hipGraph and replays it, so the T-step loop costs one
// hipGraphLaunch per step on the host.
#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "ddk_internal.h"
#include "level_chain.h"

namespace ddk {

constexpr int HEADS = 4;
constexpr int HIDDEN = HEADS * 32;  // LinearAttention hidden width is 128 whatever unet_chan is (blocks.py:119-122)
constexpr int GROUPS = 8;
constexpr float GN_EPS = 1e-5f, LN_EPS = 1e-5f;

static inline int pad32(int c) { return (c + 31) / 32 * 32; }

enum PackKind { PK_COPY = 0, PK_CONV = 1, PK_CONVT = 2, PK_LINEAR_T = 3, PK_WINO = 4, PK_LOCAL = 5, PK_WLOCAL = 6, PK_FIRST = 7, PK_CONVT_WINO = 8,
                PK_ROWS = 9 /* [O][I] rows into rows of pitch ld */, PK_LOCAL1 = 10 /* a 1x1 filter in conv_local.hip's operand order */,
                PK_CONVT_LOCAL = 11 /* a transpose-conv filter in the level chain's operand order */,
                PK_SKIP_WINO = 12 /* a res_conv's 1x1 filter as the skip-fold operand of the Winograd kernel */ };

struct Slot {
    std::string name;
    long long numel;
    int kind;
    size_t off;  // float offset into the packed arena
    int O, I, KH, KW, i_pad, ld, col0;
    int split = 0, split_pad = 0;   // PK_CONV over two separately padded sources (generic widths): see ddk_pack_conv_weight_split
    int attn = -1;  // >= 0: the slot feeds the folded LayerNorm of that attention site (packing it re-derives W o g, W g, W b)
};

struct ConvW {
    size_t w = 0, b = 0;
    bool has_bias = false;
    int cin = 0, cin_pad = 0, cout = 0;
    size_t wu = 0;          // Winograd-domain copy of a 3x3 filter ([cin_pad/32][16][cout][32]); has_wu says whether it exists
    bool has_wu = false;
    size_t wl = 0;          // conv_local.hip's operand-order copy (3x3 convs that feed a GroupNorm); has_wl says whether it exists
    bool has_wl = false;
    size_t wwl = 0;         // and its Winograd-domain form for the 8x8 maps (conv3x3_gn_wlocal_kernel); has_wwl
    bool has_wwl = false;
    size_t wf = 0;          // conv_first.hip's operand-order copy (the network's first conv, C_in <= 8); has_wf
    bool has_wf = false;
    size_t wl1 = 0;         // a 1x1 filter (to_out, res_conv) in conv_local.hip's operand order, one tap: the level chain's 1x1 ops
    bool has_wl1 = false;
    size_t wtl = 0;         // a transpose-conv filter in the level chain's operand order (CH_UPT); has_wtl
    bool has_wtl = false;
    size_t wsk = 0;         // a res_conv's 1x1 filter / 4 in the Winograd kernel's operand order (the skip fold, DDK_OPT_SKIP_FOLD); has_wsk
    bool has_wsk = false;
};
struct NormW { size_t g = 0, b = 0; int c_real = 0; };
struct ResW {
    // ci / co: channel counts as the kernels see them (co is padded to 32 at generic widths); *_real: the reference's
    int ci = 0, ci_pad = 0, co = 0, temb_off = 0, ci_real = 0, co_real = 0;
    ConvW c1, c2, res;
    NormW n1, n2;
    bool has_res = false;
};
struct AttnW {
    int c = 0, c_real = 0;
    NormW ln;
    ConvW qkv, out;
    // LayerNorm folded into to_qkv (derived at pack time by ddk_unet_finalize_pack): W o g, W g, W b
    size_t qkv_lnw = 0, ln_c1 = 0, ln_c2 = 0;
    size_t qkv_op = 0;      // qkv_lnw in the operand order of linattn_small_qkv_kernel (derived with it)
};

}  // namespace ddk

using namespace ddk;

// One captured step of a chain: a reverse step of the sampler, or a step of the likelihood sweep.  A hipGraph bakes in every
// pointer its kernels were launched with, so an entry is valid for exactly this kind of chain, this set of buffers and this
// shape; t, the Philox seed / stream id and the injected-noise step index are read from device memory by the kernels, so the
// same graph serves every step of every chain on those buffers.
struct ChainKey {
    StepKind kind;                           // how the chain's steps end: one kind per chain entry
    const void* bufs[14];                    // every buffer the step's kernels are launched with (unused entries null)
    const void* ws;
    const void* noise;                       // also in bufs; injected draws: no 16-step graph (see run_chain)
    int B, H, W, t_start, device;
    unsigned long long pack_epoch;
    int restore_n = 0;                       // the plane-wide kinds: Stage's key_n (every operand is staged in the workspace).
                                             // StepKind::Restore, RestoreMasked: the block (y and the mask are staged in the workspace; the kind
                                             // says whether a mask is present, so a masked and an unmasked chain never share a graph)
    bool restore_mask = false;               // StepKind::RestoreMultistep, RestoreNoisy, one kind with or without a mask: whether its kernels were given one
    int restore_gray = 0;                    // StepKind::RestoreGray: the weights (rst.gray), so "mean" and "luma" chains never share a graph
    bool operator==(const ChainKey& o) const {
        for (int i = 0; i < 14; ++i)
            if (bufs[i] != o.bufs[i]) return false;
        return kind == o.kind && ws == o.ws && noise == o.noise && B == o.B && H == o.H && W == o.W && t_start == o.t_start &&
               device == o.device && pack_epoch == o.pack_epoch && restore_n == o.restore_n && restore_mask == o.restore_mask && restore_gray == o.restore_gray;
    }
};
struct SamplerGraph {
    ChainKey key;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph_multi = nullptr;        // SAMPLER_MULTI consecutive steps in one graph (captured when a chain is long enough)
    hipGraphExec_t exec_multi = nullptr;
    hipEvent_t done = nullptr;               // recorded behind the entry's latest launches: what an eviction has to wait for
    unsigned long long last_use = 0;
};
constexpr int SAMPLER_MULTI = 16;

struct ddk_unet {
    // sampler state cached across ddk_sampler_run calls (guarded by `mu`; see ddk_sampler_invalidate)
    std::mutex mu;
    std::vector<SamplerGraph> graphs;
    unsigned long long use_clock = 0;
    unsigned long long pack_epoch = 0;       // bumped by every pack / finalize: weights changed
    struct {
        const void* ws = nullptr;
        int t_start = -1, B = 0, H = 0, W = 0;
        unsigned long long pack_epoch = 0;
        std::vector<int64_t> map;            // timestep of each row (ddk_sampler_run_spaced); empty: row k is timestep k
    } table;
    ddk_unet_config cfg;
    int cluster_gn = 1;                      // GroupNorm finished inside the Winograd conv launch where eligible (ddk_unet_set_option):
                                             // 0 never, 1 in ddk_sampler_run (whose caller checks ddk_unet_cluster_check at the chain's
                                             // sync point), 2 in ddk_unet_forward too
    int cluster_limit = 1 << 30;             // diagnostic: only the first so many eligible launches of a forward take that path
    int cluster_np_max = 8;                  // largest cluster (workgroups per image and n tile) that takes the path
    bool cluster_split = true;               // ... also on shapes whose channel chunks are split over 2-4 workgroups (conv_wino_cluster_split_np):
                                             // a tile's first workgroup sums its partners' partial tiles in the launch (diagnostic option 11)
    bool attn_kvctx = true;                  // folded attention block: k, v projection + context in one launch (no kv tensor)
    bool attn_fold_parts = true;             // ... and the per-image matrix folded straight from that launch's split records: no merge launch, no
                                             // ctx tensor (DDK_OPT_ATTENTION_FOLD_PARTIALS; attn_fold_parts_ok)
    bool attn_split = true;                  // 16x16 / 8x8 maps: to_qkv + core in one launch, an (image, head) split over two workgroups that
                                             // exchange their context partials in the launch (DDK_OPT_ATTENTION_SPLIT) -- wherever the
                                             // in-launch GroupNorm may run; 0: the projection and linattn_small_kernel as two launches
    bool skip_fold = true;                   // a ResnetBlock's res_conv computed inside its first 3x3 conv's Winograd launch where that conv runs
                                             // on the 64-channel tile (DDK_OPT_SKIP_FOLD; conv_wino_skip_ok)
    bool fold_down_reduce = false;           // Downsample conv's split-K slabs summed by the image-local ResnetBlock behind it (no reduce launch).
                                             // OFF by default: measured 6 us per step SLOWER (each of an image's eight workgroups re-sums the slabs:
                                             // +6.3 / +5.9 us on the two consumers against reduce launches of 5.2 / 4.9 us; tools/fold_ab.py)
    bool restore_fused = true;               // the Restore kind's fused tail where eligible (DDK_OPT_RESTORE_FUSED_TAIL; 0: always the unfused tail)
    bool first_gn = true;                    // the first Block's GroupNorm + Mish + shift inside conv_first_kernel's launch (DDK_OPT_FIRST_GROUPNORM),
                                             // wherever the in-launch GroupNorm of the Winograd convs may run
    int level_chain = 9;                     // bit 0: the whole 4x4 level (ResnetBlocks + attention of downs[-1], mid, ups[0]) as ONE persistent launch
                                             // (level_chain.hip) wherever the in-launch GroupNorm may run (its workgroups wait for each other too);
                                             // bit 3: ... with the Downsample conv in front of it and the Upsample transpose conv behind it inside
                                             // the same launch (8x8 -> 4x4 -> ... -> 4x4 -> 8x8: two igemm + slab-reduce pairs less);
                                             // bits 1, 2: the two 8x8 levels (downs[-2]; ups[1]) likewise, one launch each -- built, tested,
                                             // OFF by default: measured 100 us per step SLOWER (150 + 170 us against 104 + 125 for the 16
                                             // launches: a hop moves a 64 KB image to each of 8 workgroups, 5 us of staging and 7 us of
                                             // tail per op where the launches pay 2.9 + 2.4 + 2.0; profiles/r06_chain8_clock.txt, r06_chain8_ab.txt)
    int level_chain_max_batch = 32;          // the chain walks images in rounds of 32 (one workgroup per CU): measured at cfg4 it wins up to ONE round
                                             // (batch 16: 0.984 -> 0.947 ms, 32: 1.282 -> 1.232) and loses from the second on (48: 2.084 -> 2.142,
                                             // 64: 2.071 -> 2.095, 192: 5.753 -> 5.976; tools/chain_batch_ab.py) -- the launches it replaces amortise
                                             // their boundaries over the larger batch, the chain's hops do not (diagnostic option 10 moves the limit)
    int attn_fold_min_hw = 256;              // ... on maps with MORE pixels than this (diagnostic option 9: 255 lets the 16x16, C = 128 site take it)
    bool attn_fold = true;                   // attention on maps with HW > 256, C = 128: q projection + apply + to_out as ONE per-image C x C conv
    // unet_chan % 8 == 0 but not % 32 (reference blocks.py:75 takes any GroupNorm(8, C)): every tensor keeps a pitch of pad32(C) channels
    // with zero padding, the convs run on the generic im2col kernels over zero-padded weights and the normalisations on their
    // generic forms (norm_act.hip) -- correct, untuned, none of the fused paths
    bool generic = false;
    std::vector<int> dimp;                   // dims padded to 32 (== dims unless generic)
    std::vector<Slot> slots;
    size_t packed_floats = 0;
    int L = 0;
    std::vector<int> dims;  // [in, chan*m0, ...]
    int time_dim = 0, temb_total = 0;
    size_t freqs = 0, w1t = 0, b1 = 0, w2t = 0, b2 = 0, temb_wt = 0, temb_bias = 0;
    std::vector<ResW> down_res, up_res;  // 2 per level
    std::vector<AttnW> down_attn, up_attn;
    std::vector<ConvW> down_conv, up_conv;
    ResW mid1, mid2;
    AttnW mid_attn;
    ConvW final_conv;
    NormW final_norm;
    size_t final_w = 0, final_b = 0;

    size_t alloc(size_t n) {
        const size_t o = packed_floats;
        packed_floats += (n + 3) / 4 * 4;
        return o;
    }
    size_t add_copy(const std::string& name, long long n) {
        const size_t o = alloc((size_t)n);
        slots.push_back(Slot{name, n, PK_COPY, o, 0, 0, 0, 0, 0, 0, 0});
        return o;
    }
    void add_copy_at(const std::string& name, long long n, size_t off) {
        slots.push_back(Slot{name, n, PK_COPY, off, 0, 0, 0, 0, 0, 0, 0});
    }
    // split > 0: the cin input channels are the concat of two sources of `split` and cin - split channels, each padded to 32 on its own
    ConvW add_conv(const std::string& prefix, int cout, int cin, int k, bool bias, bool gn_follows = false, int split = 0, bool local = false) {
        ConvW c;
        c.cin = cin; c.cin_pad = split > 0 ? pad32(split) + pad32(cin - split) : pad32(cin); c.cout = cout;
        const int cout_rows = pad32(cout);          // rows beyond cout stay zero (the arena is zero-filled): N as the kernels see it
        c.w = alloc((size_t)cout_rows * k * k * c.cin_pad);
        Slot sl{prefix + "weight", (long long)cout * cin * k * k, PK_CONV, c.w, cout, cin, k, k, c.cin_pad, 0, 0};
        if (split > 0 && c.cin_pad != cin) { sl.split = split; sl.split_pad = pad32(split); }
        slots.push_back(sl);
        c.has_bias = bias;
        if (bias) {
            c.b = alloc((size_t)cout_rows);
            slots.push_back(Slot{prefix + "bias", cout, PK_COPY, c.b, 0, 0, 0, 0, 0, 0, 0});
        }
        if (generic) return c;                      // no Winograd / image-local / first-layer copies: the generic kernels only
        if (k == 1 && bias && cout % 32 == 0 && c.cin_pad == cin && cin % 32 == 0) {
            // to_out / res_conv: also in the operand order of the image-local kernels (level_chain.hip's 1x1 ops)
            c.wl1 = alloc((size_t)cout * c.cin_pad);
            c.has_wl1 = true;
            slots.push_back(Slot{prefix + "weight", (long long)cout * cin, PK_LOCAL1, c.wl1, cout, cin, 1, 1, c.cin_pad, 0, 0});
        }
        if (k == 3 && cout % 64 == 0) {
            // the same state_dict tensor feeds a second slot: its Winograd-domain form G g G^T for conv3x3_wino_kernel
            c.wu = alloc((size_t)16 * cout * c.cin_pad);
            c.has_wu = true;
            slots.push_back(Slot{prefix + "weight", (long long)cout * cin * k * k, PK_WINO, c.wu, cout, cin, k, k, c.cin_pad, 0, 0});
        }
        if (k == 3 && (gn_follows || local) && cout % 32 == 0) {
            // and a third for the one-launch conv + GroupNorm kernel of the 4x4 maps (its MFMA operand order; `local`: the Downsample conv
            // the level chain absorbs)
            c.wl = alloc((size_t)9 * cout * c.cin_pad);
            c.has_wl = true;
            slots.push_back(Slot{prefix + "weight", (long long)cout * cin * k * k, PK_LOCAL, c.wl, cout, cin, k, k, c.cin_pad, 0, 0});
            if (gn_follows && (c.cin_pad <= 320 || c.cin_pad == 512)) {     // (512: the 8x8 level chain walks the concat input as two staged halves)
                c.wwl = alloc((size_t)16 * cout * c.cin_pad);
                c.has_wwl = true;
                slots.push_back(Slot{prefix + "weight", (long long)cout * cin * k * k, PK_WLOCAL, c.wwl, cout, cin, k, k, c.cin_pad, 0, 0});
            }
        }
        return c;
    }
    ConvW add_convT(const std::string& prefix, int ch, bool local = false) {
        ConvW c;
        c.cin = ch; c.cin_pad = pad32(ch); c.cout = ch;
        c.w = alloc((size_t)16 * pad32(ch) * pad32(ch));
        slots.push_back(Slot{prefix + "weight", (long long)16 * ch * ch, PK_CONVT, c.w, ch, ch, 4, 4, pad32(ch), 0, 0});
        c.has_bias = true;
        c.b = alloc((size_t)pad32(ch));
        slots.push_back(Slot{prefix + "bias", ch, PK_COPY, c.b, 0, 0, 0, 0, 0, 0, 0});
        if (local && ch % 32 == 0 && !generic) {
            // ... in the level chain's operand order (four phases x 2 x 2 taps: level_chain.hip, CH_UPT)
            c.wtl = alloc((size_t)16 * ch * ch);
            c.has_wtl = true;
            slots.push_back(Slot{prefix + "weight", (long long)16 * ch * ch, PK_CONVT_LOCAL, c.wtl, ch, ch, 4, 4, ch, 0, 0});
        }
        if (ch % 128 == 0) {
            // the same tensor's Winograd F(2x2, 2x2) form, four phases x 9 positions (conv_winoT_kernel.inc)
            c.wu = alloc((size_t)36 * ch * ch);
            c.has_wu = true;
            slots.push_back(Slot{prefix + "weight", (long long)16 * ch * ch, PK_CONVT_WINO, c.wu, ch, ch, 4, 4, ch, 0, 0});
        }
        return c;
    }
    NormW add_norm(const std::string& wname, const std::string& bname, int c) {
        NormW n;
        n.c_real = c;
        n.g = alloc((size_t)pad32(c));              // padding stays zero
        slots.push_back(Slot{wname, c, PK_COPY, n.g, 0, 0, 0, 0, 0, 0, 0});
        n.b = alloc((size_t)pad32(c));
        slots.push_back(Slot{bname, c, PK_COPY, n.b, 0, 0, 0, 0, 0, 0, 0});
        return n;
    }
    // ci, co: the reference's channel counts; split > 0: the input is the concat (unet.py:97) of `split` + (ci - split) channels
    ResW add_res(const std::string& p, int ci, int co, int& temb_cursor, int split = 0) {
        ResW r;
        r.ci_real = ci; r.co_real = co;
        r.ci = ci; r.ci_pad = split > 0 ? pad32(split) + pad32(ci - split) : pad32(ci); r.co = pad32(co);
        if (!generic) r.co = co;
        r.temb_off = temb_cursor;
        temb_cursor += co;
        slots.push_back(Slot{p + "mlp.1.weight", (long long)co * time_dim, PK_LINEAR_T, temb_wt, co, time_dim, 0, 0, 0, temb_total, r.temb_off});
        add_copy_at(p + "mlp.1.bias", co, temb_bias + r.temb_off);
        r.c1 = add_conv(p + "block1.block.0.", co, ci, 3, true, true, split);
        r.n1 = add_norm(p + "block1.block.1.weight", p + "block1.block.1.bias", co);
        r.c2 = add_conv(p + "block2.block.0.", co, co, 3, true, true);
        r.n2 = add_norm(p + "block2.block.1.weight", p + "block2.block.1.bias", co);
        r.has_res = ci != co;
        if (r.has_res) r.res = add_conv(p + "res_conv.", co, ci, 1, true, false, split);
        if (r.has_res && !generic && r.c1.has_wu && r.res.cin_pad == ci) {
            // the same tensor also as the operand of the skip fold, next to the Winograd copy of the 3x3 conv it rides on
            r.res.wsk = alloc((size_t)co * r.res.cin_pad);
            r.res.has_wsk = true;
            slots.push_back(Slot{p + "res_conv.weight", (long long)co * ci, PK_SKIP_WINO, r.res.wsk, co, ci, 1, 1, r.res.cin_pad, 0, 0});
        }
        return r;
    }
    int n_attn = 0;
    std::vector<AttnW> attn_all;   // copies in creation order (slot.attn indexes this)
    AttnW add_attn(const std::string& p, int c) {
        AttnW a;
        a.c = generic ? pad32(c) : c;
        a.c_real = c;
        const size_t s0 = slots.size();
        a.qkv = add_conv(p + "fn.fn.to_qkv.", 3 * HIDDEN, c, 1, false);
        const size_t s1 = slots.size();
        a.out = add_conv(p + "fn.fn.to_out.", c, HIDDEN, 1, true);
        const size_t s2 = slots.size();
        a.ln = add_norm(p + "fn.norm.g", p + "fn.norm.b", c);
        for (size_t i = s0; i < s1; ++i) slots[i].attn = n_attn;               // to_qkv weight
        for (size_t i = s2; i < slots.size(); ++i) slots[i].attn = n_attn;     // LayerNorm g, b
        a.qkv_lnw = alloc((size_t)3 * HIDDEN * pad32(c));
        a.ln_c1 = alloc((size_t)3 * HIDDEN);
        a.ln_c2 = alloc((size_t)3 * HIDDEN);
        a.qkv_op = alloc((size_t)3 * HIDDEN * pad32(c));
        attn_all.push_back(a);
        ++n_attn;
        return a;
    }
};

static int total_temb(const ddk_unet& u) {
    // 2 ResnetBlocks per down level, 2 mid, 2 per up level; C_out per unet.py:43-66
    int tot = 0;
    for (int l = 0; l < u.L; ++l) tot += 2 * u.dims[l + 1];
    tot += 2 * u.dims[u.L];
    for (int i = 0; i < u.L - 1; ++i) tot += 2 * u.dims[u.L - 1 - i];
    return tot;
}

extern "C" ddk_unet* ddk_unet_create(const ddk_unet_config* cfg) {
    if (!cfg || cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->in_ch < 1 || cfg->chan < 8 || cfg->chan % 8 ||
        cfg->chan > 512) {
        // (GroupNorm(8, C) of blocks.py:75 needs C % 8 == 0 in the reference too; multiples of 32 take the tuned kernels, other
        //  multiples of 8 the generic ones)
        set_error("unet_create: need 1 <= n_levels <= 8, in_ch >= 1, unet_chan a multiple of 8 in [8, 512]");
        return nullptr;
    }
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->mults[i] < 1) { set_error("unet_create: unet_dims entries must be >= 1"); return nullptr; }
    if (cfg->mults[0] != 1) {
        // final_conv is Block(dim, dim) applied to the last up level's dim * unet_dims[0] channels (unet.py:59-72): the reference
        // itself cannot run a forward with unet_dims[0] != 1 (its Conv2d raises on the channel mismatch), so this is not a narrowing
        set_error("unet_create: unet_dims[0] must be 1 (the reference's final Block(dim, dim) meets dim * unet_dims[0] channels "
                  "otherwise and raises, unet.py:69-72)");
        return nullptr;
    }
    {   // best effort: a plan can be created on a host without a GPU (shape / FLOP queries); launches re-check
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && ensure_device_init() != DDK_OK) return nullptr;
        (void)hipGetLastError();
    }
    ddk_unet* u = new ddk_unet();
    u->cfg = *cfg;
    u->L = cfg->n_levels;
    u->generic = cfg->chan % 32 != 0;
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->chan * cfg->mults[i] > 512) { set_error("unet_create: level widths above 512 channels are not supported"); delete u; return nullptr; }
    u->dims.push_back(cfg->in_ch);
    for (int i = 0; i < u->L; ++i) u->dims.push_back(cfg->chan * cfg->mults[i]);
    for (int d : u->dims) u->dimp.push_back(u->generic ? pad32(d) : d);
    u->time_dim = cfg->chan;
    u->temb_total = total_temb(*u);
    const int td = u->time_dim;

    u->freqs = u->add_copy("@sinusoidal_freqs", td / 2);
    u->w1t = u->alloc((size_t)td * 4 * td);
    u->slots.push_back(Slot{"time_mlp.1.weight", (long long)4 * td * td, PK_LINEAR_T, u->w1t, 4 * td, td, 0, 0, 0, 4 * td, 0});
    u->b1 = u->add_copy("time_mlp.1.bias", 4 * td);
    u->w2t = u->alloc((size_t)4 * td * td);
    u->slots.push_back(Slot{"time_mlp.3.weight", (long long)4 * td * td, PK_LINEAR_T, u->w2t, td, 4 * td, 0, 0, 0, td, 0});
    u->b2 = u->add_copy("time_mlp.3.bias", td);
    u->temb_wt = u->alloc((size_t)td * u->temb_total);
    u->temb_bias = u->alloc((size_t)u->temb_total);

    int cur = 0;
    for (int l = 0; l < u->L; ++l) {
        const std::string p = "downs." + std::to_string(l) + ".";
        const int ci = u->dims[l], co = u->dims[l + 1];
        u->down_res.push_back(u->add_res(p + "0.", ci, co, cur));
        if (l == 0 && ci <= 8 && co <= 256 && !u->generic) {
            // the network's first conv also gets conv_first.hip's layout (K = 9 * C_in exactly, unpadded input)
            ConvW& c1 = u->down_res[0].c1;
            const int K2 = (9 * ci + 1) / 2;
            c1.wf = u->alloc((size_t)(co / 32) * K2 * 64);
            c1.has_wf = true;
            u->slots.push_back(Slot{p + "0.block1.block.0.weight", (long long)co * ci * 9, PK_FIRST, c1.wf, co, ci, 3, 3, 0, 0, 0});
        }
        u->down_res.push_back(u->add_res(p + "1.", co, co, cur));
        u->down_attn.push_back(u->add_attn(p + "2.", co));
        if (l < u->L - 1) u->down_conv.push_back(u->add_conv(p + "3.conv.", co, co, 3, true, false, 0, /*local=*/l == u->L - 2));
    }
    const int mid = u->dims[u->L];
    u->mid1 = u->add_res("mid_block1.", mid, mid, cur);
    u->mid_attn = u->add_attn("mid_attn.", mid);
    u->mid2 = u->add_res("mid_block2.", mid, mid, cur);
    for (int i = 0; i < u->L - 1; ++i) {
        const std::string p = "ups." + std::to_string(i) + ".";
        const int din = u->dims[u->L - 1 - i], dout = u->dims[u->L - i];  // reversed(in_out[1:])[i]
        u->up_res.push_back(u->add_res(p + "0.", 2 * dout, din, cur, dout));
        u->up_res.push_back(u->add_res(p + "1.", din, din, cur));
        u->up_attn.push_back(u->add_attn(p + "2.", din));
        u->up_conv.push_back(u->add_convT(p + "3.conv.", din, /*local=*/i == 0));
    }
    u->final_conv = u->add_conv("final_conv.0.block.0.", cfg->chan, cfg->chan, 3, true, true);
    u->final_norm = u->add_norm("final_conv.0.block.1.weight", "final_conv.0.block.1.bias", cfg->chan);
    if (u->generic) {        // rows of pitch pad32(chan): the projection reads the padded activation
        u->final_w = u->alloc((size_t)cfg->in_ch * pad32(cfg->chan));
        u->slots.push_back(Slot{"final_conv.1.weight", (long long)cfg->in_ch * cfg->chan, PK_ROWS, u->final_w, cfg->in_ch, cfg->chan, 0, 0, 0,
                                pad32(cfg->chan), 0});
    } else {
        u->final_w = u->add_copy("final_conv.1.weight", (long long)cfg->in_ch * cfg->chan);
    }
    u->final_b = u->add_copy("final_conv.1.bias", cfg->in_ch);
    if (cur != u->temb_total) {
        set_error("unet_create: internal temb accounting mismatch");
        delete u;
        return nullptr;
    }
    return u;
}

static void drop_graphs(ddk_unet* u) {   // caller holds u->mu (or owns u exclusively)
    for (SamplerGraph& g : u->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
        if (g.exec_multi) (void)hipGraphExecDestroy(g.exec_multi);
        if (g.graph_multi) (void)hipGraphDestroy(g.graph_multi);
        if (g.done) (void)hipEventDestroy(g.done);
    }
    u->graphs.clear();
    u->table.ws = nullptr;
}

/* Destroying a plan that has captured sampler graphs waits for the device first (an executable graph must outlive its
   in-flight launches). */
extern "C" void ddk_unet_destroy(ddk_unet* u) {
    if (!u) return;
    if (!u->graphs.empty()) (void)hipDeviceSynchronize();
    drop_graphs(u);
    delete u;
}

extern "C" int ddk_sampler_invalidate(ddk_unet* u) {
    DDK_REQUIRE(u, "sampler_invalidate: null plan");
    std::lock_guard<std::mutex> lock(u->mu);
    if (!u->graphs.empty()) DDK_HIP(hipDeviceSynchronize());
    drop_graphs(u);
    return DDK_OK;
}
static void destroy_entry(SamplerGraph& g) {
    if (g.done) { (void)hipEventSynchronize(g.done); (void)hipEventDestroy(g.done); }
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    if (g.exec_multi) (void)hipGraphExecDestroy(g.exec_multi);
    if (g.graph_multi) (void)hipGraphDestroy(g.graph_multi);
}

/* Drops only what points into `workspace` (the caller is about to free or reuse it): the cached graphs captured on it, after
   waiting for THEIR launches (the per-entry event), and the shift table if it lives there.  Other buffer sets keep their graphs. */
extern "C" int ddk_sampler_release_workspace(ddk_unet* u, const void* workspace) {
    DDK_REQUIRE(u && workspace, "sampler_release_workspace: arguments");
    std::lock_guard<std::mutex> lock(u->mu);
    for (size_t i = 0; i < u->graphs.size();) {
        if (u->graphs[i].key.ws == workspace) {
            destroy_entry(u->graphs[i]);
            u->graphs.erase(u->graphs.begin() + (long)i);
        } else {
            ++i;
        }
    }
    if (u->table.ws == workspace) u->table.ws = nullptr;
    return DDK_OK;
}

extern "C" int ddk_unet_set_option(ddk_unet* u, int option, int value) {
    DDK_REQUIRE(u, "unet_set_option: null plan");
    // a captured step bakes every choice in: setting one waits for the cached graphs and drops them first (drops_graphs)
    static const struct {
        int option;
        bool drops_graphs;
        void (*set)(ddk_unet&, int);
    } options[] = {
        {DDK_OPT_CLUSTER_GROUPNORM, true, [](ddk_unet& p, int v) { p.cluster_gn = v < 0 ? 0 : v > 2 ? 2 : v; }},
        {DDK_OPT_ATTENTION_FOLD, true, [](ddk_unet& p, int v) { p.attn_fold = v != 0; }},
        {DDK_OPT_ATTENTION_KV_CONTEXT, true, [](ddk_unet& p, int v) { p.attn_kvctx = v != 0; }},
        {DDK_OPT_FIRST_GROUPNORM, true, [](ddk_unet& p, int v) { p.first_gn = v != 0; }},
        {DDK_OPT_RESTORE_FUSED_TAIL, true, [](ddk_unet& p, int v) { p.restore_fused = v != 0; }},
        {DDK_OPT_ATTENTION_SPLIT, true, [](ddk_unet& p, int v) { p.attn_split = v != 0; }},
        {DDK_OPT_SKIP_FOLD, true, [](ddk_unet& p, int v) { p.skip_fold = v != 0; }},
        {DDK_OPT_ATTENTION_FOLD_PARTIALS, true, [](ddk_unet& p, int v) { p.attn_fold_parts = v != 0; }},
        // 0 off, 1 (default): the 4x4 level with its Downsample / Upsample convs, 2: the 4x4 level alone, 3: the 8x8 levels as well,
        // 4: the 8x8 levels only, 8 / 16: only downs[-2] / only ups[1]
        {DDK_OPT_LEVEL_CHAIN, true, [](ddk_unet& p, int v) {
             p.level_chain = v == 1 ? 9 : v == 2 ? 1 : v == 3 ? 15 : v == 4 ? 6 : v == 8 ? 2 : v == 16 ? 4 : v != 0 ? 9 : 0;
         }},
        {DDK_OPT_FOLD_DOWNSAMPLE_REDUCE, true, [](ddk_unet& p, int v) { p.fold_down_reduce = v != 0; }},
        // diagnostics (not in ddk.h): largest batch the level chain takes; the folded attention block from this many pixels up;
        // cap on the cluster launches per forward (no graph is dropped); largest cluster size that takes the in-launch GroupNorm;
        // the in-launch GroupNorm on channel-chunk-split shapes
        {10, true, [](ddk_unet& p, int v) { p.level_chain_max_batch = v; }},
        {9, true, [](ddk_unet& p, int v) { p.attn_fold_min_hw = v; }},
        {2, false, [](ddk_unet& p, int v) { p.cluster_limit = v; }},
        {4, true, [](ddk_unet& p, int v) { p.cluster_np_max = v; }},
        {11, true, [](ddk_unet& p, int v) { p.cluster_split = v != 0; }},
    };
    for (const auto& o : options) {
        if (o.option != option) continue;
        std::lock_guard<std::mutex> lock(u->mu);
        if (o.drops_graphs) {
            if (!u->graphs.empty()) DDK_HIP(hipDeviceSynchronize());
            drop_graphs(u);
        }
        o.set(*u, value);
        return DDK_OK;
    }
    return fail_arg("unet_set_option: unknown option");
}
extern "C" unsigned ddk_debug_cluster_timeouts(void) {
    unsigned sum = 0;
    for (unsigned v : {ddk::conv_wino_cluster_timeouts(), ddk::conv_first_cluster_timeouts(), ddk::level_chain_cluster_timeouts(),
                       ddk::attention_cluster_timeouts()}) {
        if (v == ~0u) return ~0u;
        sum += v;
    }
    return sum;
}
extern "C" int ddk_unet_num_slots(const ddk_unet* u) { return u ? (int)u->slots.size() : 0; }
extern "C" const char* ddk_unet_slot_name(const ddk_unet* u, int slot) {
    return (u && slot >= 0 && slot < (int)u->slots.size()) ? u->slots[slot].name.c_str() : nullptr;
}
extern "C" long long ddk_unet_slot_numel(const ddk_unet* u, int slot) {
    return (u && slot >= 0 && slot < (int)u->slots.size()) ? u->slots[slot].numel : -1;
}
extern "C" size_t ddk_unet_packed_bytes(const ddk_unet* u) { return u ? u->packed_floats * sizeof(float) : 0; }

// w[n][c] (packed 1x1 weight, row pitch cp) -> wg[n][c] = w*g[c], c1[n] = sum_c w*g, c2[n] = sum_c w*b   (one wave per n)
__global__ __launch_bounds__(64) void ln_fold_kernel(const float* __restrict__ w, const float* __restrict__ g, const float* __restrict__ b,
                                                     float* __restrict__ wg, float* __restrict__ c1, float* __restrict__ c2, int C, int cp) {
    const int n = blockIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int c = threadIdx.x; c < cp; c += 64) {
        const float wv = w[(long long)n * cp + c];
        const float gv = c < C ? g[c] : 0.f, bv = c < C ? b[c] : 0.f;
        wg[(long long)n * cp + c] = wv * gv;
        s1 += wv * gv;
        s2 += wv * bv;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x == 0) { c1[n] = s1; c2[n] = s2; }
}

static int fold_attn(const AttnW& a, float* P, hipStream_t st) {
    hipLaunchKernelGGL(ln_fold_kernel, dim3(3 * HIDDEN), dim3(64), 0, st, P + a.qkv.w, P + a.ln.g, P + a.ln.b, P + a.qkv_lnw, P + a.ln_c1,
                       P + a.ln_c2, a.c, pad32(a.c));
    DDK_TRY(check_launch("ln_fold_kernel"));
    return qkv_operand_pack(P + a.qkv_lnw, P + a.qkv_op, HEADS, pad32(a.c), st);
}

// Derived weights of every attention site.  ddk_unet_pack_slot already re-derives a site's weights whenever one of its three
// source slots is packed (so a caller that packs every slot, in any order, ends up consistent); this entry point re-derives
// all of them explicitly, e.g. after writing into the packed arena by other means.
static void weights_changed(const ddk_unet* u) {
    ddk_unet* m = const_cast<ddk_unet*>(u);      // the cache bookkeeping is logically mutable
    std::lock_guard<std::mutex> lock(m->mu);
    ++m->pack_epoch;
}

extern "C" int ddk_unet_finalize_pack(const ddk_unet* u, void* packed, ddk_stream_t s) {
    DDK_REQUIRE(u && packed, "unet_finalize_pack: arguments");
    weights_changed(u);
    for (const AttnW& a : u->attn_all) DDK_TRY(fold_attn(a, static_cast<float*>(packed), as_stream(s)));
    return DDK_OK;
}

extern "C" int ddk_unet_pack_slot(const ddk_unet* u, int slot, const float* canonical, void* packed, ddk_stream_t s) {
    DDK_REQUIRE(u && canonical && packed && slot >= 0 && slot < (int)u->slots.size(), "unet_pack_slot: arguments");
    const Slot& sl = u->slots[slot];
    float* dst = static_cast<float*>(packed) + sl.off;
    weights_changed(u);
    int rc;
    switch (sl.kind) {
        case PK_COPY:
            DDK_HIP(hipMemcpyAsync(dst, canonical, (size_t)sl.numel * sizeof(float), hipMemcpyDeviceToDevice, as_stream(s)));
            rc = DDK_OK;
            break;
        case PK_CONV:
            rc = sl.split > 0 ? ddk_pack_conv_weight_split(canonical, dst, sl.O, sl.I, sl.KH, sl.KW, sl.i_pad, sl.split, sl.split_pad, s)
                              : ddk_pack_conv_weight(canonical, dst, sl.O, sl.I, sl.KH, sl.KW, sl.i_pad, s);
            break;
        case PK_CONVT: rc = sl.i_pad == sl.I ? ddk_pack_convT_weight(canonical, dst, sl.I, sl.O, s)
                                             : ddk_pack_convT_weight_padded(canonical, dst, sl.I, sl.O, sl.i_pad, s); break;
        case PK_ROWS:
            DDK_HIP(hipMemcpy2DAsync(dst, (size_t)sl.ld * sizeof(float), canonical, (size_t)sl.I * sizeof(float), (size_t)sl.I * sizeof(float),
                                     (size_t)sl.O, hipMemcpyDeviceToDevice, as_stream(s)));
            rc = DDK_OK;
            break;
        case PK_LINEAR_T: rc = ddk_pack_linear_T(canonical, dst, sl.O, sl.I, sl.ld, sl.col0, s); break;
        case PK_WINO: rc = ddk_pack_conv_weight_wino(canonical, dst, sl.O, sl.I, sl.i_pad, s); break;
        case PK_LOCAL: rc = ddk_pack_conv_weight_local(canonical, dst, sl.O, sl.I, sl.i_pad, s); break;
        case PK_LOCAL1: rc = ddk_pack_conv1x1_weight_local(canonical, dst, sl.O, sl.I, sl.i_pad, s); break;
        case PK_SKIP_WINO: rc = ddk_pack_conv_skip_weight_wino(canonical, dst, sl.O, sl.I, sl.i_pad, s); break;
        case PK_CONVT_LOCAL: rc = ddk_pack_convT_weight_local(canonical, dst, sl.I, sl.O, s); break;
        case PK_WLOCAL: rc = ddk_pack_conv_weight_wino_local(canonical, dst, sl.O, sl.I, sl.i_pad, s); break;
        case PK_FIRST: rc = ddk_pack_conv_weight_first(canonical, dst, sl.O, sl.I, s); break;
        case PK_CONVT_WINO: rc = ddk_pack_convT_weight_wino(canonical, dst, sl.I, sl.O, sl.i_pad, s); break;
        default: return fail_arg("unet_pack_slot: slot kind");
    }
    DDK_TRY(rc);
    // to_qkv weight / LayerNorm g / b of an attention site: re-derive its folded weights (stream-ordered after the pack above;
    // whichever of the three is packed last leaves them consistent)
    if (sl.attn >= 0) DDK_TRY(fold_attn(u->attn_all[sl.attn], static_cast<float*>(packed), as_stream(s)));
    return DDK_OK;
}

// ------------------------------------------------------------------------------------------------
namespace ddk {

// Workspace carve-up (all offsets in floats, 16-byte aligned).
struct Layout {
    size_t act = 0;      // one general activation buffer (max over layers of M*C)
    size_t qkv = 0, o = 0, ctx = 0, splitk = 0, gn_ws = 0, cl = 0, chain = 0;
    std::vector<size_t> skip;  // per level
    size_t xpad = 0, temb = 0, tact = 0;
    // offsets
    size_t off_A = 0, off_B = 0, off_C = 0, off_raw = 0, off_a1 = 0, off_res = 0, off_xn = 0, off_qkv = 0, off_o = 0, off_ctx = 0,
           off_splitk = 0, off_gn = 0, off_xpad = 0, off_temb = 0, off_tact = 0, off_cl = 0, off_chain = 0;
    std::vector<size_t> off_skip;
    size_t total = 0;
};

static size_t al4(size_t n) { return (n + 3) / 4 * 4; }

static void upd(size_t& m, size_t v) { if (v > m) m = v; }

// The 3x3 stride-1 convs run as Winograd F(2x2,3x3) wherever the shape allows (conv_wino.hip); their split count and slab
// workspace follow that kernel's plan.
static bool convT_wino_use(int B, int H, int W, int cin, int N) {
    return convT_wino_ok(H, W, cin, N) && convT_wino_splits(B, H, W, cin, N) <= 2;
}
static bool use_wino(const ConvW& cw, int H, int W, int cin, int N) {
    return cw.has_wu && conv_wino_ok(DDK_CONV3X3_S1, H, W, cin, N);
}
static size_t conv3_ws_floats(const ConvW& cw, int B, int H, int W, int cin, int N) {
    if (!use_wino(cw, H, W, cin, N)) return conv_workspace_bytes(DDK_CONV3X3_S1, B, H, W, cin, N) / 4;
    const int s = conv_wino_splits(B, H, W, cin, N);
    return s > 1 ? (size_t)s * B * H * W * N : 0;
}

// (the cluster counter area in front of the records: cl_counter_floats() and its offsets, ddk_internal.h)
constexpr int CHAIN_BUFS = 18;                // activations that cross workgroups inside the level chain, [B][16][256] each
constexpr int CHAIN8_BUFS = 5;                // ... inside an 8x8 chain, [B][64][256] each

static void res_sizes(const ResW& r, int B, int H, int W, Layout& ly) {
    const size_t M = (size_t)B * H * W;
    upd(ly.act, M * r.co);
    // (a first conv that carries the skip fold keeps the skip conv's partial slabs behind its own: DDK_OPT_SKIP_FOLD)
    upd(ly.splitk, (r.has_res && r.res.has_wsk ? 2 : 1) * conv3_ws_floats(r.c1, B, H, W, r.ci_pad, r.co));
    upd(ly.splitk, conv3_ws_floats(r.c2, B, H, W, r.co, r.co));
    if (r.has_res) upd(ly.splitk, conv_workspace_bytes(DDK_CONV1X1, B, H, W, r.ci_pad, r.co) / 4);
    upd(ly.gn_ws, groupnorm_workspace_bytes(B, H * W, r.co, GROUPS) / 4);
    upd(ly.gn_ws, (size_t)2 * GROUPS * (M / 128 + 1));      // {mean, M2} partials the Winograd conv leaves for GroupNorm
    upd(ly.cl, cl_counter_floats(B) + conv_wino_cluster_ws_floats(B, H, W, r.co));   // cluster GroupNorm: counters, then records
    if (H * W % 128 == 0 && H * W / 128 <= 8) upd(ly.cl, cl_counter_floats(B) + conv_first_gn_ws_floats(B, H, W));   // ... of the first Block
}

static void attn_sizes(const AttnW& a, int B, int H, int W, Layout& ly) {
    const size_t M = (size_t)B * H * W;
    upd(ly.act, M * a.c);
    upd(ly.qkv, M * 3 * HIDDEN);
    upd(ly.o, M * HIDDEN);
    upd(ly.ctx, (size_t)B * HEADS * 32 * 32);
    upd(ly.splitk, linattn_context_workspace_bytes(B, H * W, HEADS) / 4);   // the context partials reuse the split-K slab area
    if (attn_kvctx_ok(B, H * W, a.c, HEADS)) upd(ly.splitk, attn_kvctx_workspace_bytes(B, H * W) / 4);
    upd(ly.splitk, conv_workspace_bytes(DDK_CONV1X1, B, H, W, a.c, 3 * HIDDEN) / 4);
    upd(ly.splitk, conv_workspace_bytes(DDK_CONV1X1, B, H, W, HIDDEN, a.c) / 4);
    if ((H * W == 64 || H * W == 256) && B <= 32) upd(ly.cl, cl_counter_floats(B) + attn_split_record_floats(B));   // the pixel-split launch's records
}

// The level chain (level_chain.hip) takes the last level when it is a 4x4 map of 256 channels whose neighbours are 256 wide too (cfg1,
// cfg2, cfg4): ResnetBlocks without a skip conv on the way down and in the middle, one 512 -> 256 ResnetBlock on the way up.
static bool chain_plain(const ResW& r, bool wino) {
    return r.ci == 256 && r.co == 256 && !r.has_res && r.c1.has_bias && r.c2.has_bias && (wino ? r.c1.has_wwl && r.c2.has_wwl : r.c1.has_wl && r.c2.has_wl);
}
static bool chain_att(const AttnW& a) { return a.c == 256 && a.out.has_wl1 && a.out.has_bias; }
static bool chain_cat(const ResW& r, bool wino) {
    return r.ci == 512 && r.ci_pad == 512 && r.co == 256 && r.has_res && r.res.has_wl1 && r.res.has_bias && r.c1.cin_pad == 512 && r.c1.has_bias &&
           r.c2.has_bias && (wino ? r.c1.has_wwl && r.c2.has_wwl : r.c1.has_wl && r.c2.has_wl);
}
static bool level_chain_shape_ok(const ddk_unet& u, int H0, int W0) {
    if (u.generic || u.L < 2) return false;
    const int sh = u.L - 1;
    if ((H0 >> sh) != 4 || (W0 >> sh) != 4 || (H0 & ((1 << sh) - 1)) || (W0 & ((1 << sh) - 1))) return false;
    if (u.dimp[u.L] != 256 || u.dimp[u.L - 1] != 256 || GROUPS != 8) return false;
    return chain_plain(u.down_res[2 * sh], false) && chain_plain(u.down_res[2 * sh + 1], false) && chain_plain(u.mid1, false) &&
           chain_plain(u.mid2, false) && chain_plain(u.up_res[1], false) && chain_att(u.down_attn[sh]) && chain_att(u.mid_attn) &&
           chain_att(u.up_attn[0]) && chain_cat(u.up_res[0], false);
}
// ... and the level above it when that is an 8x8 map of 256 channels between 256-wide neighbours (cfg4: downs[2] and ups[1])
static bool level8_chain_shape_ok(const ddk_unet& u, int H0, int W0) {
    if (u.generic || u.L < 3) return false;
    const int sh = u.L - 2;
    if ((H0 >> sh) != 8 || (W0 >> sh) != 8 || (H0 & ((1 << sh) - 1)) || (W0 & ((1 << sh) - 1))) return false;
    if (u.dimp[sh + 1] != 256 || u.dimp[sh] != 256 || u.dimp[sh + 2] != 256 || GROUPS != 8) return false;
    return chain_plain(u.down_res[2 * sh], true) && chain_plain(u.down_res[2 * sh + 1], true) && chain_att(u.down_attn[sh]) &&
           chain_cat(u.up_res[2], true) && chain_plain(u.up_res[3], true) && chain_att(u.up_attn[1]);
}

static Layout make_layout(const ddk_unet& u, int B, int H0, int W0) {
    Layout ly;
    int H = H0, W = W0;
    ly.skip.resize(u.L);
    for (int l = 0; l < u.L; ++l) {
        res_sizes(u.down_res[2 * l], B, H, W, ly);
        res_sizes(u.down_res[2 * l + 1], B, H, W, ly);
        attn_sizes(u.down_attn[l], B, H, W, ly);
        ly.skip[l] = al4((size_t)B * H * W * u.dimp[l + 1]);
        if (l < u.L - 1) {
            upd(ly.splitk, conv_workspace_bytes(DDK_CONV3X3_S2, B, H, W, u.dimp[l + 1], u.dimp[l + 1]) / 4);
            H /= 2; W /= 2;
            upd(ly.act, (size_t)B * H * W * u.dimp[l + 1]);
        }
    }
    res_sizes(u.mid1, B, H, W, ly);
    attn_sizes(u.mid_attn, B, H, W, ly);
    res_sizes(u.mid2, B, H, W, ly);
    for (int i = 0; i < u.L - 1; ++i) {
        res_sizes(u.up_res[2 * i], B, H, W, ly);
        res_sizes(u.up_res[2 * i + 1], B, H, W, ly);
        attn_sizes(u.up_attn[i], B, H, W, ly);
        const int c = pad32(u.up_conv[i].cout);
        upd(ly.splitk, conv_workspace_bytes(DDK_CONVT4X4_S2, B, H, W, c, c) / 4);
        H *= 2; W *= 2;
        upd(ly.act, (size_t)B * H * W * c);
    }
    upd(ly.act, (size_t)B * H * W * pad32(u.cfg.chan));
    upd(ly.splitk, conv3_ws_floats(u.final_conv, B, H, W, pad32(u.cfg.chan), pad32(u.cfg.chan)));
    upd(ly.gn_ws, groupnorm_workspace_bytes(B, H * W, pad32(u.cfg.chan), GROUPS) / 4);
    upd(ly.gn_ws, (size_t)2 * GROUPS * ((size_t)B * H * W / 128 + 1));
    ly.xpad = al4((size_t)B * H0 * W0 * pad32(u.cfg.in_ch));
    ly.temb = al4((size_t)B * u.temb_total);
    ly.tact = al4((size_t)B * u.time_dim);
    ly.act = al4(ly.act); ly.qkv = al4(ly.qkv); ly.o = al4(ly.o); ly.ctx = al4(ly.ctx);
    ly.splitk = al4(ly.splitk); ly.gn_ws = al4(ly.gn_ws); ly.cl = al4(ly.cl);
    if (level_chain_shape_ok(u, H0, W0)) ly.chain = (size_t)CHAIN_BUFS * B * 16 * 256;
    if (level8_chain_shape_ok(u, H0, W0)) upd(ly.chain, (size_t)CHAIN8_BUFS * B * 64 * 256);     // the chains run one after the other

    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += n; return o; };
    ly.off_A = take(ly.act); ly.off_B = take(ly.act); ly.off_C = take(ly.act);
    ly.off_raw = take(ly.act); ly.off_a1 = take(ly.act); ly.off_res = take(ly.act); ly.off_xn = take(ly.act);
    ly.off_qkv = take(ly.qkv); ly.off_o = take(ly.o); ly.off_ctx = take(ly.ctx);
    ly.off_splitk = take(ly.splitk); ly.off_gn = take(ly.gn_ws); ly.off_cl = take(ly.cl); ly.off_chain = take(ly.chain);
    ly.off_xpad = take(ly.xpad); ly.off_temb = take(ly.temb); ly.off_tact = take(ly.tact);
    ly.off_skip.resize(u.L);
    for (int l = 0; l < u.L; ++l) ly.off_skip[l] = take(ly.skip[l]);
    ly.total = off;
    return ly;
}

struct Ctx {
    const ddk_unet& u;
    const float* P;  // packed weights
    float* W;        // workspace base
    const Layout& ly;
    int B;
    hipStream_t st;
    const float* temb;            // [B][temb_total], or the sampler's per-timestep table [t_start+1][temb_total]
    const long long* temb_rows;   // nullptr: row b;  sampler: row = t_cur[b] (device), so one table serves every step
    bool allow_cluster = false;   // this call's owner checks ddk_unet_cluster_check (sampler; forward only with option value 2)
    int n_cluster = 0;            // cluster launches issued so far in this forward
    const float* x_first = nullptr;   // the network input, unpadded, and its padded copy: the first conv may take the small-C_in
    const float* x_padded = nullptr;  // kernel on maps the one-launch first block does not cover (run_conv_gn)

    // The arguments of one conv of this forward: kind, sources, weight, its Winograd form where the shape takes it, bias, shape and the
    // split-K workspace.  A site adds only what is special to it: resid, gn_partials, defer_reduce (whose slabs' reader adds the bias).
    ddk_conv_args conv_args(int kind, const ConvW& cw, const float* src0, int c0, const float* src1, int c1, float* out, int H, int Wd, int N,
                            const float* weight_override = nullptr) const {
        ddk_conv_args a{};
        a.kind = kind;
        a.src0 = src0; a.src1 = src1; a.c0 = c0; a.c1 = c1;
        a.weight = weight_override ? weight_override : P + cw.w;
        a.bias = cw.has_bias ? P + cw.b : nullptr;
        a.out = out;
        a.B = B; a.H = H; a.W = Wd; a.N = N;
        a.workspace = W + ly.off_splitk;
        a.workspace_bytes = ly.splitk * sizeof(float);
        if (kind == DDK_CONV3X3_S1 && !weight_override && use_wino(cw, H, Wd, c0 + c1, N)) a.weight_wino = P + cw.wu;
        // (measured, B = 32: 128 ch 16 -> 32: 47.8 -> 28.0 us; 256 ch 8 -> 16 (2 slabs): 49.4 -> 37.0; 256 ch 4 -> 8 would need 8 slabs of one
        //  chunk each and loses, 20.7 -> 21.9: the direct kernel keeps the maps that small)
        if (kind == DDK_CONVT4X4_S2 && !weight_override && cw.has_wu && !src1 && convT_wino_use(B, H, Wd, c0, N)) a.weight_wino = P + cw.wu;
        return a;
    }
    // GroupNorm + Mish (+ time shift, its rows) finished inside a conv's launch, exchanging through this workspace's cluster area
    WinoGnFuse gn_fuse(const NormW& n, const float* temb_shift, const long long* rows) const {
        float* cl = W + ly.off_cl;
        const ClWords w = cl_words(cl, B);
        return WinoGnFuse{P + n.g, P + n.b, temb_shift, rows, u.temb_total, GN_EPS, GROUPS, cl + cl_counter_floats(B), w.counters, w.fail};
    }
};

// The skip fold's operands (ddk_conv_args.skip_*): a res_conv computed inside the 3x3 conv launch that reads the same input
struct SkipFold {
    const float* w = nullptr;
    const float* b = nullptr;
    float* out = nullptr;
    bool want_slabs = false;    // where the conv leaves split-K slabs for its GroupNorm (CG_SLABS), leave the skip partials as slabs too,
                                // behind the conv's in the workspace: the caller has a reader that sums them (+ bias)
    mutable int left = 0;       // > 1: that many skip slabs were left there and `out` is unwritten
    void put(ddk_conv_args& a) const { a.skip_weight = w; a.skip_bias = b; a.skip_out = out; }
};
static int run_conv(Ctx& c, int kind, const ConvW& cw, const float* src0, int c0, const float* src1, int c1, const float* resid,
                    float* out, int H, int W, int N, const float* weight_override = nullptr, const ConvLnFold* ln = nullptr,
                    const SkipFold& sk = SkipFold()) {
    ddk_conv_args a = c.conv_args(kind, cw, src0, c0, src1, c1, out, H, W, N, weight_override);
    a.resid = resid;
    sk.put(a);
    return conv_forward(a, c.st, ln);
}
// ... leaving its `splits` split-K slabs in the workspace (`out` is not written) for a reader that sums them and adds the bias: `left`
static int run_conv_slabs(Ctx& c, int kind, const ConvW& cw, const float* src0, int c0, const float* src1, int c1, float* out, int H, int W, int N,
                          int splits, AddendSlabs& left, const SkipFold& sk = SkipFold()) {
    ddk_conv_args a = c.conv_args(kind, cw, src0, c0, src1, c1, out, H, W, N);
    a.bias = nullptr;
    a.defer_reduce = 1;
    sk.put(a);
    if (sk.out && sk.want_slabs) {
        const long long slab = (long long)c.B * H * W * N;
        a.skip_out = c.W + c.ly.off_splitk + (long long)splits * slab;
        a.skip_slab_stride = slab;
        sk.left = splits;
    }
    const int s = kind == DDK_CONV3X3_S2 ? 2 : 1;
    left = AddendSlabs{splits, (long long)c.B * (H / s) * (W / s) * N, cw.has_bias ? c.P + cw.b : nullptr};
    return conv_forward(a, c.st);
}
// ... as a one-pass Winograd conv whose epilogue leaves per-tile {mean, M2} in the GroupNorm area (shapes with conv_wino_stats_parts() > 0)
static int run_conv_parts(Ctx& c, const ConvW& cw, const float* src0, int c0, const float* src1, int c1, float* raw, int H, int W, int N,
                          const SkipFold& sk = SkipFold()) {
    ddk_conv_args a = c.conv_args(DDK_CONV3X3_S1, cw, src0, c0, src1, c1, raw, H, W, N);
    sk.put(a);
    a.gn_partials = c.W + c.ly.off_gn;
    a.gn_groups = GROUPS;
    return conv_forward(a, c.st);
}

// conv3x3 -> GroupNorm + Mish (+ shift) (+ residual): the kernels it can run on, in the order of precedence classify_conv_gn tests them
enum ConvGnPath {
    CG_GENERIC,        // widths that are not multiples of 32: plain conv over the zero-padded weights, then GroupNorm over the REAL channels
    CG_LOCAL,          // 4x4 maps (and 2x2 maps, four images to a block): one image x 32 channels per workgroup, k reduced inside it ->
                       // statistics, Mish, shift and residual in the conv's own epilogue, no slabs, no GroupNorm launch (conv_local.hip)
    CG_WLOCAL,         // 8x8 maps: the same image-local tiling in Winograd form
    CG_FIRST,          // the network's first conv on a map too large for the one-launch first block (256x256: 512 statistics tiles per
                       // image): the K = 9 C_in kernel on the unpadded input, not a 32-channel im2col conv (724 -> ~70 us at 8 x 256 x 256)
    CG_CLUSTER,        // one launch: the workgroups of an image exchange their tile statistics and normalise their own tile in registers
    CG_CLUSTER_SPLIT,  // ... on a shape whose channel chunks are split over workgroups (16x16 maps of 64-channel tiles at batch 32): a
                       // tile's first workgroup sums its partners' partial tiles in the launch -- no slabs left, no GroupNorm launch
    CG_PARTS,          // one-pass Winograd conv: its epilogue leaves per-tile {mean, M2}; GroupNorm then is a single streaming read + write
    CG_SLABS,          // the conv splits k, the GroupNorm is register-resident: the slabs stay in the workspace and the GroupNorm kernel
                       // sums them (plus the conv bias) while loading -- one kernel and one HBM round trip fewer
    CG_PLAIN           // conv, then GroupNorm
};
struct ConvGnChoice {
    ConvGnPath path = CG_PLAIN;
    int np = 0;            // statistics tiles per image (CG_CLUSTER, CG_CLUSTER_SPLIT: the cluster's workgroups; CG_PARTS)
    int cl_splits = 1;     // CG_CLUSTER_SPLIT: channel-chunk splits
    int splits = 1;        // CG_SLABS, CG_PLAIN: split-K slabs
    bool wino = false;     // past the image-local paths: the conv is a Winograd F(2x2,3x3) launch (what ddk_unet_flops_executed prices)
    bool local() const { return path == CG_LOCAL || path == CG_WLOCAL; }
};
// No side effects.  first_input: the source is the padded copy of the network input (and the unpadded one is at hand).  cluster: an
// in-launch GroupNorm may still be issued by this call -- the caller passes allow_cluster && n_cluster < cluster_limit and counts the
// launch when a cluster path comes back.  (The ladder this replaces tested `n_cluster++ < cluster_limit` last in each cluster
// condition; a count that has reached the limit can only fail that test, so not counting past the limit changes nothing.)
// splitk_floats: the workspace's split-K area, which CG_CLUSTER_SPLIT's partial tiles must fit.
static ConvGnChoice classify_conv_gn(const ddk_unet& u, const ConvW& cw, int B, int H, int W, int c0, int c1, int N, bool first_input,
                                     bool cluster, size_t splitk_floats) {
    ConvGnChoice k;
    const int cin = c0 + c1;
    auto is = [&](ConvGnPath p) { k.path = p; return k; };
    if (u.generic) return is(CG_GENERIC);
    if (cw.has_wl && (H * W == 16 || (H * W == 4 && B % 4 == 0)) && conv_gn_local_ok(H, W, cin, c0, N, GROUPS)) return is(CG_LOCAL);
    if (cw.has_wwl && H * W == 64 && conv_gn_wlocal_ok(H, W, cin, c0, N, GROUPS)) return is(CG_WLOCAL);
    k.wino = use_wino(cw, H, W, cin, N);
    if (cw.has_wf && first_input && conv_first_ok(u.cfg.in_ch, N, H, W, GROUPS)) return is(CG_FIRST);
    cluster = cluster && cw.has_wu && conv_wino_cluster_device_ok();
    k.np = cluster ? conv_wino_cluster_np(B, H, W, cin, N, GROUPS) : 0;
    if (k.np > 0 && k.np <= u.cluster_np_max) return is(CG_CLUSTER);
    k.np = cluster && u.cluster_split ? conv_wino_cluster_split_np(B, H, W, cin, N, GROUPS, &k.cl_splits) : 0;
    if (k.np > 0 && k.np <= u.cluster_np_max && (size_t)k.cl_splits * B * H * W * N <= splitk_floats &&
        conv_wino_cluster_pair_words(B, H, W, N) <= CL_PAIR_WORDS)
        return is(CG_CLUSTER_SPLIT);
    k.np = cw.has_wu ? conv_wino_stats_parts(B, H, W, cin, N, GROUPS) : 0;
    if (k.np > 0) return is(CG_PARTS);
    k.splits = k.wino ? conv_wino_splits(B, H, W, cin, N) : conv_splits(DDK_CONV3X3_S1, B, H, W, cin, N);
    return is(k.splits > 1 && groupnorm_workspace_bytes(B, H * W, N, GROUPS) == 0 ? CG_SLABS : CG_PLAIN);
}
static bool conv_gn_is_local(const ddk_unet& u, const ConvW& cw, int B, int H, int W, int c0, int c1, int N) {
    return classify_conv_gn(u, cw, B, H, W, c0, c1, N, false, false, 0).local();
}

static int run_conv_gn(Ctx& c, const ConvW& cw, const float* src0, int c0, const float* src1, int c1, float* raw, const NormW& n,
                       const float* temb, const float* addend, float* out, int H, int W, int N, const AddendSlabs& as = AddendSlabs(),
                       const AddendSlabs& ss = AddendSlabs(), const SkipFold& sk = SkipFold()) {
    const ConvGnChoice k = classify_conv_gn(c.u, cw, c.B, H, W, c0, c1, N, c.x_first && src0 == c.x_padded && !src1,
                                            c.allow_cluster && c.n_cluster < c.u.cluster_limit, c.ly.splitk);
    // (res_folds_skip admits exactly the shapes whose every choice here is one of these Winograd forms)
    if (sk.out && !(k.wino && (k.path == CG_CLUSTER || k.path == CG_CLUSTER_SPLIT || k.path == CG_PARTS || k.path == CG_SLABS || k.path == CG_PLAIN)))
        return fail_arg("run_conv_gn: skip fold on a path that cannot carry it");
    if (ss.n > 1 && !k.local()) return fail_arg("run_conv_gn: slab source on a path that cannot sum it");
    if (as.n > 1 && !k.local())
        return fail_arg(k.path == CG_GENERIC ? "run_conv_gn: slab addend / source on the generic path"
                                             : "run_conv_gn: slab addend on a path that cannot sum it");
    const float* bias = cw.has_bias ? c.P + cw.b : nullptr;
    const float *g = c.P + n.g, *b = c.P + n.b;
    float* gnp = c.W + c.ly.off_gn;
    switch (k.path) {
        case CG_GENERIC:
            DDK_TRY(run_conv(c, DDK_CONV3X3_S1, cw, src0, c0, src1, c1, nullptr, raw, H, W, N));
            return groupnorm_mish_generic(raw, g, b, temb, c.u.temb_total, addend, out, c.B, H * W, N, n.c_real, GROUPS, GN_EPS, c.st, c.temb_rows);
        case CG_LOCAL:
        case CG_WLOCAL:
            return (k.path == CG_LOCAL ? conv_gn_local : conv_gn_wlocal)(src0, c0, src1, c1, c.P + (k.path == CG_LOCAL ? cw.wl : cw.wwl), bias, g, b,
                       temb, c.u.temb_total, c.temb_rows, addend, out, c.B, H, W, N, GROUPS, GN_EPS, c.st, as, ss);
        case CG_FIRST:
            DDK_TRY(conv_first(c.x_first, c.P + cw.wf, bias, raw, nullptr, c.B, H, W, c.u.cfg.in_ch, N, GROUPS, nullptr, nullptr, c.st));
            break;
        case CG_CLUSTER:
        case CG_CLUSTER_SPLIT: {
            ++c.n_cluster;
            ddk_conv_args a = c.conv_args(DDK_CONV3X3_S1, cw, src0, c0, src1, c1, out, H, W, N);
            a.resid = addend;
            sk.put(a);
            WinoGnFuse f = c.gn_fuse(n, temb, c.temb_rows);
            if (k.path == CG_CLUSTER_SPLIT) f.pairs = reinterpret_cast<unsigned*>(c.W + c.ly.off_cl + cl_pair_offset(c.B));
            return conv_forward(a, c.st, nullptr, &f);
        }
        case CG_PARTS:
            DDK_TRY(run_conv_parts(c, cw, src0, c0, src1, c1, raw, H, W, N, sk));
            return groupnorm_mish_parts(raw, gnp, k.np, g, b, temb, c.u.temb_total, addend, out, c.B, H * W, N, GROUPS, GN_EPS, c.st, c.temb_rows);
        case CG_SLABS: {
            AddendSlabs sl;
            DDK_TRY(run_conv_slabs(c, DDK_CONV3X3_S1, cw, src0, c0, src1, c1, raw, H, W, N, k.splits, sl, sk));
            return groupnorm_mish_ex(c.W + c.ly.off_splitk, sl.n, sl.stride, sl.bias, g, b, temb, c.u.temb_total, addend, out, c.B, H * W, N,
                                     GROUPS, GN_EPS, nullptr, 0, c.st, c.temb_rows);
        }
        case CG_PLAIN:
            DDK_TRY(run_conv(c, DDK_CONV3X3_S1, cw, src0, c0, src1, c1, nullptr, raw, H, W, N, nullptr, nullptr, sk));
            break;
    }
    return groupnorm_mish(raw, g, b, temb, c.u.temb_total, addend, out, c.B, H * W, N, GROUPS, GN_EPS, gnp, c.ly.gn_ws * sizeof(float), c.st,
                          c.temb_rows);
}

// blocks.py:105-115 (eval): out = Mish(GN(conv2(Mish(GN(conv1(x))) + temb))) + res(x)
// ss.n > 1 (res_takes_slab_source only): src0 is the split-K slab area the stride-2 conv in front left; both its readers -- the first
// Block's staging loop and the second Block's residual -- sum the slabs (+ that conv's bias) in splitk_reduce_kernel's order
static bool res_takes_slab_source(const ddk_unet& u, const ResW& r, int B, int H, int W, int c0) {
    return !u.generic && !r.has_res && conv_gn_is_local(u, r.c1, B, H, W, c0, 0, r.co) && conv_gn_is_local(u, r.c2, B, H, W, r.co, 0, r.co);
}

// The skip fold (DDK_OPT_SKIP_FOLD): the block's first conv is a Winograd launch on the 64-channel tile, whichever of its GroupNorm
// forms it takes (in-launch, with or without the partner hand-off; partials; slabs; plain).  Shape and kernel decide, not whether this
// call may exchange in the launch: the sampler, ddk_unet_forward and a step loop over it run the same arithmetic.
static bool res_folds_skip(const Ctx& c, const ResW& r, const float* src0, int c0, const float* src1, int c1, int H, int W) {
    if (!r.has_res || !c.u.skip_fold || !r.res.has_wsk || c.u.generic || r.res.cin_pad != c0 + c1) return false;
    const ConvGnChoice k = classify_conv_gn(c.u, r.c1, c.B, H, W, c0, c1, r.co, c.x_first && src0 == c.x_padded && !src1, false, 0);
    return k.wino && (k.path == CG_PARTS || k.path == CG_SLABS || k.path == CG_PLAIN) && conv_wino_skip_ok(c.B, H, W, c0 + c1, r.co);
}

static int run_res(Ctx& c, const ResW& r, const float* src0, int c0, const float* src1, int c1, float* out, int H, int W,
                   const AddendSlabs& ss = AddendSlabs()) {
    float* raw = c.W + c.ly.off_raw;
    float* a1 = c.W + c.ly.off_a1;
    float* res = c.W + c.ly.off_res;
    // the 1x1 skip first: the second conv's split-K slabs and the skip conv's would otherwise share the workspace
    const float* addend = src0;
    AddendSlabs as;
    if (ss.n > 1) {
        if (r.has_res || src1) return fail_arg("run_res: slab source with a skip conv or a second source");
        as = ss;
    }
    SkipFold sk;
    if (res_folds_skip(c, r, src0, c0, src1, c1, H, W)) {
        sk.w = c.P + r.res.wsk; sk.b = r.res.has_bias ? c.P + r.res.b : nullptr; sk.out = res;
        // an image-local second Block sums an addend in slab form and leaves the split-K workspace alone: skip slabs can wait for it
        sk.want_slabs = conv_gn_is_local(c.u, r.c2, c.B, H, W, r.co, 0, r.co);
        addend = res;
    } else if (r.has_res) {
        const int rs = conv_splits(DDK_CONV1X1, c.B, H, W, c0 + c1, r.co);
        if (rs > 1 && !conv1x1_sm_ok((long long)c.B * H * W, c0, c1, r.co) && conv_gn_is_local(c.u, r.c1, c.B, H, W, c0, c1, r.co) &&
            conv_gn_is_local(c.u, r.c2, c.B, H, W, r.co, 0, r.co)) {
            // neither Block conv touches the split-K workspace on these maps: the skip conv leaves its slabs there and the
            // second Block's epilogue sums them (+ bias) while it adds the residual -- no reduce launch
            DDK_TRY(run_conv_slabs(c, DDK_CONV1X1, r.res, src0, c0, src1, c1, res, H, W, r.co, rs, as));
            addend = c.W + c.ly.off_splitk;
        } else {
            DDK_TRY(run_conv(c, DDK_CONV1X1, r.res, src0, c0, src1, c1, nullptr, res, H, W, r.co));
            addend = res;
        }
    }
    DDK_TRY(run_conv_gn(c, r.c1, src0, c0, src1, c1, raw, r.n1, c.temb + r.temb_off, nullptr, a1, H, W, r.co, AddendSlabs(), ss, sk));
    if (sk.left > 1) {
        const long long slab = (long long)c.B * H * W * r.co;
        as = AddendSlabs{sk.left, slab, sk.b};
        addend = c.W + c.ly.off_splitk + (long long)sk.left * slab;
    }
    return run_conv_gn(c, r.c2, a1, r.co, nullptr, 0, raw, r.n2, nullptr, addend, out, H, W, r.co, as);
}

// The folded form of the attention block (attention.hip, attn_fold_kernel): maps with many more pixels than channels, C = 128
static bool attn_fold_eligible(const ddk_unet& u, const AttnW& a, int B, int H, int W) {
    const long long M = (long long)B * H * W;
    return u.attn_fold && H * W > u.attn_fold_min_hw && (H * W) % 64 == 0 && attn_fold_ok(a.c, HEADS) && conv1x1_ws_ok(M, a.c, a.c) &&
           conv_ln_fold_ok(B, H, W, a.c, 2 * HIDDEN) && B <= 256;
}

// blocks.py:8-14,63-71,126-134: out = to_out(attn(to_qkv(LN(x)))) + x
static int run_attn(Ctx& c, const AttnW& a, const float* x, float* out, int H, int W) {
    float* xn = c.W + c.ly.off_xn;
    float* qkv = c.W + c.ly.off_qkv;
    float* ctx = c.W + c.ly.off_ctx;
    float* o = c.W + c.ly.off_o;
    const long long M = (long long)c.B * H * W;
    if (!c.u.generic && H * W <= 16 && a.c % 32 == 0 && linattn_small_qkv_ok(H * W, a.c)) {
        // 4x4 maps: projection (LayerNorm folded), context and apply of one (image, head) in one workgroup -- no qkv tensor,
        // 14.6 us instead of 11.0 + 5.2.  (On 8x8 maps the same kernel does 4x the work on the same 128 workgroups -- half the
        // chip, one wave per SIMD: 25.5 us against 12.5 + 5.7 for the two launches.  Those maps and the 16x16 ones take the
        // pixel-split launch below where the in-launch exchanges may run, and the im2col kernel + linattn_small_kernel elsewhere.)
        DDK_TRY(linattn_small_qkv(x, c.P + a.qkv_op, c.P + a.ln_c1, c.P + a.ln_c2, LN_EPS, ctx, o, c.B, H * W, a.c, HEADS, c.st));
        return run_conv(c, DDK_CONV1X1, a.out, o, HIDDEN, nullptr, 0, x, out, H, W, a.c);
    }
    if (!c.u.generic && attn_fold_eligible(c.u, a, c.B, H, W)) {
        // q is linear in this attention: project k and v only, build the context, fold to_out . ctx^T . W_q (and the LayerNorm)
        // into one C x C matrix per image and apply it to x as a per-image 1x1 conv with the residual -- no q third of to_qkv, no
        // apply kernel, no separate to_out
        float* A = o;                                   // [B][C][C], then a1, a2 [B][C] (the apply output buffer is free on this path)
        float* a1 = A + (size_t)c.B * a.c * a.c;
        float* a2 = a1 + (size_t)c.B * a.c;
        const float *wqg = c.P + a.qkv_lnw, *bout = a.out.has_bias ? c.P + a.out.b : nullptr;
        const ConvLnFold lnA{a1, a2, LN_EPS};
        if (c.u.attn_kvctx && attn_kvctx_ok(c.B, H * W, a.c, HEADS) && c.ly.splitk * sizeof(float) >= attn_kvctx_workspace_bytes(c.B, H * W)) {
            // round 5: projection and context in one launch -- the 33.5 MB kv tensor of the 32x32 level is never written
            const float *wkv = wqg + (size_t)HIDDEN * a.c, *c1kv = c.P + a.ln_c1 + HIDDEN, *c2kv = c.P + a.ln_c2 + HIDDEN;
            float* part = c.W + c.ly.off_splitk;
            const int splits = attn_kvctx_splits(c.B, H * W);
            if (c.u.attn_fold_parts && attn_fold_parts_ok(a.c, HEADS, splits)) {
                // the matrix straight from the split records, which stay in the workspace until this launch has read them
                DDK_TRY(attn_kvctx_parts(x, wkv, c1kv, c2kv, LN_EPS, c.B, H * W, part, c.ly.splitk * sizeof(float), c.st));
                DDK_TRY(attn_fold_parts(part, splits, wqg, c.P + a.ln_c1, c.P + a.ln_c2, c.P + a.out.w, bout, A, a1, a2, c.B, a.c, HEADS, c.st));
                return conv1x1_ws(x, A, nullptr, x, out, M, a.c, &lnA, c.st, c.B);
            }
            DDK_TRY(attn_kvctx(x, wkv, c1kv, c2kv, LN_EPS, ctx, c.B, H * W, part, c.ly.splitk * sizeof(float), c.st));
        } else {
            const ConvLnFold lnkv{c.P + a.ln_c1 + HIDDEN, c.P + a.ln_c2 + HIDDEN, LN_EPS};
            DDK_TRY(run_conv(c, DDK_CONV1X1, a.qkv, x, a.c, nullptr, 0, nullptr, qkv, H, W, 2 * HIDDEN, c.P + a.qkv_lnw + (size_t)HIDDEN * a.c,
                             &lnkv));
            // (round 4: merging the split context partials inside attn_fold_kernel instead of the 5.5 us merge launch made that kernel 13.0 ->
            //  25.6 us -- each of an image's four workgroups redoes the 4 x 8 partial reads, one memory latency per split -- so the merge
            //  launch stays on this diagnostic path)
            DDK_TRY(linattn_context(qkv, ctx, c.B, H * W, HEADS, c.W + c.ly.off_splitk, c.ly.splitk * sizeof(float), c.st, true));
        }
        DDK_TRY(attn_fold(ctx, wqg, c.P + a.ln_c1, c.P + a.ln_c2, c.P + a.out.w, bout, A, a1, a2, c.B, a.c, HEADS, c.st));
        return conv1x1_ws(x, A, nullptr, x, out, M, a.c, &lnA, c.st, c.B);
    }
    if (!c.u.generic && c.u.attn_split && c.allow_cluster && a.c >= 128 && attn_split_ok(c.B, H * W, a.c, HEADS)) {
        // 16x16 and 8x8 maps, up to batch 32: projection (LayerNorm folded) and core of one (image, head, half of the pixels) per
        // workgroup -- 8 B workgroups, no qkv tensor; the two halves exchange their context partials inside the launch.
        // (Measured at C = 128 and 256 only; narrower sites -- at most three K chunks -- keep the two launches.)
        float* cl = c.W + c.ly.off_cl;
        DDK_TRY(attn_split(x, c.P + a.qkv_lnw, c.P + a.ln_c1, c.P + a.ln_c2, LN_EPS, ctx, o, c.B, H * W, a.c,
                           reinterpret_cast<unsigned*>(cl + cl_attn_offset(c.B)), cl + cl_counter_floats(c.B), cl_words(cl, c.B).fail, c.st));
        return run_conv(c, DDK_CONV1X1, a.out, o, HIDDEN, nullptr, 0, x, out, H, W, a.c);
    }
    if (!c.u.generic && conv_ln_fold_ok(c.B, H, W, a.c, 3 * HIDDEN)) {
        // LayerNorm folded into the projection: no LayerNorm launch, no normalised copy of x
        const ConvLnFold ln{c.P + a.ln_c1, c.P + a.ln_c2, LN_EPS};
        DDK_TRY(run_conv(c, DDK_CONV1X1, a.qkv, x, a.c, nullptr, 0, nullptr, qkv, H, W, 3 * HIDDEN, c.P + a.qkv_lnw, &ln));
    } else {
        // (generic widths: LayerNorm over the real channels, then the plain projection over zero-padded weights)
        DDK_TRY(c.u.generic ? chan_layernorm_generic(x, c.P + a.ln.g, c.P + a.ln.b, xn, M, a.c, a.c_real, LN_EPS, c.st)
                            : chan_layernorm(x, c.P + a.ln.g, c.P + a.ln.b, xn, M, a.c, LN_EPS, c.st));
        DDK_TRY(run_conv(c, DDK_CONV1X1, a.qkv, xn, a.c, nullptr, 0, nullptr, qkv, H, W, 3 * HIDDEN));
    }
    if (H * W <= 256) {      // 16x16 and smaller: k, v, q of one (image, head) fit the LDS -- context, merge and apply in one launch
                             // (256 rows: both products on the matrix pipe; the VALU form was LDS-bound there, 23 us)
        DDK_TRY(linattn_fused_small(qkv, ctx, o, c.B, H * W, HEADS, c.st));
    } else {
        // (folding the split context's merge into the apply kernel's fragment build was tried: 73 vs 11 + 5.5 us at 32x32 --
        //  hundreds of dependent L2 loads per lane; the 5 us merge launch stays)
        DDK_TRY(linattn_context(qkv, ctx, c.B, H * W, HEADS, c.W + c.ly.off_splitk, c.ly.splitk * sizeof(float), c.st));
        DDK_TRY(linattn_apply(qkv, ctx, o, c.B, H * W, HEADS, c.st));
    }
    return run_conv(c, DDK_CONV1X1, a.out, o, HIDDEN, nullptr, 0, x, out, H, W, a.c);
}

// Levels as persistent launches (level_chain.hip; unet.py:83-101).  part 0: the last level whole -- downs[-1], mid, ups[0] -- on 4x4 maps:
// `in` = the Downsample conv's output, `skip` receives the level's skip tensor (unet.py:87), `out` the up attention block's output.
// part 1: downs[-2] on 8x8 maps (in -> skip).  part 2: ups[1] on 8x8 maps (cat(in, skip) -> out).
// bit of ddk_unet::level_chain: 1 = part 0, 2 = part 1, 4 = part 2
static bool level_chain_use(const Ctx& c, int H0, int W0, int bit) {
    return c.allow_cluster && (c.u.level_chain & bit) && c.B <= c.u.level_chain_max_batch && c.ly.chain > 0 &&
           (bit == 1 ? level_chain_shape_ok(c.u, H0, W0) : level8_chain_shape_ok(c.u, H0, W0)) && level_chain_device_ok();
}

// down_src != null (part 0): `in` is not used -- the chain starts with the Downsample conv on the 8x8 map down_src (blocks.py:41-47);
// up_out != null (part 0): the chain ends with the Upsample transpose conv (blocks.py:32-38) into the 8x8 map up_out, `out` is not used
static int run_level_chain(Ctx& c, int part, const float* in, float* skip, float* out, const float* down_src = nullptr, float* up_out = nullptr) {
    const ddk_unet& u = c.u;
    const int hw = part == 0 ? 16 : 64;
    const bool wino = hw == 64;
    ChainParams p{};
    int n = 0, e = 0;
    const size_t per = (size_t)c.B * hw * 256;
    auto buf = [&](int i) { return c.W + c.ly.off_chain + (size_t)i * per; };
    auto conv3 = [&](const ConvW& cw, const NormW& nw, const float* s0, int c0, const float* s1, int c1, int temb_off, int flags, float* o) {
        ChainOp& op = p.op[n++];
        op = ChainOp{s0, s1, c.P + (wino ? cw.wwl : cw.wl), c.P + cw.b, c.P + nw.g, c.P + nw.b, o, c0, c1, CH_CONV3, flags, temb_off, 256};
    };
    auto conv1 = [&](const ConvW& cw, const float* s0, int c0, const float* s1, int c1, int flags, float* o) {
        ChainOp& op = p.op[n++];
        op = ChainOp{s0, s1, c.P + cw.wl1, c.P + cw.b, nullptr, nullptr, o, c0, c1, CH_CONV1, flags, -1, 256};
    };
    auto attn = [&](const AttnW& a, const float* s0, float* o) {
        ChainOp& op = p.op[n++];
        op = ChainOp{s0, nullptr, c.P + a.qkv_op, nullptr, c.P + a.ln_c1, c.P + a.ln_c2, o, a.c, 0, CH_ATTN, CHF_WAIT | CHF_SIGNAL, -1, HIDDEN};
    };
    const int WS = CHF_WAIT | CHF_SIGNAL, RES = CHF_ADD_KEEP | CHF_SAVE_KEEP;
    // a ResnetBlock without a skip conv (blocks.py:105-115): x enters as `keep`
    auto res_plain = [&](const ResW& r, const float* x, bool external, float* o) {
        float* h = buf(e++);
        conv3(r.c1, r.n1, x, 256, nullptr, 0, r.temb_off, external ? (CHF_SIGNAL | CHF_KEEP_FROM_SRC) : WS, h);
        conv3(r.c2, r.n2, h, 256, nullptr, 0, -1, WS | RES, o);
    };
    // Residual(PreNorm(LinearAttention)) (blocks.py:8-14, 63-71, 116-134): x is `keep`
    auto attn_block = [&](const AttnW& a, const float* x, float* o, bool signals) {
        float* heads = buf(e++);
        attn(a, x, heads);
        conv1(a.out, heads, HIDDEN, nullptr, 0, (signals ? WS : CHF_WAIT) | RES, o);
    };
    // a ResnetBlock on cat(x, skip) -> 512 channels, res_conv is a 1x1 (its result lives in keep2); x_external: x comes from another kernel
    auto res_cat = [&](const ResW& r, const float* x, bool x_external, const float* sk, float* o) {
        conv1(r.res, x, 256, sk, 256, (x_external ? 0 : CHF_WAIT) | CHF_SAVE_KEEP2 | CHF_NO_OUT, nullptr);
        float* h = buf(e++);
        conv3(r.c1, r.n1, x, 256, sk, 256, r.temb_off, CHF_SIGNAL, h);
        conv3(r.c2, r.n2, h, 256, nullptr, 0, -1, WS | CHF_ADD_KEEP2 | CHF_SAVE_KEEP, o);
    };
    if (part == 0) {
        const int sh = u.L - 1;
        if (down_src) {
            const ConvW& dc = u.down_conv[sh - 1];
            float* dn = buf(e++);
            ChainOp& op = p.op[n++];
            op = ChainOp{down_src, nullptr, c.P + dc.wl, c.P + dc.b, nullptr, nullptr, dn, 256, 0, CH_CONV3,
                         CHF_DOWN | CHF_NO_GN | CHF_SIGNAL | CHF_SAVE_KEEP, -1, 256};
            in = dn;
        }
        float* d0 = buf(e++);
        res_plain(u.down_res[2 * sh], in, down_src == nullptr, d0);
        float* d1 = buf(e++);
        res_plain(u.down_res[2 * sh + 1], d0, false, d1);
        attn_block(u.down_attn[sh], d1, skip, true);
        float* m1 = buf(e++);
        res_plain(u.mid1, skip, false, m1);
        float* ma = buf(e++);
        attn_block(u.mid_attn, m1, ma, true);
        float* m2 = buf(e++);
        res_plain(u.mid2, ma, false, m2);
        float* u0 = buf(e++);
        res_cat(u.up_res[0], m2, false, skip, u0);
        float* u1 = buf(e++);
        res_plain(u.up_res[1], u0, false, u1);
        if (up_out) {
            float* ua = buf(e++);
            attn_block(u.up_attn[0], u1, ua, true);
            const ConvW& uc = u.up_conv[0];
            ChainOp& op = p.op[n++];
            op = ChainOp{ua, nullptr, c.P + uc.wtl, c.P + uc.b, nullptr, nullptr, up_out, 256, 0, CH_UPT, CHF_WAIT, -1, 256};
        } else {
            attn_block(u.up_attn[0], u1, out, false);
        }
    } else if (part == 1) {
        const int sh = u.L - 2;
        float* d0 = buf(e++);
        res_plain(u.down_res[2 * sh], in, true, d0);
        float* d1 = buf(e++);
        res_plain(u.down_res[2 * sh + 1], d0, false, d1);
        attn_block(u.down_attn[sh], d1, skip, false);
    } else {
        float* u0 = buf(e++);
        res_cat(u.up_res[2], in, true, skip, u0);
        float* u1 = buf(e++);
        res_plain(u.up_res[3], u0, false, u1);
        attn_block(u.up_attn[1], u1, out, false);
    }
    if (n > CH_MAX_OPS || e > (part == 0 ? CHAIN_BUFS : CHAIN8_BUFS)) return fail_arg("level_chain: internal op / buffer count");
    p.n_ops = n;
    p.B = c.B;
    p.hw = hw;
    p.temb = c.temb;
    p.temb_rows = c.temb_rows;
    p.temb_stride = u.temb_total;
    float* cl = c.W + c.ly.off_cl;
    p.cnt = reinterpret_cast<unsigned*>(cl + cl_chain_offset(c.B));
    p.done = p.cnt + (size_t)c.B * 32;
    p.fail = cl_words(cl, c.B).fail;
    p.gn_eps = GN_EPS;
    p.ln_eps = LN_EPS;
    return level_chain_launch(p, c.st);
}

// What a reverse step of the sampler adds to a forward: the bookkeeping in front (t_cur[b] <- counter; counter -= 1) and the
// update of x behind it (ddpm.py:203-227).  Both ride on the forward's own first / last kernel where the shape allows.
struct StepArgs {
    int64_t* state;               // [0] step counter, [1] Philox seed, [2] stream id
    float* eps_hat;               // scratch for the unfused tail
    long long per;
    StepRule rule;                // how the step ends (never StepKind::Eps; Vlb: the forward ran on rule.vlb->xt)
};

// tiles of the final tail when the end of the forward runs as ONE launch (final_tail_kernel), else 0.  cin = the final conv's
// input channels (dimp[1]).  The Vlb, Multistep, Inpaint, Restore, RestoreMasked, RestoreMultistep, RestoreNoisy and RestoreGray kinds take
// a subset of the shapes (final_tail_ok; the last five's depends on its block, restore_n).
static int fused_tail_parts(const ddk_unet& u, int B, int H, int W, int cin, StepKind kind, int restore_n = 0) {
    const int chan = u.generic ? pad32(u.cfg.chan) : u.cfg.chan, n_out = u.cfg.in_ch;
    const int npf = u.final_conv.has_wu ? conv_wino_stats_parts(B, H, W, cin, chan, GROUPS) : 0;
    if (npf <= 0 || (restore_kind(kind) && !u.restore_fused)) return 0;
    return final_tail_ok(H * W, chan, GROUPS, n_out, npf, kind, W, restore_n) ? npf : 0;
}

// t_cur[b] = counter for every sample, then counter -= 1; also zero-pads x into xpad.  First kernel of a step on shapes the
// first-layer kernel does not take: the previous step's kernels have all completed (stream order), nobody else reads the counter.
__global__ __launch_bounds__(256) void step_prepare_kernel(const float* __restrict__ x, float* __restrict__ xpad, long long total,
                                                           int C, int c_pad, int64_t* __restrict__ counter,
                                                           int64_t* __restrict__ t_cur, int B) {
    if (blockIdx.x == 0) {
        const int64_t v = *counter;
        for (int b = threadIdx.x; b < B; b += blockDim.x) t_cur[b] = v;
        __syncthreads();
        if (threadIdx.x == 0) *counter = v - 1;
    }
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % c_pad);
        const long long m = i / c_pad;
        xpad[i] = ch < C ? x[m * C + ch] : 0.f;
    }
}

// The first ResnetBlock on the unpadded input: conv_first.hip for its first conv, and its 1x1 res_conv evaluated inside the
// second GroupNorm launch (norm_act.hip, Res1x1) -- no pad kernel, no padded 32-channel conv, no res_conv launch.  Needs the
// second conv to leave GroupNorm partials (one-pass Winograd shape).
static bool first_fast(const ddk_unet& u, int B, int H, int W) {
    const ResW& r = u.down_res[0];
    if (!r.c1.has_wf || !r.has_res || !r.c2.has_wu) return false;
    if (!conv_first_ok(r.ci, r.co, H, W, GROUPS)) return false;
    const int upr = r.co / 4;
    if (upr > 256 || 256 % upr) return false;
    if ((long long)H * W / 128 * GROUPS > 1024) return false;
    return conv_wino_stats_parts(B, H, W, r.co, r.co, GROUPS) > 0;
}

// ... as launches, x the unpadded input.  fused: the first GroupNorm + Mish + shift inside conv_first's launch (the image's 8 tiles exchange
// their statistics: no raw tensor, no GroupNorm-apply launch).  counter / t_cur (sampler): the step's bookkeeping rides on the first kernel.
static int run_first_res(Ctx& c, const float* x, bool fused, int64_t* counter, int64_t* t_cur, float* out, int H, int W) {
    const ResW& r = c.u.down_res[0];
    const float* P = c.P;
    float* raw = c.W + c.ly.off_raw;
    float* a1 = c.W + c.ly.off_a1;
    float* gnp = c.W + c.ly.off_gn;
    const float* bias1 = r.c1.has_bias ? P + r.c1.b : nullptr;
    const float* res_b = r.res.has_bias ? P + r.res.b : nullptr;
    if (fused) {
        const WinoGnFuse f = c.gn_fuse(r.n1, c.temb + r.temb_off, c.temb_rows);
        DDK_TRY(conv_first_gn(x, P + r.c1.wf, bias1, f.gamma, f.beta, f.temb, f.temb_stride, f.temb_rows, f.eps, a1, c.B, H, W, r.ci, r.co,
                              f.groups, f.records, f.counters, f.fail, counter, t_cur, c.st));
    } else {
        DDK_TRY(conv_first(x, P + r.c1.wf, bias1, raw, gnp, c.B, H, W, r.ci, r.co, GROUPS, counter, t_cur, c.st));
        DDK_TRY(groupnorm_mish_parts(raw, gnp, H * W / 128, P + r.n1.g, P + r.n1.b, c.temb + r.temb_off, c.u.temb_total, nullptr, a1, c.B,
                                     H * W, r.co, GROUPS, GN_EPS, c.st, c.temb_rows));
    }
    const int cl_np = c.allow_cluster && conv_wino_cluster_device_ok() && r.ci <= 8 ? conv_wino_cluster_np(c.B, H, W, r.co, r.co, GROUPS) : 0;
    if (cl_np > 0 && cl_np <= c.u.cluster_np_max && conv_wino_variant_new(c.B, H, W, r.co) && c.n_cluster < c.u.cluster_limit) {
        // GroupNorm + Mish + the 1x1 res_conv of the input finished in the second conv's own launch (in-launch exchange of the tile
        // statistics; the epilogue evaluates the <= 8-channel 1x1 itself): no raw tensor, no GroupNorm-apply launch
        ++c.n_cluster;                // (counted as in run_conv_gn: see classify_conv_gn)
        const ddk_conv_args a = c.conv_args(DDK_CONV3X3_S1, r.c2, a1, r.co, nullptr, 0, out, H, W, r.co);
        WinoGnFuse f = c.gn_fuse(r.n2, nullptr, nullptr);
        f.res_x = x; f.res_w = P + r.res.w; f.res_b = res_b; f.res_cin = r.ci; f.res_ld = r.res.cin_pad;
        return conv_forward(a, c.st, nullptr, &f);
    }
    DDK_TRY(run_conv_parts(c, r.c2, a1, r.co, nullptr, 0, raw, H, W, r.co));
    return groupnorm_mish_parts(raw, gnp, conv_wino_stats_parts(c.B, H, W, r.co, r.co, GROUPS), P + r.n2.g, P + r.n2.b, nullptr, c.u.temb_total,
                                nullptr, out, c.B, H * W, r.co, GROUPS, GN_EPS, c.st, nullptr, x, P + r.res.w, res_b, r.ci, r.res.cin_pad);
}

// x: NHWC input, unpadded ([B][H0][W0][in_ch]).
// temb_table != nullptr (sampler): the per-block time shifts of EVERY timestep were computed once up front
// (build_temb_table); row t[b] of the table is read directly by the GroupNorm kernels and no time kernel runs per step.
// step != nullptr (sampler): t is the t_cur array the step's first kernel fills from step->state, and the forward ends with
// the update of step->x instead of writing eps_hat to `out`.
static int forward_core(const ddk_unet& u, const float* P, const float* x, int64_t* t, float* out, int B, int H0, int W0,
                        float* ws, const Layout& ly, hipStream_t st, bool allow_cluster, const float* temb_table = nullptr,
                        const StepArgs* step = nullptr) {
    float* tact = ws + ly.off_tact;
    float* temb = ws + ly.off_temb;
    float* xpad = ws + ly.off_xpad;
    const bool fast0 = first_fast(u, B, H0, W0);
    if (!fast0) {
        const int C = u.cfg.in_ch, cp = pad32(C);
        const long long padded = (long long)B * H0 * W0 * cp;
        if (step) {
            const int prep_blocks = (int)(ceil_div(padded, 256) < 1024 ? ceil_div(padded, 256) : 1024);
            hipLaunchKernelGGL(step_prepare_kernel, dim3(prep_blocks), dim3(256), 0, st, x, xpad, padded, C, cp, step->state, t, B);
            DDK_TRY(check_launch("step_prepare_kernel"));
        } else {
            DDK_TRY(ddk_pad_channels(x, xpad, (long long)B * H0 * W0, C, cp, st));
        }
    }
    if (!temb_table) {
        DDK_TRY(time_mlp(t, P + u.freqs, P + u.w1t, P + u.b1, P + u.w2t, P + u.b2, tact, nullptr, B, u.time_dim, st));
        DDK_TRY(time_proj(tact, P + u.temb_wt, P + u.temb_bias, temb, B, u.time_dim, u.temb_total, st));
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "timestep rows are read as long long");
    Ctx c{u, P, ws, ly, B, st, temb_table ? temb_table : temb, temb_table ? reinterpret_cast<const long long*>(t) : nullptr};
    if (!fast0) { c.x_first = x; c.x_padded = xpad; }
    c.allow_cluster = allow_cluster;
    float* bufA = ws + ly.off_A;
    float* bufB = ws + ly.off_B;
    float* bufC = ws + ly.off_C;
    float* raw = ws + ly.off_raw;
    float* a1 = ws + ly.off_a1;
    float* gnp = ws + ly.off_gn;

    int H = H0, W = W0;
    const float* cur = xpad;
    int cur_c = pad32(u.cfg.in_ch);
    AddendSlabs cur_ss;           // > 1 slab: `cur` is the split-K area a Downsample conv left for the next ResnetBlock to sum
    // the first Block with its GroupNorm in the conv's launch: in the sampler that kernel leaves the step counter alone (every workgroup of
    // it reads the counter) and the step's LAST kernel decrements it (dec_counter below)
    const bool first_fused = fast0 && c.allow_cluster && u.first_gn && conv_wino_cluster_device_ok() &&
                             conv_first_gn_ok(u.down_res[0].ci, u.down_res[0].co, H0, W0, GROUPS) && u.cluster_limit > 0;
    int64_t* dec_counter = (first_fused && step) ? step->state : nullptr;
    const bool chained = level_chain_use(c, H0, W0, 1); // the last level (4x4 maps) as one persistent launch
    const bool chain_edges = chained && (u.level_chain & 8) && u.L >= 2 && u.down_conv[u.L - 2].has_wl && u.down_conv[u.L - 2].has_bias &&
                             u.up_conv[0].has_wtl && u.up_conv[0].cin == 256 && u.down_conv[u.L - 2].cin == 256;
    const bool chained8 = level_chain_use(c, H0, W0, 2);   // the level above it (8x8 maps): downs[-2] as one launch,
    const bool chained8u = level_chain_use(c, H0, W0, 4);  // ups[1] as another
    for (int l = 0; l < u.L; ++l) {
        float* skip = ws + ly.off_skip[l];
        const int co = u.dimp[l + 1];
        if (chained && l == u.L - 1) {
            // downs[-1] (2 ResnetBlocks + attention), mid_block1, mid_attn, mid_block2, ups[0] (2 ResnetBlocks + attention): 19 launches in one;
            // with the Downsample conv in front and the Upsample transpose conv behind (chain_edges): 23 in one
            DDK_TRY(run_level_chain(c, 0, cur, skip, bufB, chain_edges ? ws + ly.off_skip[l - 1] : nullptr, chain_edges ? bufA : nullptr));
            cur_c = co;
            break;
        }
        const bool level_chained = chained8 && l == u.L - 2 && cur_ss.n == 1;
        if (level_chained) {
            // downs[-2] on 8x8 maps (2 ResnetBlocks + attention): 7 launches in one
            DDK_TRY(run_level_chain(c, 1, cur, skip, nullptr));
        } else if (l == 0 && fast0) {
            DDK_TRY(run_first_res(c, x, first_fused, step ? step->state : nullptr, step ? t : nullptr, bufB, H, W));
        } else {
            DDK_TRY(run_res(c, u.down_res[2 * l], cur, cur_c, nullptr, 0, bufB, H, W, cur_ss));
            cur_ss = AddendSlabs();
        }
        if (!level_chained) {
            DDK_TRY(run_res(c, u.down_res[2 * l + 1], bufB, co, nullptr, 0, bufC, H, W));
            DDK_TRY(run_attn(c, u.down_attn[l], bufC, skip, H, W));
        }
        if (l < u.L - 1 && chain_edges && l + 1 == u.L - 1) {
            H /= 2; W /= 2;               // the level chain runs this Downsample conv itself, from `skip`
            cur = skip;
        } else if (l < u.L - 1) {
            const int s2 = conv_splits(DDK_CONV3X3_S2, B, H, W, co, co);
            if (u.fold_down_reduce && s2 > 1 && !(chained && l + 1 == u.L - 1) && !(chained8 && l + 1 == u.L - 2) &&
                res_takes_slab_source(u, u.down_res[2 * l + 2], B, H / 2, W / 2, co)) {
                // the Downsample conv splits k and the ResnetBlock behind it is image-local (8x8 / 4x4 maps, no skip conv): the conv leaves
                // its slabs in the split-K area and that block's two readers sum them -- no reduce launch, no reduced tensor
                DDK_TRY(run_conv_slabs(c, DDK_CONV3X3_S2, u.down_conv[l], skip, co, nullptr, 0, bufA, H, W, co, s2, cur_ss));
                H /= 2; W /= 2;
                cur = ws + ly.off_splitk;
            } else {
                DDK_TRY(run_conv(c, DDK_CONV3X3_S2, u.down_conv[l], skip, co, nullptr, 0, nullptr, bufA, H, W, co));
                H /= 2; W /= 2;
                cur = bufA;
            }
        } else {
            cur = skip;
        }
        cur_c = co;
    }
    if (!chained) {
        DDK_TRY(run_res(c, u.mid1, cur, cur_c, nullptr, 0, bufB, H, W));
        DDK_TRY(run_attn(c, u.mid_attn, bufB, bufC, H, W));
        DDK_TRY(run_res(c, u.mid2, bufC, cur_c, nullptr, 0, bufA, H, W));
        cur = bufA;
    }
    for (int i = 0; i < u.L - 1; ++i) {
        const int lvl = u.L - 1 - i;  // skips.pop(): the most recent skip first (unet.py:97)
        const float* skip = ws + ly.off_skip[lvl];
        const int dout = u.dimp[lvl + 1], din = u.dimp[lvl];
        if (chained8u && i == 1) {
            // ups[1] on 8x8 maps (ResnetBlock on the concat, ResnetBlock, attention): 9 launches in one
            DDK_TRY(run_level_chain(c, 2, cur, const_cast<float*>(skip), bufB));
        } else if (!(chained && i == 0)) {
            DDK_TRY(run_res(c, u.up_res[2 * i], cur, cur_c, skip, dout, bufB, H, W));
            DDK_TRY(run_res(c, u.up_res[2 * i + 1], bufB, din, nullptr, 0, bufC, H, W));
            DDK_TRY(run_attn(c, u.up_attn[i], bufC, bufB, H, W));
        }
        if (!(chain_edges && i == 0))     // (the level chain has written this transpose conv's output into bufA itself)
            DDK_TRY(run_conv(c, DDK_CONVT4X4_S2, u.up_conv[i], bufB, din, nullptr, 0, nullptr, bufA, H, W, din));
        H *= 2; W *= 2;
        cur = bufA;
        cur_c = din;
    }
    // final_conv: Block(dim, dim) then 1x1 to in_ch (unet.py:69-72)
    const int chan = u.generic ? pad32(u.cfg.chan) : u.cfg.chan, n_out = u.cfg.in_ch;
    StepRule plain{};             // a lone forward: eps_hat to `out`, no chain
    plain.kind = StepKind::Eps;
    plain.eps_out = out;
    const StepRule& rule = step ? step->rule : plain;
    ChainHooks hooks{};           // a chain keeps its Philox key in its state; a lone forward draws nothing
    if (step) {
        hooks.chain_state = step->state;
        hooks.dec_counter = dec_counter;
    }
    const int npf = fused_tail_parts(u, B, H, W, cur_c, rule.kind, rule.rst.n);
    // a Restore step whose blocks do not fit the tail's tile (or with its fused tail switched off) still ends the forward in the plain
    // tail's one launch, eps_hat to the step's scratch, and updates x behind it: the same eps_hat, bit for bit, as its fused tail sees
    // (the masked, the restore multistep and the noisy kind likewise)
    const int npe = (npf == 0 && step && restore_kind(rule.kind)) ? fused_tail_parts(u, B, H, W, cur_c, StepKind::Eps) : 0;
    if ((npf > 0 || npe > 0) && (!step || step->per == (long long)H * W * n_out)) {
        // one-pass Winograd conv with statistics, then GroupNorm + Mish + projection (+ the rule) in ONE launch
        DDK_TRY(run_conv_parts(c, u.final_conv, cur, cur_c, nullptr, 0, raw, H, W, chan));
        const TailIn in{raw, gnp, npf > 0 ? npf : npe, P + u.final_norm.g, P + u.final_norm.b, GN_EPS, P + u.final_w, P + u.final_b, n_out, B, H * W, chan, GROUPS};
        if (npf > 0) return final_tail(in, rule, t, hooks, st);
        StepRule eps_only{};
        eps_only.kind = StepKind::Eps;
        eps_only.eps_out = step->eps_hat;
        DDK_TRY(final_tail(in, eps_only, t, ChainHooks{}, st));
        return p_update(rule, step->eps_hat, t, B, step->per, hooks, st);
    }
    DDK_TRY(run_conv_gn(c, u.final_conv, cur, cur_c, nullptr, 0, raw, u.final_norm, nullptr, nullptr, a1, H, W, chan));
    float* eps_hat = step ? step->eps_hat : out;
    DDK_TRY(conv1x1_small_n(a1, P + u.final_w, P + u.final_b, eps_hat, (long long)B * H * W, chan, n_out, st));
    return step ? p_update(rule, eps_hat, t, B, step->per, hooks, st) : DDK_OK;
}

static int check_shape(const ddk_unet* u, int B, int H, int W) {
    DDK_REQUIRE(u, "unet: null plan");
    DDK_REQUIRE(B > 0 && H > 0 && W > 0, "unet: B/H/W must be positive");
    const int f = 1 << (u->L - 1);
    if (H % f || W % f) {
        set_error("unet: spatial size %dx%d must be divisible by %d (%d stride-2 stages, unet.py:43-50)", H, W, f, u->L - 1);
        return DDK_ERR_ARG;
    }
    return DDK_OK;
}

// sampler bookkeeping kernels ----------------------------------------------------------------------
// per-chain state the captured step reads from memory: [0] step counter, [1] Philox seed, [2] Philox stream id
__global__ void set_chain_state_kernel(int64_t* state, int64_t t_start, uint64_t seed, uint32_t stream_id) {
    state[0] = t_start;
    state[1] = (int64_t)seed;
    state[2] = (int64_t)stream_id;
}

}  // namespace ddk

extern "C" size_t ddk_unet_workspace_bytes(const ddk_unet* u, int B, int H, int W) {
    if (check_shape(u, B, H, W) != DDK_OK) return 0;
    return make_layout(*u, B, H, W).total * sizeof(float);
}

extern "C" int ddk_unet_forward(const ddk_unet* u, const void* packed, const float* x, const int64_t* t, float* out, int B, int H,
                                int W, void* workspace, size_t workspace_bytes, ddk_stream_t s) {
    DDK_TRY(check_shape(u, B, H, W));
    DDK_REQUIRE(packed && x && t && out && workspace, "unet_forward: null pointer");
    DDK_REQUIRE(aligned16(packed) && aligned16(workspace) && aligned16(x) && aligned16(out), "unet_forward: alignment");
    const Layout ly = make_layout(*u, B, H, W);
    if (workspace_bytes < ly.total * sizeof(float)) {
        set_error("unet_forward: workspace too small (%zu < %zu)", workspace_bytes, ly.total * sizeof(float));
        return DDK_ERR_WORKSPACE;
    }
    float* ws = static_cast<float*>(workspace);
    DDK_TRY(ensure_device_init());
    // the cluster GroupNorm's arrival / departure counters start at zero (they re-arm themselves after every launch)
    DDK_HIP(hipMemsetAsync(ws + ly.off_cl, 0, cl_counter_floats(B) * sizeof(float), as_stream(s)));
    return forward_core(*u, static_cast<const float*>(packed), x, const_cast<int64_t*>(t), out, B, H, W, ws, ly, as_stream(s),
                        u->cluster_gn >= 2);
}

/* The in-launch GroupNorm's workgroups wait for each other; when the device could not host a whole cluster at once (a foreign
 * kernel, a CU mask the library could not see) a wait times out after 20 ms, the tile is written as NaN and the workspace's
 * sticky counter moves.  This call waits for `s`, reads and clears that counter: DDK_ERR_CLUSTER means the tensors produced on
 * `workspace` since the last check are not to be used -- rerun with DDK_OPT_CLUSTER_GROUPNORM = 0. */
extern "C" int ddk_unet_cluster_check(const ddk_unet* u, void* workspace, int B, int H, int W, ddk_stream_t s) {
    DDK_TRY(check_shape(u, B, H, W));
    DDK_REQUIRE(workspace, "unet_cluster_check: null workspace");
    const Layout ly = make_layout(*u, B, H, W);
    return cluster_fail_check(cl_words(static_cast<float*>(workspace) + ly.off_cl, B).fail, as_stream(s), "in-launch GroupNorm",
                              " (the GPU is shared, masked or partitioned); results on this workspace are invalid -- rerun with "
                              "DDK_OPT_CLUSTER_GROUPNORM = 0");
}

extern "C" double ddk_unet_flops(const ddk_unet* u, int B, int H0, int W0) {
    if (check_shape(u, B, H0, W0) != DDK_OK) return 0;
    double f = 0;
    auto res = [&](const ResW& r, int H, int W) {
        f += conv_flops(DDK_CONV3X3_S1, B, H, W, r.ci_real, r.co_real) + conv_flops(DDK_CONV3X3_S1, B, H, W, r.co_real, r.co_real);
        if (r.has_res) f += conv_flops(DDK_CONV1X1, B, H, W, r.ci_real, r.co_real);
        f += 2.0 * B * u->time_dim * r.co_real;  // mlp Linear
    };
    auto attn = [&](const AttnW& a, int H, int W) {
        f += conv_flops(DDK_CONV1X1, B, H, W, a.c_real, 3 * HIDDEN) + conv_flops(DDK_CONV1X1, B, H, W, HIDDEN, a.c_real);
        f += 2.0 * 2.0 * B * HEADS * 32.0 * 32.0 * H * W;  // the two einsums
    };
    int H = H0, W = W0;
    f += 2.0 * B * (u->time_dim * 4.0 * u->time_dim) * 2;  // time_mlp Linears
    for (int l = 0; l < u->L; ++l) {
        res(u->down_res[2 * l], H, W); res(u->down_res[2 * l + 1], H, W); attn(u->down_attn[l], H, W);
        if (l < u->L - 1) { f += conv_flops(DDK_CONV3X3_S2, B, H, W, u->dims[l + 1], u->dims[l + 1]); H /= 2; W /= 2; }
    }
    res(u->mid1, H, W); attn(u->mid_attn, H, W); res(u->mid2, H, W);
    for (int i = 0; i < u->L - 1; ++i) {
        res(u->up_res[2 * i], H, W); res(u->up_res[2 * i + 1], H, W); attn(u->up_attn[i], H, W);
        f += conv_flops(DDK_CONVT4X4_S2, B, H, W, u->up_conv[i].cin, u->up_conv[i].cout);
        H *= 2; W *= 2;
    }
    f += conv_flops(DDK_CONV3X3_S1, B, H, W, u->cfg.chan, u->cfg.chan) + conv_flops(DDK_CONV1X1, B, H, W, u->cfg.chan, u->cfg.in_ch);
    return f;
}

// MFMA / FMA FLOPs the plan's kernels really issue for one forward: the same walk as ddk_unet_flops, but every 3x3 stride-1
// conv is priced by the kernel the plan dispatches it to -- Winograd F(2x2,3x3) forms issue 16 multiplies per 2x2 output tile
// instead of 36 (conv_wino.hip, conv3x3_gn_wlocal_kernel), m tiles are padded to 32 tiles, input channels to 32 -- so that
// executed / time / peak is a fraction of the matrix pipe's peak (<= 1 by construction).
extern "C" double ddk_unet_flops_executed(const ddk_unet* u, int B, int H0, int W0) {
    if (check_shape(u, B, H0, W0) != DDK_OK) return 0;
    double f = 0;
    auto conv3 = [&](const ConvW& cw, int H, int W, int c0, int c1, int N) {
        // by the path run_conv_gn takes (the cluster paths are Winograd launches like the ones they replace: same price)
        const ConvGnChoice k = classify_conv_gn(*u, cw, B, H, W, c0, c1, N, false, false, 0);
        const int cin = c0 + c1;
        if (k.path == CG_WLOCAL) return 2.0 * B * (H * W / 4) * 16.0 * cin * N;
        if (k.wino) return 2.0 * (double)(ceil_div((long long)B * (H / 2) * (W / 2), 32) * 32) * 16.0 * cin * N;
        return 2.0 * B * H * W * 9.0 * cin * N;
    };
    auto res = [&](const ResW& r, int H, int W, int c0, int c1, bool fast) {
        if (fast) {
            f += 2.0 * B * H * W * (2.0 * ((9 * r.ci + 1) / 2)) * r.co;        // conv_first: K = 9 * C_in rounded up to even
            f += 2.0 * B * H * W * (double)r.ci * r.co;                        // res_conv inside the GroupNorm launch (FMA)
        } else {
            f += conv3(r.c1, H, W, c0, c1, r.co);
            if (r.has_res) f += conv_flops(DDK_CONV1X1, B, H, W, c0 + c1, r.co);
        }
        f += conv3(r.c2, H, W, r.co, 0, r.co);
    };
    auto attn = [&](const AttnW& a, int H, int W) {
        if (attn_fold_eligible(*u, a, B, H, W)) {
            // k, v projection + context + the per-image fold (T four times per image, or P once from the split records; A once) + the
            // per-image C x C conv
            const bool parts = u->attn_kvctx && u->attn_fold_parts && attn_kvctx_ok(B, H * W, a.c, HEADS) &&
                               attn_fold_parts_ok(a.c, HEADS, attn_kvctx_splits(B, H * W));
            f += conv_flops(DDK_CONV1X1, B, H, W, a.c, 2 * HIDDEN) + 2.0 * B * HEADS * 32.0 * 32.0 * H * W;
            f += 2.0 * B * ((parts ? 1.0 : 4.0) * HIDDEN * 32.0 * a.c + (double)a.c * HIDDEN * a.c) + conv_flops(DDK_CONV1X1, B, H, W, a.c, a.c);
            return;
        }
        f += conv_flops(DDK_CONV1X1, B, H, W, a.c, 3 * HIDDEN) + conv_flops(DDK_CONV1X1, B, H, W, HIDDEN, a.c);
        f += 2.0 * 2.0 * B * HEADS * 32.0 * 32.0 * H * W;
    };
    int H = H0, W = W0, cur_c = pad32(u->cfg.in_ch);
    for (int l = 0; l < u->L; ++l) {
        const int co = u->dims[l + 1];
        res(u->down_res[2 * l], H, W, cur_c, 0, l == 0 && first_fast(*u, B, H, W));
        res(u->down_res[2 * l + 1], H, W, co, 0, false);
        attn(u->down_attn[l], H, W);
        if (l < u->L - 1) { f += conv_flops(DDK_CONV3X3_S2, B, H, W, co, co); H /= 2; W /= 2; }
        cur_c = co;
    }
    res(u->mid1, H, W, cur_c, 0, false); attn(u->mid_attn, H, W); res(u->mid2, H, W, cur_c, 0, false);
    for (int i = 0; i < u->L - 1; ++i) {
        const int lvl = u->L - 1 - i, dout = u->dims[lvl + 1], din = u->dims[lvl];
        res(u->up_res[2 * i], H, W, cur_c, dout, false);
        res(u->up_res[2 * i + 1], H, W, din, 0, false);
        attn(u->up_attn[i], H, W);
        if (u->up_conv[i].has_wu && convT_wino_use(B, H, W, din, din))  // Winograd F(2x2, 2x2) per phase: 36 position GEMMs per 2x2 input tile
            f += 2.0 * (double)(ceil_div((long long)B * (H / 2) * (W / 2), 32) * 32) * 36.0 * din * din;
        else
            f += conv_flops(DDK_CONVT4X4_S2, B, H, W, din, din);
        H *= 2; W *= 2;
        cur_c = din;
    }
    f += conv3(u->final_conv, H, W, cur_c, 0, u->cfg.chan) + 2.0 * B * H * W * (double)u->cfg.chan * u->cfg.in_ch;
    return f;
}

// ------------------------------------------------------------------------------------------------ sampler
namespace ddk {
struct SamplerLayout {
    size_t unet_floats, off_eps, off_t, off_table, off_tact_all, off_tall, total;
};
// rows = t_start + 1 timesteps: the time-shift table [rows][temb_total], its staging [rows][time_dim] and int64 t = 0..rows-1
static SamplerLayout sampler_layout(const ddk_unet& u, int B, int H, int W, int t_start) {
    SamplerLayout s;
    const size_t rows = (size_t)t_start + 1;
    s.unet_floats = make_layout(u, B, H, W).total;
    s.off_eps = s.unet_floats;
    s.off_t = s.off_eps + al4((size_t)B * H * W * u.cfg.in_ch);
    s.off_table = s.off_t + al4(2 * (size_t)(B + 3));  // int64 t_cur[B] + chain state {counter, seed, stream id}, in float units
    s.off_tact_all = s.off_table + al4(rows * u.temb_total);
    s.off_tall = s.off_tact_all + al4(rows * u.time_dim);
    s.total = s.off_tall + al4(2 * rows);
    return s;
}

__global__ void iota64_kernel(int64_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}
}  // namespace ddk


namespace ddk {
// Time-shift table for rows 0..t_start: the same two kernels a forward runs, once, with "batch" = all rows.  Row k holds the shifts
// of timestep map[k] (map == nullptr: timestep k).  It lives in the caller's workspace (sampler_layout: the sweep's workspace starts
// with the same layout) and stays valid while neither the weights (pack_epoch), the workspace nor the map change; the key keeps a
// copy of the map, so a respaced chain and a plain chain of the same length on one workspace never read each other's rows.  A
// caller that rewrites or frees the workspace between calls says so with ddk_sampler_invalidate().
static int ensure_temb_table(ddk_unet& u, const float* P, float* ws, const SamplerLayout& sl, int t_start, int B, int H, int W,
                             hipStream_t st, const int64_t* map) {
    const int rows = t_start + 1;
    const bool same_map = map ? (u.table.map.size() == (size_t)rows && std::equal(map, map + rows, u.table.map.begin()))
                              : u.table.map.empty();
    if (u.table.ws == ws && u.table.t_start == t_start && u.table.B == B && u.table.H == H && u.table.W == W &&
        u.table.pack_epoch == u.pack_epoch && same_map)
        return DDK_OK;
    u.table.ws = nullptr;                    // a rebuild that fails half way leaves no valid table behind
    int64_t* t_all = reinterpret_cast<int64_t*>(ws + sl.off_tall);
    float* tact_all = ws + sl.off_tact_all;
    if (map) {
        // the plan's own copy is the source; the wait keeps it alive (and the caller's array free) until the copy has landed
        u.table.map.assign(map, map + rows);
        DDK_HIP(hipMemcpyAsync(t_all, u.table.map.data(), (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, st));
        DDK_HIP(hipStreamSynchronize(st));
    } else {
        u.table.map.clear();
        hipLaunchKernelGGL(iota64_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, t_all, rows);
        DDK_TRY(check_launch("iota64_kernel"));
    }
    DDK_TRY(time_mlp(t_all, P + u.freqs, P + u.w1t, P + u.b1, P + u.w2t, P + u.b2, tact_all, nullptr, rows, u.time_dim, st));
    DDK_TRY(time_proj(tact_all, P + u.temb_wt, P + u.temb_bias, ws + sl.off_table, rows, u.time_dim, u.temb_total, st));
    u.table.ws = ws; u.table.t_start = t_start; u.table.B = B; u.table.H = H; u.table.W = W;
    u.table.pack_epoch = u.pack_epoch;
    return DDK_OK;
}

// n_steps steps of a chain whose state (counter, Philox key) is already in device memory, each step issued by one_step():
// eagerly, or from the plan's graph cache (caller holds u.mu).  A new key runs its first step eagerly and captures a one-step
// graph (and, for chains that can be long and draw their own noise, a SAMPLER_MULTI-step graph); at most 4 keys stay cached (LRU).
template <class F>
static int run_chain(ddk_unet& u, const ChainKey& key, int n_steps, bool use_graph, F&& one_step, hipStream_t st, const char* who) {
    if (!use_graph || n_steps == 1) {
        for (int k = 0; k < n_steps; ++k) DDK_TRY(one_step());
        return DDK_OK;
    }
    auto capture = [&](int steps, hipGraph_t& graph, hipGraphExec_t& exec) -> int {
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) {
            set_error("%s: hipStreamBeginCapture failed (%s); the legacy NULL stream cannot be captured -- pass a created stream", who,
                      hipGetErrorString(e));
            return DDK_ERR_HIP;
        }
        int rc = DDK_OK;
        for (int i = 0; i < steps && rc == DDK_OK; ++i) rc = one_step();
        e = hipStreamEndCapture(st, &graph);
        if (rc != DDK_OK) { if (graph) (void)hipGraphDestroy(graph); graph = nullptr; return rc; }
        if (e != hipSuccess) { graph = nullptr; set_error("%s: hipStreamEndCapture: %s", who, hipGetErrorString(e)); return DDK_ERR_HIP; }
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(graph);
            graph = nullptr; exec = nullptr;
            set_error("%s: hipGraphInstantiate: %s", who, hipGetErrorString(e));
            return DDK_ERR_HIP;
        }
        return DDK_OK;
    };

    SamplerGraph* hit = nullptr;
    for (SamplerGraph& g : u.graphs)
        if (g.key == key) {
            hit = &g;
            break;
        }
    int first = 0;
    if (!hit) {
        // New buffer set: run the first step eagerly, capture the second, keep the executable graph in the plan.
        if (u.graphs.size() >= 4) {      // bounded cache: retire the least recently used entry (its launches must have drained)
            size_t lru = 0;
            for (size_t i = 1; i < u.graphs.size(); ++i)
                if (u.graphs[i].last_use < u.graphs[lru].last_use) lru = i;
            // wait for the evicted entry's own launches only (not the device: another stream may be mid-capture)
            destroy_entry(u.graphs[lru]);
            u.graphs.erase(u.graphs.begin() + (long)lru);
        }
        DDK_TRY(one_step());
        first = 1;
        SamplerGraph g{};
        g.key = key;
        DDK_TRY(capture(1, g.graph, g.exec));
        u.graphs.push_back(g);
        hit = &u.graphs.back();
    }
    hit->last_use = ++u.use_clock;
    int k = first;
    // long chains: SAMPLER_MULTI steps per graph launch (t and the Philox counter live in device memory, so a graph of any number
    // of steps continues the chain); the one-step graph finishes the remainder
    // (captured with the one-step graph, on the first call for a buffer set whose chain can be that long -- not in a later, timed call)
    // (not for injected noise: a fresh noise tensor per call means a fresh cache entry per call -- parity tests -- and capturing
    //  SAMPLER_MULTI x ~80 launches for a chain that is never replayed is pure overhead)
    if (!hit->exec_multi && !key.noise && (first || n_steps - k >= 2 * SAMPLER_MULTI) && key.t_start + 1 >= 2 * SAMPLER_MULTI)
        DDK_TRY(capture(SAMPLER_MULTI, hit->graph_multi, hit->exec_multi));
    if (hit->exec_multi)
        for (; k + SAMPLER_MULTI <= n_steps; k += SAMPLER_MULTI) {
            const hipError_t e = hipGraphLaunch(hit->exec_multi, st);
            if (e != hipSuccess) { set_error("%s: hipGraphLaunch: %s", who, hipGetErrorString(e)); return DDK_ERR_HIP; }
        }
    for (; k < n_steps; ++k) {
        const hipError_t e = hipGraphLaunch(hit->exec, st);
        if (e != hipSuccess) { set_error("%s: hipGraphLaunch: %s", who, hipGetErrorString(e)); return DDK_ERR_HIP; }
    }
    if (!hit->done) DDK_HIP(hipEventCreateWithFlags(&hit->done, hipEventDisableTiming));
    DDK_HIP(hipEventRecord(hit->done, st));
    return DDK_OK;
}

// What a chain entry (sampler_chain, ddk_vlb_sweep_run) hands its steps and run_chain, filled by begin_chain.
struct ChainRun {
    ddk_unet* u;
    int B, H, W;
    const float* P;
    float* ws;
    Layout ly;
    SamplerLayout sl;                        // the workspace starts with the sampler's layout (the sweep's too)
    int64_t* t_cur;
    int64_t* state;                          // [0] step counter, [1] seed, [2] stream id
    long long per;                           // H * W * in_ch
    hipStream_t st;
    int dev = 0;                             // the current device: part of the graph cache key
    std::unique_lock<std::mutex> lock;       // u->mu, held until the entry returns

    // one UNet forward of a step on `x`: the counter bookkeeping in its first kernel, step->rule in its last
    int forward(const float* x, const StepArgs* step) {
        return forward_core(*u, P, x, t_cur, nullptr, B, H, W, ws, ly, st, u->cluster_gn >= 1, ws + sl.off_table, step);
    }
};

// The prologue both chains share, after the entry's own argument checks: shape, alignment and workspace (`workspace_floats`
// is what the entry needs in all, given the sampler layout), then under the plan's lock the cluster counters' memset, the
// chain state {t_start, seed, stream_id} and the time-shift table of rows 0..t_start (map: ensure_temb_table).
template <class Args, class Need>
static int begin_chain(ChainRun& c, const Args* a, const char* who, int t_start, uint32_t stream_id, const int64_t* map, int n_steps,
                       Need&& workspace_floats, ddk_stream_t s) {
    c.u = const_cast<ddk_unet*>(a->unet);   // the graph / table cache is logically mutable state of the plan
    const int B = a->B, H = a->H, W = a->W;
    c.B = B; c.H = H; c.W = W;
    DDK_TRY(check_shape(c.u, B, H, W));
    if (!(aligned16(a->packed) && aligned16(a->workspace) && aligned16(a->x) && aligned16(a->noise)))
        return fail_arg((std::string(who) + ": alignment").c_str());
    c.per = (long long)H * W * c.u->cfg.in_ch;
    if (c.per % 4) return fail_arg((std::string(who) + ": H*W*in_ch must be a multiple of 4").c_str());
    c.sl = sampler_layout(*c.u, B, H, W, t_start);
    const size_t need = workspace_floats(c.sl) * sizeof(float);
    if (a->workspace_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu)", who, a->workspace_bytes, need);
        return DDK_ERR_WORKSPACE;
    }
    DDK_TRY(ensure_device_init());
    c.ly = make_layout(*c.u, B, H, W);
    c.st = as_stream(s);
    c.ws = static_cast<float*>(a->workspace);
    c.P = static_cast<const float*>(a->packed);
    c.t_cur = reinterpret_cast<int64_t*>(c.ws + c.sl.off_t);
    c.state = c.t_cur + B;
    c.lock = std::unique_lock<std::mutex>(c.u->mu);
    DDK_HIP(hipMemsetAsync(c.ws + c.ly.off_cl, 0, cl_counter_floats(B) * sizeof(float), c.st));  // cluster GroupNorm counters (outside the graph)
    hipLaunchKernelGGL(set_chain_state_kernel, dim3(1), dim3(1), 0, c.st, c.state, (int64_t)t_start, a->seed, stream_id);
    DDK_TRY(check_launch("set_chain_state_kernel"));
    DDK_TRY(ensure_temb_table(*c.u, c.P, c.ws, c.sl, t_start, B, H, W, c.st, map));
    if (a->use_graph && n_steps > 1) DDK_HIP(hipGetDevice(&c.dev));
    return DDK_OK;
}
}  // namespace ddk

extern "C" int ddk_sampler_run(const ddk_sampler_args* a, ddk_stream_t s) {
    return ddk_sampler_run_spaced(a, nullptr, s);
}

namespace ddk {
// a host timestep map of t_start + 1 entries: map[0] == 0, strictly increasing, below 2^31 (null: the identity)
static int check_timestep_map(const int64_t* map, int t_start, const char* who) {
    if (!map) return DDK_OK;
    if (map[0] != 0) {
        set_error("%s: timestep_map[0] must be 0, got %lld", who, (long long)map[0]);
        return DDK_ERR_ARG;
    }
    for (int k = 1; k <= t_start; ++k)
        if (map[k] <= map[k - 1] || map[k] >= (int64_t(1) << 31)) {
            set_error("%s: timestep_map must increase strictly and stay below 2^31 (entry %d = %lld after %lld)", who, k,
                      (long long)map[k], (long long)map[k - 1]);
            return DDK_ERR_ARG;
        }
    return DDK_OK;
}
}  // namespace ddk

namespace ddk {
// floats a chain keeps behind the sampler layout, by its rule: the multistep history [B][H][W][in_ch]; the inpainting op's known
// latent and mask; a restore kind's measurement.  The size queries and sampler_chain's carve-up both come from here.
// The restore kinds (restore_n = the block, 1 included): (RestoreMultistep: the history, then) y of that block, [B][H/n][W/n][in_ch]
// (the grey y is a third of that place), and behind it the mask [B][H/n][W/n], reserved with or without one.  Restore itself keeps
// room for n = 2 without a mask, a quarter of the latent, whatever its n; RestoreMasked, RestoreNoisy and RestoreGray never keep less
// than that at n >= 2, since a masked call without a mask is the Restore kind's chain.
struct RestoreStage {
    size_t hist, y, mask;         // the floats of each part, 4-float aligned; y starts at hist, the mask at hist + y
};
static RestoreStage restore_stage(size_t n, int B, int H, int W, StepKind kind, int restore_n) {
    const size_t nn = (size_t)restore_n * restore_n;
    return {kind == StepKind::RestoreMultistep ? al4(n) : 0, al4(n / nn), al4((size_t)B * H * W / nn)};
}
// The plane-wide kinds (no block) lay their staging area out with a bump: every part is a multiple of four floats, so each starts on a
// 16-byte boundary.  A layout holds its parts' offsets in floats from the chain's extra area, then the total; n is the latent's floats.
struct Bump {
    size_t at = 0;
    size_t take(size_t floats) { const size_t off = at; at += al4(floats); return off; }
};
// RestoreBlur: P_h [H][H], P_w [W][W], Yp and T, the last two of the latent's size.  Q_h and Q_w are only read while Yp is formed, from
// the caller's buffers.
struct BlurStage { size_t ph, pw, yp, tmp, total; };
static BlurStage blur_stage(size_t n, int H, int W) {
    Bump b;
    return {b.take((size_t)H * H), b.take((size_t)W * W), b.take(n), b.take(n), b.at};      // (a braced list: left to right)
}
// RestoreHadamard: perm [H W] int32, y [B][C][m] in a place of the latent's size (m <= H W) and T of the latent's size
struct CsStage { size_t perm, y, tmp, total; };
static CsStage cs_stage(size_t n, int H, int W) {
    Bump b;
    return {b.take((size_t)H * W), b.take(n), b.take(n), b.at};
}
// RestoreFFT: the mask [H W], the twiddles (max(H, W) / 2 complex), Yp of the latent's size and the complex T of twice it
struct FftStage { size_t mask, tw, yp, tmp, total; };
static FftStage fft_stage(size_t n, int H, int W) {
    Bump b;
    return {b.take((size_t)H * W), b.take((size_t)(H > W ? H : W)), b.take(n), b.take(2 * al4(n)), b.at};
}
// RestoreFFTNoisy: RestoreFFT's area (the place of the image Yp stays unused), behind its T the draw's T2 of the same size when a plane
// takes the multi-launch form, then gain [H W], nsc (one float per row of the chain) and the complex spectrum of A+ y
struct FftNoisyStage { FftStage f; size_t gain, nsc, yhat, total; };
static FftNoisyStage fft_noisy_stage(size_t n, int H, int W, int t_start) {
    const FftStage f = fft_stage(n, H, W);
    Bump b{f.total + (restore_fft_plane_form(H, W) ? 0 : 2 * al4(n))};
    return {f, b.take((size_t)H * W), b.take((size_t)t_start + 1), b.take(2 * al4(n)), b.at};
}
static size_t chain_extra_floats(const ddk_unet& u, int B, int H, int W, StepKind kind, int restore_n = 0, int t_start = 0) {
    const size_t n = al4((size_t)B * H * W * u.cfg.in_ch);
    if (kind == StepKind::RestoreFFTNoisy) return fft_noisy_stage(n, H, W, t_start).total;
    if (kind == StepKind::RestoreFFT) return fft_stage(n, H, W).total;
    if (kind == StepKind::RestoreHadamard) return cs_stage(n, H, W).total;
    if (kind == StepKind::RestoreBlur) return blur_stage(n, H, W).total;
    if (kind == StepKind::Restore) return al4(n / 4);
    if (restore_kind(kind)) {
        const RestoreStage g = restore_stage(n, B, H, W, kind, restore_n);
        const size_t m = g.hist + g.y + g.mask;
        return kind != StepKind::RestoreMultistep && restore_n > 1 && m < al4(n / 4) ? al4(n / 4) : m;
    }
    return kind == StepKind::Multistep ? n : kind == StepKind::Inpaint ? 2 * n : 0;
}
static size_t sampler_bytes(const ddk_unet* u, int B, int H, int W, int t_start, StepKind kind, int restore_n = 0) {
    if (check_shape(u, B, H, W) != DDK_OK || t_start < 0) return 0;
    return (sampler_layout(*u, B, H, W, t_start).total + chain_extra_floats(*u, B, H, W, kind, restore_n, t_start)) * sizeof(float);
}

// A plane-wide kind's operands, staged before the first step and outside any captured one.  On entry rule.rst.y is the CALLER's y and
// the kind's member of rule (blr, had, fft, fnz) holds the caller's arrays; each function copies them into the chain's extra area, forms
// Yp or the spectrum there and rewrites rule to point into the workspace.
struct Stage {                    // the chain's stream, extra area, latent floats, shape, channels and first row; then what the graph key needs of
    hipStream_t st;               // the staged operands besides the workspace:
    float* extra;
    size_t n;
    int B, H, W, C, t_start;
    int key_n = 0;                // RestoreHadamard: m, the measured coefficients per plane (the kernels are launched with it); else 0, the kind says it
    NoisyTables key_tables{};     // RestoreFFTNoisy: the caller's gain and nsc, which name the point-spread function and sigma_y; else null
    int copy(size_t off, const void* from, size_t bytes) const {
        DDK_HIP(hipMemcpyAsync(extra + off, from, bytes, hipMemcpyDeviceToDevice, st));
        return DDK_OK;
    }
};
static int stage_blur(Stage& g, StepRule& rule, ddk_stream_t s) {
    const BlurStage l = blur_stage(g.n, g.H, g.W);
    DDK_TRY(g.copy(l.ph, rule.blr.ph, (size_t)g.H * g.H * sizeof(float)));
    DDK_TRY(g.copy(l.pw, rule.blr.pw, (size_t)g.W * g.W * sizeof(float)));
    // Yp = Q_h y Q_w^T.  rule.rst.H x rule.rst.W is the size of that y (the entry's h, w): the plane's own takes the square form, in
    // place on Yp; a smaller one the size-changing form with T as its scratch, [B][H][w][C] never exceeding it
    if (rule.rst.H == g.H && rule.rst.W == g.W)
        DDK_TRY(ddk_separable_apply(rule.rst.y, rule.blr.qh, rule.blr.qw, g.extra + l.yp, g.B, g.H, g.W, g.C, s));
    else
        DDK_TRY(ddk_separable_apply_rect(rule.rst.y, rule.blr.qh, rule.blr.qw, g.extra + l.yp, g.extra + l.tmp, g.B, rule.rst.H, rule.rst.W, g.H,
                                         g.W, g.C, s));
    rule.blr = BlurOps{g.extra + l.ph, g.extra + l.pw, g.extra + l.tmp, nullptr, nullptr};
    rule.rst = RestoreOps{g.extra + l.yp, 0, g.H, g.W, 0, nullptr};
    return DDK_OK;
}
static int stage_cs(Stage& g, StepRule& rule) {
    const CsStage l = cs_stage(g.n, g.H, g.W);
    DDK_TRY(g.copy(l.perm, rule.had.perm, (size_t)g.H * g.W * sizeof(int32_t)));
    DDK_TRY(g.copy(l.y, rule.rst.y, (size_t)g.B * g.C * rule.had.m * sizeof(float)));
    g.key_n = rule.had.m;
    rule.had = HadamardOps{reinterpret_cast<const int32_t*>(g.extra + l.perm), g.extra + l.tmp, rule.had.m};
    rule.rst = RestoreOps{g.extra + l.y, 0, g.H, g.W, 0, nullptr};
    return DDK_OK;
}
static int stage_fft(Stage& g, StepRule& rule) {
    const FftStage l = fft_stage(g.n, g.H, g.W);
    DDK_TRY(g.copy(l.mask, rule.fft.mask, (size_t)g.H * g.W * sizeof(float)));
    DDK_TRY(g.copy(l.tw, rule.fft.tw, (size_t)(g.H > g.W ? g.H : g.W) * sizeof(float)));
    // Yp = Re F2^-1(P^ F2 y) / N
    DDK_TRY(circular_conv(rule.rst.y, rule.fft.pinv, g.extra + l.tw, g.extra + l.yp, g.extra + l.tmp, g.B, g.H, g.W, g.C, g.st));
    rule.fft = FftOps{g.extra + l.mask, g.extra + l.tw, g.extra + l.tmp, nullptr};
    rule.rst = RestoreOps{g.extra + l.yp, 0, g.H, g.W, 0, nullptr};
    return DDK_OK;
}
// as stage_fft, with gain and nsc copied in as well and the SPECTRUM of A+ y, P^ . F2 y in the transform's order, in rst.y
static int stage_fft_noisy(Stage& g, StepRule& rule) {
    const FftNoisyStage l = fft_noisy_stage(g.n, g.H, g.W, g.t_start);
    DDK_TRY(g.copy(l.f.mask, rule.fnz.mask, (size_t)g.H * g.W * sizeof(float)));
    DDK_TRY(g.copy(l.f.tw, rule.fnz.tw, (size_t)(g.H > g.W ? g.H : g.W) * sizeof(float)));
    DDK_TRY(g.copy(l.gain, rule.fnz.gain, (size_t)g.H * g.W * sizeof(float)));
    DDK_TRY(g.copy(l.nsc, rule.fnz.nsc, ((size_t)g.t_start + 1) * sizeof(float)));
    DDK_TRY(circular_spectrum(rule.rst.y, rule.fnz.pinv, g.extra + l.f.tw, g.extra + l.yhat, g.extra + l.f.tmp, g.B, g.H, g.W, g.C, g.st));
    g.key_tables = NoisyTables{rule.fnz.gain, rule.fnz.nsc};
    rule.fnz = FftNoisyOps{g.extra + l.f.mask, g.extra + l.f.tw, g.extra + l.f.tmp, g.extra + l.gain, g.extra + l.nsc, nullptr};
    rule.rst = RestoreOps{g.extra + l.yhat, 0, g.H, g.W, 0, nullptr};
    return DDK_OK;
}
static int stage_plane(Stage& g, StepRule& rule, ddk_stream_t s) {
    return rule.kind == StepKind::RestoreBlur ? stage_blur(g, rule, s) : rule.kind == StepKind::RestoreHadamard ? stage_cs(g, rule)
           : rule.kind == StepKind::RestoreFFT ? stage_fft(g, rule) : stage_fft_noisy(g, rule);
}

// What the sampler entries share once their own arguments are checked: n_steps reverse steps on a->x, step k at timestep map[k],
// each ending in `rule`.  The entry sets rule.kind and the operands only its kind has (c3; inp, with the CALLER's known / mask; rst, with the CALLER's y);
// x, the noise and the tables c_recip .. sigma come from *a here.  What a kind keeps in the workspace is staged after begin_chain
// and outside any captured step, so no chain sees another's and the cached graph points only into the workspace:
//   Multistep: the history, zeroed by every call (c3[t_start] == 0 makes the first step first order whatever it would hold)
//   Inpaint:   known and mask, copied in before the first op
//   the block restore kinds: (RestoreMultistep: the history, zeroed by every call as Multistep's, then) y and, when given, the mask,
//              copied in before the first step (restore_stage's layout)
//   the plane-wide restore kinds: stage_plane
// The graph key: the kind, every table the step reads and the restore block; the staged operands live in the workspace, which is
// in the key.
static int sampler_chain(const ddk_sampler_args* a, const char* who, const int64_t* map, StepRule rule, ddk_stream_t s) {
    const int B = a->B, H = a->H, W = a->W, n_steps = a->t_start - a->t_end + 1;
    ChainRun c;
    DDK_TRY(begin_chain(c, a, who, a->t_start, a->stream_id, map, n_steps,
                        [&](const SamplerLayout& sl) { return sl.total + chain_extra_floats(*a->unet, B, H, W, rule.kind, rule.rst.n, a->t_start); }, s));
    rule.x = a->x; rule.noise = a->noise; rule.noise_step_stride = a->noise ? B * c.per : 0; rule.t_first = a->t_start;
    rule.c_recip = a->c_recip; rule.c_recipm1 = a->c_recipm1; rule.c1 = a->c1; rule.c2 = a->c2; rule.sigma = a->sigma;
    const size_t n = (size_t)B * c.per;
    float* extra = c.ws + c.sl.total;
    const bool plane = plane_kind(rule.kind);
    Stage pk{c.st, extra, n, B, H, W, c.u->cfg.in_ch, a->t_start};
    if (rule.kind == StepKind::Multistep) {
        DDK_HIP(hipMemsetAsync(extra, 0, n * sizeof(float), c.st));
        rule.x0_hist = extra;
    } else if (rule.kind == StepKind::Inpaint) {
        DDK_HIP(hipMemcpyAsync(extra, rule.inp.known, n * sizeof(float), hipMemcpyDeviceToDevice, c.st));
        DDK_HIP(hipMemcpyAsync(extra + al4(n), rule.inp.mask, n * sizeof(float), hipMemcpyDeviceToDevice, c.st));
        rule.inp.known = extra;
        rule.inp.mask = extra + al4(n);
    } else if (plane) {
        DDK_TRY(stage_plane(pk, rule, s));
    } else if (restore_kind(rule.kind)) {
        const RestoreStage g = restore_stage(n, B, H, W, rule.kind, rule.rst.n);
        const size_t nn = (size_t)rule.rst.n * rule.rst.n, nm = (size_t)B * H * W / nn;      // one float per block: the mask, and the grey y
        rule.rst.H = H; rule.rst.W = W;
        if (g.hist) {
            DDK_HIP(hipMemsetAsync(extra, 0, n * sizeof(float), c.st));
            rule.x0_hist = extra;
        }
        float* ystage = extra + g.hist;
        DDK_HIP(hipMemcpyAsync(ystage, rule.rst.y, (rule.kind == StepKind::RestoreGray ? nm : n / nn) * sizeof(float),
                               hipMemcpyDeviceToDevice, c.st));
        rule.rst.y = ystage;
        if (rule.rst.mask) {
            DDK_HIP(hipMemcpyAsync(ystage + g.y, rule.rst.mask, nm * sizeof(float), hipMemcpyDeviceToDevice, c.st));
            rule.rst.mask = ystage + g.y;
        }
    }
    const StepArgs step{c.state, c.ws + c.sl.off_eps, c.per, rule};

    // one reverse step: bookkeeping (in the forward's first kernel), UNet, the rule (in its last kernel)
    auto one_step = [&]() -> int { return c.forward(a->x, &step); };

    // the RestoreNoisy / RestoreGray tables share the Inpaint operands' storage (StepRule): each kind's key names its own; the plane-wide
    // kinds' operands are staged, so the workspace names them (but for pk's key_n and key_tables)
    const bool noisy = rule.kind == StepKind::RestoreNoisy || rule.kind == StepKind::RestoreGray;
    const InpaintOps ik = noisy || plane ? InpaintOps{} : rule.inp;
    const NoisyTables nk = noisy ? rule.nsy : pk.key_tables;
    const ChainKey key{rule.kind,
                       {a->packed, a->x, rule.c_recip, rule.c_recipm1, rule.c1, rule.c2, rule.sigma, rule.c3, ik.ka, ik.kb, ik.ja, ik.jb, nk.lam,
                        nk.sgm},
                       a->workspace, a->noise, B, H, W, a->t_start, c.dev, c.u->pack_epoch,
                       plane ? pk.key_n : restore_kind(rule.kind) ? rule.rst.n : 0,
                       (rule.kind == StepKind::RestoreMultistep || noisy) && rule.rst.mask != nullptr,
                       rule.kind == StepKind::RestoreGray ? rule.rst.gray : 0};
    return run_chain(*c.u, key, n_steps, a->use_graph != 0, one_step, c.st, who);
}
}  // namespace ddk

extern "C" size_t ddk_sampler_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return sampler_bytes(u, B, H, W, t_start, StepKind::Ancestral);
}

extern "C" int ddk_sampler_run_spaced(const ddk_sampler_args* a, const int64_t* timestep_map, ddk_stream_t s) {
    DDK_REQUIRE(a && a->unet && a->packed && a->x && a->workspace, "sampler: null pointer");
    DDK_REQUIRE(a->c_recip && a->c_recipm1 && a->c1 && a->c2 && a->sigma, "sampler: null schedule table");
    DDK_REQUIRE(a->t_start >= a->t_end && a->t_end >= 0, "sampler: need t_start >= t_end >= 0");
    DDK_TRY(check_timestep_map(timestep_map, a->t_start, "sampler"));
    StepRule rule{};
    rule.kind = StepKind::Ancestral;
    return sampler_chain(a, "sampler", timestep_map, rule, s);
}

// ------------------------------------------------------------------------------------------------ multistep sampler
// DPM-Solver++(2M): the sampler's chain with the update x_prev = (c1 x0 + c2 x) + c3 x0_hist, x0_hist <- x0.
// A kind of its own and c3 in the graph key: a DDIM chain on the same buffers never replays this graph, nor this one a DDIM graph.
extern "C" size_t ddk_sampler_multistep_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return sampler_bytes(u, B, H, W, t_start, StepKind::Multistep);
}

extern "C" int ddk_sampler_run_multistep(const ddk_sampler_args* a, const int64_t* timestep_map, const float* c3, ddk_stream_t s) {
    DDK_REQUIRE(a && a->unet && a->packed && a->x && a->workspace, "sampler_multistep: null pointer");
    DDK_REQUIRE(a->c_recip && a->c_recipm1 && a->c1 && a->c2 && c3, "sampler_multistep: null schedule table");
    DDK_REQUIRE(!a->noise, "sampler_multistep: the solver is deterministic, noise must be NULL");
    DDK_REQUIRE(a->t_start >= a->t_end && a->t_end >= 0, "sampler_multistep: need t_start >= t_end >= 0");
    DDK_TRY(check_timestep_map(timestep_map, a->t_start, "sampler_multistep"));
    StepRule rule{};
    rule.kind = StepKind::Multistep;
    rule.c3 = c3;
    return sampler_chain(a, "sampler_multistep", timestep_map, rule, s);
}

// ------------------------------------------------------------------------------------------------ inpainting sampler
// RePaint: N reverse ops, row k at timestep map[k]; every op ends in RePaint's select and optional forward
// jump (StepKind::Inpaint).
namespace ddk {
// RePaint's map revisits timesteps, so it is not monotone: map[0] == 0 (the only op at tau = 0) and 0 < map[k] < 2^31 for k > 0
static int check_inpaint_map(const int64_t* map, int t_start, const char* who) {
    if (map[0] != 0) {
        set_error("%s: timestep_map[0] must be 0, got %lld", who, (long long)map[0]);
        return DDK_ERR_ARG;
    }
    for (int k = 1; k <= t_start; ++k)
        if (map[k] <= 0 || map[k] >= (int64_t(1) << 31)) {
            set_error("%s: timestep_map[%d] = %lld must lie in (0, 2^31)", who, k, (long long)map[k]);
            return DDK_ERR_ARG;
        }
    return DDK_OK;
}
}  // namespace ddk

extern "C" size_t ddk_sampler_inpaint_workspace_bytes(const ddk_unet* u, int B, int H, int W, int n_ops) {
    return sampler_bytes(u, B, H, W, n_ops - 1, StepKind::Inpaint);
}

extern "C" int ddk_sampler_run_inpaint(const ddk_sampler_args* a, const ddk_inpaint_args* ip, ddk_stream_t s) {
    DDK_REQUIRE(a && ip && a->unet && a->packed && a->x && a->workspace, "sampler_inpaint: null pointer");
    DDK_REQUIRE(a->c_recip && a->c_recipm1 && a->c1 && a->c2 && a->sigma, "sampler_inpaint: null schedule table");
    DDK_REQUIRE(ip->timestep_map && ip->known && ip->mask && ip->ka && ip->kb && ip->ja && ip->jb, "sampler_inpaint: null inpainting operand");
    DDK_REQUIRE(!a->noise, "sampler_inpaint: injected noise is not supported, noise must be NULL (Philox only)");
    DDK_REQUIRE(a->stream_id < INPAINT_Z3_BIT, "sampler_inpaint: stream_id must be < 2^29 (bits 29, 30 key the extra draws)");
    DDK_REQUIRE(a->t_start >= a->t_end && a->t_end >= 0, "sampler_inpaint: need t_start >= t_end >= 0");
    DDK_REQUIRE(aligned16(ip->known) && aligned16(ip->mask), "sampler_inpaint: alignment");
    DDK_TRY(check_inpaint_map(ip->timestep_map, a->t_start, "sampler_inpaint"));
    StepRule rule{};
    rule.kind = StepKind::Inpaint;
    rule.inp = InpaintOps{ip->known, ip->mask, ip->ka, ip->kb, ip->ja, ip->jb};
    return sampler_chain(a, "sampler_inpaint", ip->timestep_map, rule, s);
}

// ------------------------------------------------------------------------------------------------ restoration samplers
// DDNM (DESIGN.md sections 3.6, 3.8 - 3.11): the spaced sampler's chain and tables, every step ending in one of the restore kinds.  A
// kind of its own, n, whether a mask was given and the grey weights in the graph key: no chain replays another's graph.
namespace ddk {
static bool restore_n_ok(int n, bool n1) { return n == 2 || n == 4 || n == 8 || (n1 && n == 1); }

static size_t restore_bytes(const ddk_unet* u, int B, int H, int W, int t_start, StepKind kind, int n) {
    return restore_n_ok(n, true) ? sampler_bytes(u, B, H, W, t_start, kind, n) : 0;
}

static int restore_tail_parts(const ddk_unet* u, int B, int H, int W, StepKind kind, int n) {
    if (check_shape(u, B, H, W) != DDK_OK || !restore_n_ok(n, true)) return -1;
    return fused_tail_parts(*u, B, H, W, u->dimp[1], kind, n);
}

// What the restore entries share: the checks, the rule and the chain.  The kind says which tables the step reads (sigma, or
// RestoreMultistep's c3; RestoreNoisy's and RestoreGray's lam and sgm); n1: whether the entry takes n = 1, which every kind but the grey
// one constrains through a mask only.
static int restore_chain(const ddk_sampler_args* a, const char* who, const int64_t* map, StepKind kind, bool n1, bool masked_ws, const float* c3,
                         NoisyTables nsy, const float* y, const float* mask, int n, int weights, ddk_stream_t s) {
    auto bad = [who](const char* what) {
        set_error("bad argument: %s: %s", who, what);
        return DDK_ERR_ARG;
    };
    const bool hist = kind == StepKind::RestoreMultistep, gray = kind == StepKind::RestoreGray, noisy = gray || kind == StepKind::RestoreNoisy;
    if (!(a && a->unet && a->packed && a->x && a->workspace && y)) return bad("null pointer");
    if (!(a->c_recip && a->c_recipm1 && a->c1 && a->c2 && (hist ? c3 : a->sigma) && (!noisy || (nsy.lam && nsy.sgm)))) return bad("null schedule table");
    if (a->noise) return bad(hist ? "the solver is deterministic, noise must be NULL" : "injected noise is not supported, noise must be NULL (Philox only)");
    if (gray && a->unet->cfg.in_ch != 3) return bad("the grey operator needs a 3-channel model");
    if (gray && !(weights == GRAY_MEAN || weights == GRAY_LUMA)) return bad("weights must be 1 (mean) or 2 (luma)");
    if (!(a->t_start >= a->t_end && a->t_end >= 0)) return bad("need t_start >= t_end >= 0");
    if (!(restore_n_ok(n, n1) && a->H > 0 && a->W > 0 && a->H % n == 0 && a->W % n == 0))
        return bad(n1 ? "n must be 1, 2, 4 or 8 and divide H and W" : "n must be 2, 4 or 8 and divide H and W");
    if (!(mask || n != 1 || gray)) return bad("n = 1 needs a mask (nothing would be constrained)");
    DDK_TRY(check_timestep_map(map, a->t_start, who));
    // masked_ws: the entry holds the workspace to the masked query's size with or without a mask (never less than the Restore kind's)
    if (masked_ws && a->workspace_bytes < sampler_bytes(a->unet, a->B, a->H, a->W, a->t_start, StepKind::RestoreMasked, n)) {
        set_error("%s: workspace too small (ddk_%s_workspace_bytes)", who, who);
        return DDK_ERR_WORKSPACE;
    }
    StepRule rule{};
    rule.kind = kind;
    rule.c3 = c3;
    if (noisy) rule.nsy = nsy;
    rule.rst = RestoreOps{y, n, a->H, a->W, weights, mask};
    return sampler_chain(a, who, map, rule, s);
}
}  // namespace ddk

extern "C" size_t ddk_sampler_restore_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return sampler_bytes(u, B, H, W, t_start, StepKind::Restore);
}
extern "C" size_t ddk_sampler_restore_masked_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start, int n) {
    return restore_bytes(u, B, H, W, t_start, StepKind::RestoreMasked, n);
}
extern "C" size_t ddk_sampler_restore_multistep_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start, int n) {
    return restore_bytes(u, B, H, W, t_start, StepKind::RestoreMultistep, n);
}
extern "C" size_t ddk_sampler_restore_noisy_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start, int n) {
    return restore_bytes(u, B, H, W, t_start, StepKind::RestoreNoisy, n);
}
extern "C" size_t ddk_sampler_restore_gray_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start, int n) {
    return restore_bytes(u, B, H, W, t_start, StepKind::RestoreGray, n);
}

extern "C" int ddk_sampler_restore_tail_parts(const ddk_unet* u, int B, int H, int W, int n) {
    if (check_shape(u, B, H, W) != DDK_OK) return -1;
    return fused_tail_parts(*u, B, H, W, u->dimp[1], StepKind::Restore, n);      // any n: what final_tail_ok makes of it
}
extern "C" int ddk_sampler_restore_masked_tail_parts(const ddk_unet* u, int B, int H, int W, int n) {
    return restore_tail_parts(u, B, H, W, StepKind::RestoreMasked, n);
}
extern "C" int ddk_sampler_restore_multistep_tail_parts(const ddk_unet* u, int B, int H, int W, int n) {
    return restore_tail_parts(u, B, H, W, StepKind::RestoreMultistep, n);
}
extern "C" int ddk_sampler_restore_noisy_tail_parts(const ddk_unet* u, int B, int H, int W, int n) {
    return restore_tail_parts(u, B, H, W, StepKind::RestoreNoisy, n);
}
extern "C" int ddk_sampler_restore_gray_tail_parts(const ddk_unet* u, int B, int H, int W, int n) {
    return restore_tail_parts(u, B, H, W, StepKind::RestoreGray, n);
}

// super-resolution, A = pool_n (section 3.6)
extern "C" int ddk_sampler_run_restore(const ddk_sampler_args* a, const int64_t* timestep_map, const float* y, int n, ddk_stream_t s) {
    return restore_chain(a, "sampler_restore", timestep_map, StepKind::Restore, false, false, nullptr, {}, y, nullptr, n, 0, s);
}

// A = mask o pool_n (section 3.8): n = 1 is inpainting on the spaced / DDIM tables, an all-measured mask at n >= 2 is
// ddk_sampler_run_restore, in between is super-resolution of a low-resolution image with holes.  With a mask the steps end in
// StepKind::RestoreMasked; without one (n >= 2 only) the chain IS the Restore kind's: its rule, its kernels, its graph key.
extern "C" int ddk_sampler_run_restore_masked(const ddk_sampler_args* a, const int64_t* timestep_map, const float* y, const float* mask, int n,
                                              ddk_stream_t s) {
    return restore_chain(a, "sampler_restore_masked", timestep_map, mask ? StepKind::RestoreMasked : StepKind::Restore, true, true, nullptr, {}, y,
                         mask, n, 0, s);
}

// the DPM-Solver++(2M) chain (section 3.9): ddk_sampler_run_multistep's tables and zeroed history, y and the optional mask of
// ddk_sampler_run_restore_masked
extern "C" int ddk_sampler_run_restore_multistep(const ddk_sampler_args* a, const int64_t* timestep_map, const float* c3, const float* y,
                                                 const float* mask, int n, ddk_stream_t s) {
    return restore_chain(a, "sampler_restore_multistep", timestep_map, StepKind::RestoreMultistep, true, false, c3, {}, y, mask, n, 0, s);
}

// DDNM+ for a noisy measurement (section 3.10): ddk_sampler_run_restore_masked's chain with the per-row tables lam and sgm
extern "C" int ddk_sampler_run_restore_noisy(const ddk_sampler_args* a, const int64_t* timestep_map, const float* lam, const float* sgm,
                                             const float* y, const float* mask, int n, ddk_stream_t s) {
    return restore_chain(a, "sampler_restore_noisy", timestep_map, StepKind::RestoreNoisy, true, false, nullptr, {lam, sgm}, y, mask, n, 0, s);
}

// A = mask o pool_n o grey_w on a 3-channel pixel model (section 3.11): ddk_sampler_run_restore_noisy's chain; y and the mask are
// [B][H/n][W/n], the mask optional at every n
extern "C" int ddk_sampler_run_restore_gray(const ddk_sampler_args* a, const int64_t* timestep_map, const float* lam, const float* sgm,
                                            const float* y, const float* mask, int n, int weights, ddk_stream_t s) {
    return restore_chain(a, "sampler_restore_gray", timestep_map, StepKind::RestoreGray, true, false, nullptr, {lam, sgm}, y, mask, n, weights, s);
}

// The plane-wide restore kinds (sections 3.14, 3.15, 3.17 - 3.19): the spaced sampler's chain on a pixel-space model, every step ending
// in a kind whose operator couples a whole plane, so no step takes the fused tail: the forward writes eps_hat to the step's scratch and
// the kind's own update follows (separable.hip, hadamard.hip, fft_conv.hip).  What their entries share:
namespace ddk {
static bool plane_shape_ok(StepKind kind, int H, int W, int channels) {
    return kind == StepKind::RestoreBlur ? restore_blur_shape_ok(H, W, channels)
           : kind == StepKind::RestoreHadamard ? restore_cs_shape_ok(H, W, channels) : restore_fft_shape_ok(H, W, channels);
}
static size_t plane_bytes(const ddk_unet* u, int B, int H, int W, int t_start, StepKind kind) {
    if (check_shape(u, B, H, W) != DDK_OK || !plane_shape_ok(kind, H, W, u->cfg.in_ch)) return 0;
    return sampler_bytes(u, B, H, W, t_start, kind);
}
static int plane_tail_parts(const ddk_unet* u, int B, int H, int W, StepKind kind) {
    if (check_shape(u, B, H, W) != DDK_OK) return -1;
    return fused_tail_parts(*u, B, H, W, u->dimp[1], kind);      // 0: final_tail_ok takes no plane-wide kind
}
// A run entry: its checks, then the chain.  In this order: null pointers (`ops` are the entry's own operands, all required), null
// schedule tables, injected noise, t_start >= t_end >= 0, the kind's shape rule, what only the entry checks (own(): null, or its
// text; it may still write to rule), the operands' alignment, the timestep map
template <class Own>
static int plane_chain(const ddk_sampler_args* a, const char* who, const int64_t* map, const StepRule& rule,
                       std::initializer_list<const void*> ops, Own&& own, ddk_stream_t s) {
    auto bad = [who](const char* what) {
        set_error("bad argument: %s: %s", who, what);
        return DDK_ERR_ARG;
    };
    bool there = a && a->unet && a->packed && a->x && a->workspace, aligned = true;
    for (const void* p : ops) { there = there && p; aligned = aligned && aligned16(p); }
    if (!there) return bad("null pointer");
    if (!(a->c_recip && a->c_recipm1 && a->c1 && a->c2 && a->sigma)) return bad("null schedule table");
    if (a->noise) return bad("injected noise is not supported, noise must be NULL (Philox only)");
    if (!(a->t_start >= a->t_end && a->t_end >= 0)) return bad("need t_start >= t_end >= 0");
    if (!plane_shape_ok(rule.kind, a->H, a->W, a->unet->cfg.in_ch))
        return bad(rule.kind == StepKind::RestoreBlur ? "H and W must be multiples of 16 in [16, 256], the model's channels 1 to 8"
                                                      : "H and W must be powers of two in [16, 256], the model's channels 1 to 8");
    if (const char* fault = own()) return bad(fault);
    if (!aligned) return bad("alignment");
    DDK_TRY(check_timestep_map(map, a->t_start, who));
    return sampler_chain(a, who, map, rule, s);
}
static StepRule plane_rule(StepKind kind, const float* y) {
    StepRule rule{};
    rule.kind = kind;
    rule.rst.y = y;
    return rule;
}
// (the deconvolution entries: one workgroup row per plane)
static const char* fft_planes_fault(const ddk_sampler_args* a) {
    return a->B > 0 && (long long)a->B * a->unet->cfg.in_ch <= 65535 ? nullptr : "B channels must be in [1, 65535]";
}
}  // namespace ddk

// DDNM deblurring, A(X) = A_h X A_w^T per channel (section 3.14), StepKind::RestoreBlur.  P = A+ A and Q = A+ of the two axes are the
// caller's (models/diffusion/blur.py), row-major [H][H] and [W][W] device arrays; y is the blurred image in x's layout.
extern "C" size_t ddk_sampler_restore_blur_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return plane_bytes(u, B, H, W, t_start, StepKind::RestoreBlur);
}
extern "C" int ddk_sampler_restore_blur_tail_parts(const ddk_unet* u, int B, int H, int W) {
    return plane_tail_parts(u, B, H, W, StepKind::RestoreBlur);
}
// (both entries: y is [B][h][w][C], Q_h [H][h], Q_w [W][w]; the deblurring entry's h, w are the plane's)
static int restore_blur_chain(const ddk_sampler_args* a, const char* who, const int64_t* timestep_map, const float* P_h, const float* P_w,
                              const float* Q_h, const float* Q_w, const float* y, bool sized, int h, int w, ddk_stream_t s) {
    StepRule rule = plane_rule(StepKind::RestoreBlur, y);
    rule.blr = BlurOps{P_h, P_w, nullptr, Q_h, Q_w};
    return plane_chain(a, who, timestep_map, rule, {y, P_h, P_w, Q_h, Q_w}, [&]() -> const char* {
        const int hh = rule.rst.H = sized ? h : a->H, ww = rule.rst.W = sized ? w : a->W;      // of the caller's y, until stage_blur has formed Yp
        return hh >= 4 && hh <= a->H && hh % 4 == 0 && ww >= 4 && ww <= a->W && ww % 4 == 0 ? nullptr : "h and w must be multiples of 4 in [4, H] and [4, W]";
    }, s);
}
extern "C" int ddk_sampler_run_restore_blur(const ddk_sampler_args* a, const int64_t* timestep_map, const float* P_h, const float* P_w,
                                            const float* Q_h, const float* Q_w, const float* y, ddk_stream_t s) {
    return restore_blur_chain(a, "sampler_restore_blur", timestep_map, P_h, P_w, Q_h, Q_w, y, false, 0, 0, s);
}
// DDNM for a size-changing separable operator (section 3.15): the same chain with y [B][h][w][C] and Q_h [H][h], Q_w [W][w]
extern "C" int ddk_sampler_run_restore_sep(const ddk_sampler_args* a, const int64_t* timestep_map, const float* P_h, const float* P_w,
                                           const float* Q_h, const float* Q_w, const float* y, int h, int w, ddk_stream_t s) {
    return restore_blur_chain(a, "sampler_restore_sep", timestep_map, P_h, P_w, Q_h, Q_w, y, true, h, w, s);
}

// DDNM compressed sensing (section 3.17), StepKind::RestoreHadamard.  y [B][C][m] and perm [H W] are the caller's device arrays, copied
// into the workspace before the first step.
extern "C" size_t ddk_sampler_restore_cs_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return plane_bytes(u, B, H, W, t_start, StepKind::RestoreHadamard);
}
extern "C" int ddk_sampler_restore_cs_tail_parts(const ddk_unet* u, int B, int H, int W) {
    return plane_tail_parts(u, B, H, W, StepKind::RestoreHadamard);
}
extern "C" int ddk_sampler_run_restore_cs(const ddk_sampler_args* a, const int64_t* timestep_map, const float* y, const int32_t* perm, int m,
                                          ddk_stream_t s) {
    StepRule rule = plane_rule(StepKind::RestoreHadamard, y);
    rule.had = HadamardOps{perm, nullptr, m};
    return plane_chain(a, "sampler_restore_cs", timestep_map, rule, {y, perm},
                       [&]() { return restore_cs_rows_ok(a->H, a->W, m) ? nullptr : "m must be a multiple of 4 in [4, H W]"; }, s);
}

// DDNM deconvolution of a 2-D point-spread function with periodic boundary (section 3.18), StepKind::RestoreFFT.  mask [H][W], P^ [H][W]
// complex, the twiddles and y (x's layout) are the caller's device arrays; mask and twiddles are copied into the workspace and Yp = A+ y
// is formed there before the first step.
extern "C" size_t ddk_sampler_restore_fft_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return plane_bytes(u, B, H, W, t_start, StepKind::RestoreFFT);
}
extern "C" int ddk_sampler_restore_fft_tail_parts(const ddk_unet* u, int B, int H, int W) {
    return plane_tail_parts(u, B, H, W, StepKind::RestoreFFT);
}
extern "C" int ddk_sampler_run_restore_fft(const ddk_sampler_args* a, const int64_t* timestep_map, const float* mask, const float* P,
                                           const float* twiddles, const float* y, ddk_stream_t s) {
    StepRule rule = plane_rule(StepKind::RestoreFFT, y);
    rule.fft = FftOps{mask, twiddles, nullptr, P};
    return plane_chain(a, "sampler_restore_fft", timestep_map, rule, {mask, P, twiddles, y}, [&]() { return fft_planes_fault(a); }, s);
}

// DDNM+ deconvolution of a noisy blurred image (section 3.19): ddk_sampler_run_restore_fft's chain, every step ending in
// StepKind::RestoreFFTNoisy.  gain [H][W] and nsc (t_start + 1 floats) join the caller's device arrays; all of them are copied into
// the workspace and the spectrum of A+ y is formed there before the first step.  The caller's gain and nsc are in the graph key, so a
// chain of one sigma_y never replays another's graph, and the kind keeps it from a deconvolution chain's.
extern "C" size_t ddk_sampler_restore_fft_noisy_workspace_bytes(const ddk_unet* u, int B, int H, int W, int t_start) {
    return plane_bytes(u, B, H, W, t_start, StepKind::RestoreFFTNoisy);
}
extern "C" int ddk_sampler_restore_fft_noisy_tail_parts(const ddk_unet* u, int B, int H, int W) {
    return plane_tail_parts(u, B, H, W, StepKind::RestoreFFTNoisy);
}
extern "C" int ddk_sampler_run_restore_fft_noisy(const ddk_sampler_args* a, const int64_t* timestep_map, const float* mask, const float* P,
                                                 const float* gain, const float* nsc, const float* twiddles, const float* y, ddk_stream_t s) {
    StepRule rule = plane_rule(StepKind::RestoreFFTNoisy, y);
    rule.fnz = FftNoisyOps{mask, twiddles, nullptr, gain, nsc, P};
    return plane_chain(a, "sampler_restore_fft_noisy", timestep_map, rule, {mask, P, gain, nsc, twiddles, y},
                       [&]() { return fft_planes_fault(a); }, s);
}

// ------------------------------------------------------------------------------------------------ likelihood sweep
namespace ddk {
struct SweepLayout {
    SamplerLayout sl;             // the sampler's layout first (UNet scratch, eps_hat, t_cur + chain state, time-shift table)
    size_t off_xt, off_part, total;
    int nslot;
};
static SweepLayout sweep_layout(const ddk_unet& u, int B, int H, int W, int T) {
    SweepLayout s;
    s.sl = sampler_layout(u, B, H, W, T - 1);
    const long long per = (long long)H * W * u.cfg.in_ch;
    const int npf = fused_tail_parts(u, B, H, W, u.dimp[1], StepKind::Vlb);
    s.nslot = npf > 0 ? npf : vlb_sweep_slots_unfused(B, per);
    s.off_xt = s.sl.total;
    s.off_part = s.off_xt + al4((size_t)B * per);
    s.total = s.off_part + al4((size_t)T * B * s.nslot * 2);
    return s;
}
}  // namespace ddk

extern "C" size_t ddk_vlb_sweep_workspace_bytes(const ddk_unet* u, int B, int H, int W, int T) {
    if (check_shape(u, B, H, W) != DDK_OK || T < 1) return 0;
    return sweep_layout(*u, B, H, W, T).total * sizeof(float);
}

extern "C" int ddk_vlb_sweep_run(const ddk_vlb_sweep_args* a, ddk_stream_t s) {
    DDK_REQUIRE(a && a->unet && a->packed && a->x && a->workspace && a->vlb_t && a->l_simple_t, "vlb_sweep: null pointer");
    DDK_REQUIRE(a->sqrt_acp && a->sqrt_1m_acp && a->c_recip && a->c_recipm1 && a->c1 && a->c2 && a->post_logvar,
                "vlb_sweep: null schedule table");
    DDK_REQUIRE(a->T >= 1, "vlb_sweep: need T >= 1");
    DDK_REQUIRE((a->stream_id & VLB_STREAM_BIT) == 0, "vlb_sweep: stream_id must be < 2^31 (the top bit separates the sweep's draws)");
    const int B = a->B, H = a->H, W = a->W, T = a->T;
    ChainRun c;
    DDK_TRY(begin_chain(c, a, "vlb_sweep", T - 1, a->stream_id | VLB_STREAM_BIT, nullptr, T,
                        [&](const SamplerLayout&) { return sweep_layout(*a->unet, B, H, W, T).total; }, s));
    const SweepLayout vl = sweep_layout(*c.u, B, H, W, T);
    const long long per = c.per;
    float* xt = c.ws + vl.off_xt;
    float* partials = c.ws + vl.off_part;
    const VlbStep v{a->x, xt, a->noise, a->noise ? B * per : 0, T - 1, a->c_recip, a->c_recipm1, a->c1, a->c2, a->post_logvar,
                    partials, vl.nslot};
    const StepArgs step{c.state, c.ws + c.sl.off_eps, per, vlb_rule(v)};

    // one step: x_t = q_sample(x, t, eps), UNet(x_t, t) with the counter bookkeeping of a reverse step, the VLB epilogue
    auto one_step = [&]() -> int {
        DDK_TRY(vlb_step_input(v, a->sqrt_acp, a->sqrt_1m_acp, c.state, B, per, c.st));
        return c.forward(xt, &step);
    };

    const ChainKey key{StepKind::Vlb,
                       {a->packed, a->x, a->noise, a->sqrt_acp, a->sqrt_1m_acp, a->c_recip, a->c_recipm1, a->c1, a->c2, a->post_logvar},
                       a->workspace, a->noise, B, H, W, T - 1, c.dev, c.u->pack_epoch};
    DDK_TRY(run_chain(*c.u, key, T, a->use_graph != 0, one_step, c.st, "vlb_sweep"));
    return vlb_sweep_finalize(partials, vl.nslot, a->vlb_t, a->l_simple_t, T, B, per, c.st);
}
