"""Python handle on the native UNet plan / sampler of libddk.so (csrc/unet_plan.hip).

The plan is created from the reference config keys (models/unet/unet.py:19-22), tells us which
state_dict tensors it needs (names = reference keys), repacks them into one device arena and then
runs a whole forward -- or the whole T-step sampling loop -- from a single C call.
"""
import contextlib
import ctypes as C
import math
import types
import warnings

import torch

from . import lib as L


def sinusoidal_freqs(dim):
    """The fp32 frequency table of SinusoidalPosEmb (blocks.py:24-26), computed with the same torch
    CPU expression as the reference so the table is bit-identical to its CPU path."""
    half = dim // 2
    step = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half) * -step)


# the sampler entries by workspace kind: (method, chain name in messages, name of the workspace in messages)
SAMPLERS = {"smp": ("sample", "sampler", "sampler"), "sms": ("sample_multistep", "sampler_multistep", "multistep sampler"),
            "sin": ("sample_inpaint", "sampler_inpaint", "inpainting sampler"),
            "srs": ("sample_restore", "sampler_restore", "super-resolution sampler"),
            "srm": ("sample_restore_masked", "sampler_restore_masked", "masked restoration sampler"),
            "srx": ("sample_restore_multistep", "sampler_restore_multistep", "restoration solver"),
            "srn": ("sample_restore_noisy", "sampler_restore_noisy", "noisy restoration sampler"),
            "srg": ("sample_restore_gray", "sampler_restore_gray", "colourisation sampler"),
            "srb": ("sample_restore_blur", "sampler_restore_blur", "deblurring sampler"),
            "srq": ("sample_restore_sep", "sampler_restore_sep", "separable restoration sampler"),
            "src": ("sample_restore_cs", "sampler_restore_cs", "compressed-sensing sampler"),
            "srf": ("sample_restore_fft", "sampler_restore_fft", "deconvolution sampler"),
            "sfn": ("sample_restore_fft_noisy", "sampler_restore_fft_noisy", "noisy deconvolution sampler")}
# workspace kinds whose captured step graphs point into them (the samplers', the likelihood sweep's): UnetPlan._workspace keeps up
# to 3 of each
CHAIN_WORKSPACES = (*SAMPLERS, "vsw")


class UnetPlan:
    def __init__(self, in_ch, chan, mults):
        lib = L.load()
        cfg = L.UnetConfig(in_ch, chan, len(mults), (C.c_int * 8)(*list(mults) + [0] * (8 - len(mults))))
        self._lib = lib
        self.handle = lib.ddk_unet_create(C.byref(cfg))
        if not self.handle:
            raise L.DDKError(f"ddk_unet_create failed: {L.last_error()}")
        self.in_ch, self.chan, self.mults = in_ch, chan, tuple(mults)
        self.slot_names = [lib.ddk_unet_slot_name(self.handle, i).decode() for i in range(lib.ddk_unet_num_slots(self.handle))]
        self.slot_numel = [lib.ddk_unet_slot_numel(self.handle, i) for i in range(len(self.slot_names))]
        self.packed = None
        self._ws = {}          # (kind, nbytes, device) -> tensor; sampler workspaces are kept (LRU of 3): cached graphs point into them
        self._state = {}       # chain state x per (shape, device): a stable address for the captured sampler graph
        self._cluster = 1      # DDK_OPT_CLUSTER_GROUPNORM as last set (the library's default is 1: sampler only)
        self._cluster_dev = None   # whether THIS device can host the in-launch GroupNorm at all (asked once, at the first chain)

    def __deepcopy__(self, memo):
        return None     # a copied module (EMA) builds its own native plan on first use

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.ddk_unet_destroy(self.handle)    # waits for the device if sampler graphs are cached
                self.handle = None
        except Exception:
            pass

    # ---------------------------------------------------------------- weights
    def pack(self, tensors, device):
        """tensors: mapping reference-key -> fp32 tensor (any device).  Builds the packed arena."""
        lib = self._lib
        nbytes = lib.ddk_unet_packed_bytes(self.handle)
        packed = torch.zeros(nbytes // 4, device=device, dtype=torch.float32)
        keep = []
        for i, name in enumerate(self.slot_names):
            if name == "@sinusoidal_freqs":
                src = sinusoidal_freqs(self.chan)
            else:
                if name not in tensors:
                    raise L.DDKError(f"UNet weight '{name}' missing from the state dict")
                src = tensors[name]
            src = src.detach().to(device=device, dtype=torch.float32).contiguous()
            if src.numel() != self.slot_numel[i]:
                raise L.DDKError(f"UNet weight '{name}': expected {self.slot_numel[i]} elements, got {src.numel()}")
            keep.append(src)
            L.check(lib.ddk_unet_pack_slot(self.handle, i, L.ptr(src), L.ptr(packed), L.stream()), f"pack {name}")
        torch.cuda.current_stream().synchronize()  # sources may be temporaries
        self.packed = packed
        return packed

    # ---------------------------------------------------------------- forward
    def _workspace(self, kind, nbytes, device):
        """Scratch per (kind, size, device).  The sampler keeps up to 3 workspaces (LRU): the captured step graphs and the
        time-shift table live in / point into their workspace, so a trainer that alternates sample() (t_start = T-1) and
        reconstruct() (t_start = t_rec_max) at every logging event keeps both sets of graphs instead of re-capturing twice per event.
        Only an eviction drops the plan's cached graphs (ddk_sampler_invalidate waits for the device).  The likelihood sweep's
        workspaces ("vsw"), the multistep sampler's ("sms"), the inpainting sampler's ("sin"), the super-resolution sampler's
        ("srs"), the masked restoration sampler's ("srm"), the restoration solver's ("srx"), the noisy restoration sampler's ("srn") and the
        colourisation sampler's ("srg") are kept the same way: their captured steps point into them too."""
        key = (kind, nbytes, str(device))
        hit = self._ws.get(key)
        if hit is not None:
            self._ws[key] = self._ws.pop(key)          # most recently used last
            return hit
        if kind in CHAIN_WORKSPACES:
            mine = [k for k in self._ws if k[0] == kind]       # dict order = least recently used first
            if len(mine) >= 3:
                # evict ONLY the least recently used workspace; the plan drops the graphs that point into it (and waits for
                # their launches), the other two keep theirs
                old = self._ws[mine[0]]
                L.check(self._lib.ddk_sampler_release_workspace(self.handle, L.ptr(old)), "sampler_release_workspace")
                del self._ws[mine[0]]
        else:
            for k in [k for k in self._ws if k[0] == kind]:
                del self._ws[k]
        buf = torch.empty(max(nbytes, 16) // 4 + 4, device=device, dtype=torch.float32)
        self._ws[key] = buf
        return buf

    OPT_CLUSTER_GROUPNORM = 1
    OPT_ATTENTION_FOLD = 3
    OPT_FOLD_DOWNSAMPLE_REDUCE = 5
    OPT_ATTENTION_KV_CONTEXT = 6
    OPT_LEVEL_CHAIN = 7
    OPT_FIRST_GROUPNORM = 8
    OPT_RESTORE_FUSED_TAIL = 12
    OPT_ATTENTION_SPLIT = 13
    OPT_SKIP_FOLD = 14
    OPT_ATTENTION_FOLD_PARTIALS = 15

    def set_option(self, option, value):
        """ddk_unet_set_option: e.g. (OPT_CLUSTER_GROUPNORM, 0) keeps conv + GroupNorm-apply as two launches
        (1: in-launch GroupNorm inside the sampler, 2: in single forwards too -- both checked after the call, see below)."""
        L.check(self._lib.ddk_unet_set_option(self.handle, option, int(value)), "unet_set_option")
        if option == self.OPT_CLUSTER_GROUPNORM:
            self._cluster = max(0, min(2, int(value)))

    @contextlib.contextmanager
    def forwards_as_in_chain(self):
        """While open, single forwards choose their kernels as a sampler step does: with the option at its default (1) the chain
        runs the in-launch GroupNorm and a lone forward the two-launch one, whose other summation order moves eps_hat by a few
        1e-6 at the cfg4 shape -- more per step than a Python loop may differ from the native chain over a whole run.  Sets the
        option to 2 (each forward then waits for its own check) and puts 1 back on leaving, unless a failed check has switched the
        option off meanwhile.  Values 0 and 2 already agree with the chain and are left alone.  Setting the option drops the
        plan's cached graphs: this is for the Python loops that tests and debugging compare with the native sampler."""
        raised = self._cluster == 1
        if raised:
            self.set_option(self.OPT_CLUSTER_GROUPNORM, 2)
        try:
            yield
        finally:
            if raised and self._cluster == 2:
                self.set_option(self.OPT_CLUSTER_GROUPNORM, 1)

    def _cluster_failed(self, ws, b, h, w, stream_ptr):
        """ddk_unet_cluster_check at a sync point.  True when an in-launch GroupNorm exchange timed out on `ws` (the GPU was
        shared / masked): the caller restores its input and reruns; the option is switched off for the rest of the process'
        use of this plan, loudly."""
        rc = self._lib.ddk_unet_cluster_check(self.handle, L.ptr(ws), b, h, w, stream_ptr)
        if rc == 0:
            return False
        if rc != L.ERR_CLUSTER:
            L.check(rc, "unet_cluster_check")
        warnings.warn("ddk: " + L.last_error() + " -- switching DDK_OPT_CLUSTER_GROUPNORM off for this plan and rerunning",
                      RuntimeWarning, stacklevel=3)
        self.set_option(self.OPT_CLUSTER_GROUPNORM, 0)
        return True

    def _chain_guarded(self):
        """Whether a chain has to be checked for a failed in-launch GroupNorm.  On a device that never takes that path (masked /
        partitioned: no launch is issued, csrc/unet_plan.hip gates on the same device test) there is nothing to check: no saved
        input, no stream wait behind the chain.  The device is asked once, at the first chain."""
        if self._cluster_dev is None:
            self._cluster_dev = self._lib.ddk_conv3x3_gn_mish_cluster_ok(32, 32, 32, 128, 128, 8) > 0
        return self._cluster >= 1 and self._cluster_dev

    def _run_chain(self, who, call, ws, b, h, w, graphed, restore=None):
        """Issues a chain with call(stream_ptr) on workspace `ws` of a [b, h, w] batch.  With the in-launch GroupNorm on, waits for
        it (the chain's sync point: T steps of work against one stream synchronisation); when it reports a failure, restore()
        puts the chain's input back and the chain runs again with the option off.  A graphed chain (hipGraph capture is illegal
        on the legacy NULL stream) runs on a side stream ordered after the current one."""
        guard = self._chain_guarded()
        for rerun in (False, True):
            if rerun and restore is not None:
                restore()
            if graphed:
                cur = torch.cuda.current_stream()
                side = _side_stream(ws.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    call(side.cuda_stream)
                    failed = guard and self._cluster >= 1 and self._cluster_failed(ws, b, h, w, side.cuda_stream)
                cur.wait_stream(side)
            else:
                call(L.stream())
                failed = guard and self._cluster >= 1 and self._cluster_failed(ws, b, h, w, L.stream())
            if not failed:
                return
        raise L.DDKError(f"{who}: in-launch GroupNorm reported a failure with the option off")

    def cluster_timeouts(self):
        return int(self._lib.ddk_debug_cluster_timeouts())

    def flops(self, b, h, w):
        return self._lib.ddk_unet_flops(self.handle, b, h, w)

    def flops_executed(self, b, h, w):
        """FLOPs the dispatched kernels issue (Winograd convs: 16/36 of the direct multiplies)."""
        return self._lib.ddk_unet_flops_executed(self.handle, b, h, w)

    def forward_nhwc(self, x, t):
        """x [B,H,W,in_ch] fp32, t [B] int64 -> eps_hat [B,H,W,in_ch]."""
        if self.packed is None:
            raise L.DDKError("UnetPlan.forward before pack()")
        b, h, w, c = x.shape
        if c != self.in_ch:
            raise L.DDKError(f"expected {self.in_ch} input channels, got {c}")
        if t.dtype != torch.int64:
            raise L.DDKError("timesteps must be int64")
        lib = self._lib
        nbytes = lib.ddk_unet_workspace_bytes(self.handle, b, h, w)
        if nbytes == 0:
            raise L.DDKError(f"unet workspace query failed: {L.last_error()}")
        ws = self._workspace("fwd", nbytes, x.device)
        out = torch.empty_like(x)
        for _ in range(2):
            L.check(lib.ddk_unet_forward(self.handle, L.ptr(self.packed), L.ptr(x), L.ptr(t), L.ptr(out), b, h, w,
                                         L.ptr(ws), nbytes, L.stream()), "unet_forward")
            # option value 2 only (tests / diagnostics): a single forward has no sync point of its own, so this one waits
            if self._cluster < 2 or not self._cluster_failed(ws, b, h, w, L.stream()):
                break
        return out

    # ---------------------------------------------------------------- sampler
    def _need_packed(self, kind):
        if self.packed is None:
            raise L.DDKError(f"UnetPlan.{SAMPLERS[kind][0]} before pack()")

    def _run_sampler(self, kind, x, t_start, t_end, bytes_query, call, use_graph):
        """What the sampler entries share once their own arguments are checked: steps t_start .. t_end in place on x [B,H,W,in_ch].
        kind: the entry's key in SAMPLERS, also its workspace kind; bytes_query(b, h, w): its workspace size query;
        call(x, ws, nbytes, stream_ptr): the C call, x being the buffer the chain runs on (_chain_x)."""
        _, who, label = SAMPLERS[kind]
        b, h, w, _ = x.shape
        nbytes = bytes_query(b, h, w)
        if nbytes == 0:
            raise L.DDKError(f"{label} workspace query failed: {L.last_error()}")
        ws = self._workspace(kind, nbytes, x.device)
        caller_x, x = x, self._chain_x(x)
        # the in-launch GroupNorm can fail (loudly) when the GPU is shared: keep x_T so the chain can be rerun without it
        x_start = x.clone() if self._chain_guarded() else None
        self._run_chain(who, lambda stream_ptr: call(x, ws, nbytes, stream_ptr), ws, b, h, w, use_graph and t_start - t_end + 1 > 1,
                        restore=lambda: x.copy_(x_start))
        if caller_x.data_ptr() != x.data_ptr():
            caller_x.copy_(x)
        return caller_x

    @staticmethod
    def _timestep_map(timesteps, t_start):
        if timesteps is None:
            return None
        if len(timesteps) != t_start + 1:
            raise L.DDKError(f"timestep map must have t_start + 1 = {t_start + 1} entries, got {len(timesteps)}")
        return (C.c_int64 * len(timesteps))(*[int(v) for v in timesteps])

    def _sampler_args(self, x, noise, tables, t_start, t_end, seed, stream_id, use_graph, ws, nbytes):
        b, h, w, _ = x.shape
        return L.SamplerArgs(self.handle, L.ptr(self.packed), L.ptr(x), L.ptr(noise), L.ptr(tables["c_recip"]),
                             L.ptr(tables["c_recipm1"]), L.ptr(tables["c1"]), L.ptr(tables["c2"]), L.ptr(tables.get("sigma")),
                             b, h, w, t_start, t_end, seed, stream_id, int(use_graph), L.ptr(ws), nbytes)

    def sample_nhwc(self, x, tables, t_start, t_end=0, noise=None, seed=0, stream_id=0, use_graph=True, timesteps=None):
        """Run steps t_start .. t_end (inclusive) of the reverse chain in place on x [B,H,W,in_ch].

        tables: dict with c_recip, c_recipm1, c1, c2, sigma ([T] fp32 device tensors).
        noise: optional [n_steps,B,H,W,in_ch] injected draws (parity tests); else in-kernel Philox.
        timesteps: optional timestep map of a respaced / DDIM chain (t_start + 1 ints, map[0] == 0, increasing): step k runs
        the UNet at timesteps[k] while the tables and the Philox draws are indexed by k (ddk_sampler_run_spaced).
        """
        self._need_packed("smp")
        lib = self._lib
        tmap = self._timestep_map(timesteps, t_start)
        n_steps = t_start - t_end + 1
        if noise is not None and tuple(noise.shape) != (n_steps, *x.shape):
            raise L.DDKError(f"injected noise must be {(n_steps, *x.shape)}, got {tuple(noise.shape)}")

        def call(x, ws, nbytes, stream_ptr):
            a = self._sampler_args(x, noise, tables, t_start, t_end, seed, stream_id, use_graph, ws, nbytes)
            if tmap is None:
                L.check(lib.ddk_sampler_run(C.byref(a), stream_ptr), "sampler_run")
            else:
                L.check(lib.ddk_sampler_run_spaced(C.byref(a), tmap, stream_ptr), "sampler_run_spaced")

        return self._run_sampler("smp", x, t_start, t_end,
                                 lambda b, h, w: lib.ddk_sampler_workspace_bytes(self.handle, b, h, w, t_start), call, use_graph)

    def _chain_x(self, x):
        """The buffer a sampler chain runs on.  The captured graph holds the ADDRESS of the chain state.  A caller that keeps
        passing the same tensor (bench, a serving loop) is run in place; once a different address shows up for this shape
        (p_sample_loop builds a fresh tensor per call) the chain moves to a plan-owned state buffer, so later calls hit the
        cached graph again."""
        skey = (tuple(x.shape), str(x.device))
        mode = self._state.get(skey)
        if mode is None:
            mode = self._state[skey] = {"ptr": x.data_ptr(), "buf": None}
        if mode["buf"] is None and mode["ptr"] != x.data_ptr():
            mode["buf"] = torch.empty_like(x)
        if mode["buf"] is not None:
            mode["buf"].copy_(x)
            return mode["buf"]
        return x

    def sample_multistep_nhwc(self, x, tables, t_start, t_end=0, stream_id=0, use_graph=True, timesteps=None):
        """DPM-Solver++(2M) steps t_start .. t_end (inclusive) in place on x [B,H,W,in_ch] (ddk_sampler_run_multistep).

        tables: dict with c_recip, c_recipm1, c1, c2, c3 (K-row fp32 device tensors of models/diffusion/respace.py
        dpm_solver_tables; c3[t_start] == 0).  timesteps: the chain's timestep map (t_start + 1 ints, map[0] == 0, increasing) or
        None for the identity.  Deterministic: no noise, no seed.  The solver's history lives in the plan's "sms" workspace and is
        zeroed by every call."""
        self._need_packed("sms")
        lib = self._lib
        tmap = self._timestep_map(timesteps, t_start)

        def call(x, ws, nbytes, stream_ptr):
            a = self._sampler_args(x, None, tables, t_start, t_end, 0, stream_id, use_graph, ws, nbytes)
            L.check(lib.ddk_sampler_run_multistep(C.byref(a), tmap, L.ptr(tables["c3"]), stream_ptr), "sampler_run_multistep")

        return self._run_sampler("sms", x, t_start, t_end,
                                 lambda b, h, w: lib.ddk_sampler_multistep_workspace_bytes(self.handle, b, h, w, t_start), call, use_graph)

    def sample_inpaint_nhwc(self, x, known, mask, tables, timesteps, t_end=0, seed=0, stream_id=0, use_graph=True):
        """RePaint ops N-1 .. t_end (inclusive) in place on x [B,H,W,in_ch] (ddk_sampler_run_inpaint).

        known, mask: [B,H,W,in_ch] fp32 device tensors (mask nonzero = known), copied into the plan's "sin" workspace by every call,
        so a loop over images replays one cached graph.  tables: dict with c_recip, c_recipm1, c1, c2, sigma, ka, kb, ja, jb (N-row
        fp32 device tensors of models/diffusion/respace.py repaint_tables).  timesteps: the N-entry timestep map (map[0] == 0, not
        monotone).  Philox only: no injected noise; stream_id < 2^29."""
        self._need_packed("sin")
        b, h, w, c = x.shape
        for name, v in (("known", known), ("mask", mask)):
            if tuple(v.shape) != (b, h, w, c) or v.dtype != torch.float32 or not v.is_contiguous():
                raise L.DDKError(f"{name} must be a contiguous fp32 [{b},{h},{w},{c}] tensor, got {tuple(v.shape)} {v.dtype}")
        lib = self._lib
        n_ops = len(timesteps)
        t_start = n_ops - 1
        tmap = (C.c_int64 * n_ops)(*[int(v) for v in timesteps])

        def call(x, ws, nbytes, stream_ptr):
            a = self._sampler_args(x, None, tables, t_start, t_end, seed, stream_id, use_graph, ws, nbytes)
            ip = L.InpaintArgs(tmap, L.ptr(known), L.ptr(mask), L.ptr(tables["ka"]), L.ptr(tables["kb"]), L.ptr(tables["ja"]),
                               L.ptr(tables["jb"]))
            L.check(lib.ddk_sampler_run_inpaint(C.byref(a), C.byref(ip), stream_ptr), "sampler_run_inpaint")

        return self._run_sampler("sin", x, t_start, t_end,
                                 lambda b, h, w: lib.ddk_sampler_inpaint_workspace_bytes(self.handle, b, h, w, n_ops), call, use_graph)

    # the restoration samplers (DDNM; DESIGN.md sections 3.6, 3.8 - 3.11): the C entries of each workspace kind (run, workspace query, tail query), less their ddk_ prefix
    RESTORE_ENTRIES = {
        "srs": ("sampler_run_restore", "sampler_restore_workspace_bytes", "sampler_restore_tail_parts"),
        "srm": ("sampler_run_restore_masked", "sampler_restore_masked_workspace_bytes", "sampler_restore_masked_tail_parts"),
        "srx": ("sampler_run_restore_multistep", "sampler_restore_multistep_workspace_bytes",
                "sampler_restore_multistep_tail_parts"),
        "srn": ("sampler_run_restore_noisy", "sampler_restore_noisy_workspace_bytes", "sampler_restore_noisy_tail_parts"),
        "srg": ("sampler_run_restore_gray", "sampler_restore_gray_workspace_bytes", "sampler_restore_gray_tail_parts"),
        "srb": ("sampler_run_restore_blur", "sampler_restore_blur_workspace_bytes", "sampler_restore_blur_tail_parts"),
        # the size-changing entry is the deblurring chain with a y of its own size: its workspace and tail queries serve both
        "srq": ("sampler_run_restore_sep", "sampler_restore_blur_workspace_bytes", "sampler_restore_blur_tail_parts"),
        "src": ("sampler_run_restore_cs", "sampler_restore_cs_workspace_bytes", "sampler_restore_cs_tail_parts"),
        "srf": ("sampler_run_restore_fft", "sampler_restore_fft_workspace_bytes", "sampler_restore_fft_tail_parts"),
        "sfn": ("sampler_run_restore_fft_noisy", "sampler_restore_fft_noisy_workspace_bytes", "sampler_restore_fft_noisy_tail_parts")}

    # What each entry takes, keyed like RESTORE_ENTRIES.  q holds b, h, w, c of x, n, the rows of the chain and what `derive` adds.
    #   blocks: the block sizes n of a block kind; mask_at_1: its n = 1 needs a mask; gray: the grey entry (3 channels, weights, y [B,H/n,W/n])
    #   grid:   (test of H and of W, its words): the shape rule of a plane-wide kind, which has no block and no mask of pixels
    #   derive: (q, y, given) -> what the entry reads off its operands; also: q -> None or what is wrong with that, checked behind grid
    #   ops:    the named extra operands as (name, shape of q, dtype): contiguous tensors on x's device; y: the shape of y
    #   order:  how the C entry takes y, the operands and the integers of q, behind the tables of `head`; n_query: the workspace query takes n
    _F, _I = torch.float32, torch.int32
    _POW2, _MULT16 = (lambda v: v & (v - 1) == 0, "powers of two"), (lambda v: v % 16 == 0, "multiples of 16")
    _BLOCK_Y, _FULL_Y = (lambda q: (q.b, q.h // q.n, q.w // q.n, q.c)), (lambda q: (q.b, q.h, q.w, q.c))
    _MASKED = dict(blocks=(1, 2, 4, 8), mask_at_1=True, y=_BLOCK_Y, order=("y", "mask", "n"), n_query=True)
    _SEP = dict(grid=_MULT16, y=lambda q: (q.b, q.yh, q.yw, q.c),
                also=lambda q: None if q.yh % 4 == 0 and q.yw % 4 == 0 and 4 <= q.yh <= q.h and 4 <= q.yw <= q.w else
                f"y's size must be multiples of 4 in [4, {q.h}] and [4, {q.w}], got {q.yh} x {q.yw}",
                ops=(("P_h", lambda q: (q.h, q.h), _F), ("P_w", lambda q: (q.w, q.w), _F), ("Q_h", lambda q: (q.h, q.yh), _F),
                     ("Q_w", lambda q: (q.w, q.yw), _F)))
    _FFT_OPS = (("mask", lambda q: (q.h, q.w), _F), ("P", lambda q: (q.h, q.w, 2), _F), ("gain", lambda q: (q.h, q.w), _F),
                ("nsc", lambda q: (q.rows,), _F))
    RESTORE_OPS = {
        "srs": dict(blocks=(2, 4, 8), y=_BLOCK_Y, order=("y", "n")),
        "srm": _MASKED, "srx": _MASKED, "srn": _MASKED,
        "srg": dict(blocks=(1, 2, 4, 8), gray=True, y=lambda q: (q.b, q.h // q.n, q.w // q.n), order=("y", "mask", "n", "weights"), n_query=True),
        "srb": dict(_SEP, derive=lambda q, y, g: dict(yh=q.h, yw=q.w), order=("P_h", "P_w", "Q_h", "Q_w", "y")),
        "srq": dict(_SEP, order=("P_h", "P_w", "Q_h", "Q_w", "y", "yh", "yw"),      # a size of 0: refused by `also`
                    derive=lambda q, y, g: dict(zip(("yh", "yw"), (int(v.shape[1]) if v is not None and v.dim() == 2 else 0
                                                                   for v in (g["Q_h"], g["Q_w"]))))),
        "src": dict(grid=_POW2, y=lambda q: (q.b, q.c, q.m), ops=(("perm", lambda q: (q.h * q.w,), _I),), order=("y", "perm", "m"),
                    derive=lambda q, y, g: dict(m=int(y.shape[2]) if y is not None and y.dim() == 3 else 0),      # 0: refused by `also`
                    also=lambda q: None if isinstance(q.m, int) and 4 <= q.m <= q.h * q.w and q.m % 4 == 0 else
                    f"m must be a multiple of 4 in [4, {q.h * q.w}], got {q.m!r}"),
        "srf": dict(grid=_POW2, y=_FULL_Y, ops=_FFT_OPS[:2], order=("mask", "P", "twiddles", "y")),
        "sfn": dict(grid=_POW2, y=_FULL_Y, ops=_FFT_OPS, order=("mask", "P", "gain", "nsc", "twiddles", "y"))}

    def _restore_tail_parts(self, kind, b, h, w, n=None):
        return int(getattr(self._lib, "ddk_" + self.RESTORE_ENTRIES[kind][2])(self.handle, b, h, w, *(() if n is None else (int(n),))))

    def _sample_restore(self, kind, x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, head=(), n=1, **given):
        """What the restoration samplers share: one walk over the entry's description in RESTORE_OPS -- the checks on the shape, n, the
        named operands, y, the mask and the tables, then the chain.  kind: the entry's key in SAMPLERS, RESTORE_ENTRIES and
        RESTORE_OPS; head: the names of the tables the C entry takes before its operands; given: the entry's other operands by name."""
        self._need_packed(kind)
        name, d = SAMPLERS[kind][0], self.RESTORE_OPS[kind]
        b, h, w, c = x.shape
        mask = None if "grid" in d else given.get("mask")      # (a plane-wide kind's "mask" is one of its ops: of frequencies, not of pixels)
        q = types.SimpleNamespace(b=b, h=h, w=w, c=c, n=n, rows=t_start + 1)
        q.__dict__.update(d["derive"](q, y, given) if "derive" in d else {})
        if "grid" in d:
            ok, words = d["grid"]
            if not (ok(h) and ok(w) and 16 <= h <= 256 and 16 <= w <= 256 and 1 <= c <= 8):
                raise L.DDKError(f"{name}: H and W must be {words} in [16, 256] and the channels 1 to 8, got [{h},{w},{c}]")
            if "also" in d and d["also"](q):
                raise L.DDKError(f"{name}: {d['also'](q)}")
            for what, shape, dtype in d["ops"]:
                v, shape = given[what], shape(q)
                if v is None or tuple(v.shape) != shape or v.dtype != dtype or not v.is_contiguous() or v.device != x.device:
                    raise L.DDKError(f"{name}: {what} must be a contiguous {'fp32' if dtype == self._F else 'int32'} "
                                     f"[{','.join(map(str, shape))}] tensor on x's device")
        else:
            if d.get("gray") and c != 3:
                raise L.DDKError(f"{name}: the grey operator needs a 3-channel map, got {c} channels")
            if d.get("gray") and given["weights"] not in L.GRAY_WEIGHTS:
                raise L.DDKError(f"{name}: weights must be 'mean' or 'luma', got {given['weights']!r}")
            if n not in d["blocks"] or h % n or w % n:
                raise L.DDKError(f"{name}: n must be {'1, ' if 1 in d['blocks'] else ''}2, 4 or 8 and divide H = {h} and W = {w}, got {n}")
            if mask is None and n == 1 and d.get("mask_at_1"):
                raise L.DDKError(f"{name}: n = 1 needs a mask (nothing would be constrained)")
        for what, v, shape in (("y", y, d["y"](q)), ("mask", mask, (b, h // n, w // n))):
            if v is not None and (tuple(v.shape) != shape or v.dtype != torch.float32 or not v.is_contiguous()):
                raise L.DDKError(f"{what} must be a contiguous fp32 [{','.join(map(str, shape))}] tensor, got {tuple(v.shape)} {v.dtype}")
        for t in head:
            if t != "c3" and (tuple(tables[t].shape) != tuple(tables["c1"].shape) or tables[t].dtype != torch.float32):      # c3: the solver's own
                raise L.DDKError(f"tables[{t!r}] must be an fp32 tensor with one entry per row of c1, got {tuple(tables[t].shape)}")
        run_name = self.RESTORE_ENTRIES[kind][0]
        run, workspace_bytes = (getattr(self._lib, "ddk_" + f) for f in self.RESTORE_ENTRIES[kind][:2])
        tmap = self._timestep_map(timesteps, t_start)
        given["y"] = y
        if "twiddles" in d["order"]:
            from . import ops
            given["twiddles"] = ops.fft_twiddles(max(h, w), x.device)
        operands = tuple(L.GRAY_WEIGHTS[given[o]] if o == "weights" else int(getattr(q, o)) if hasattr(q, o) else L.ptr(given[o])
                         for o in d["order"])

        def call(x, ws, nbytes, stream_ptr):
            a = self._sampler_args(x, None, tables, t_start, t_end, seed, stream_id, use_graph, ws, nbytes)
            L.check(run(C.byref(a), tmap, *(L.ptr(tables[t]) for t in head), *operands, stream_ptr), run_name)

        return self._run_sampler(kind, x, t_start, t_end,
                                 lambda b, h, w: workspace_bytes(self.handle, b, h, w, t_start, *((int(n),) if d.get("n_query") else ())), call,
                                 use_graph)

    def restore_tail_parts(self, b, h, w, n):
        """Tiles per image of the fused tail of a super-resolution step on [b, h, w] with block n, or 0: the unfused tail."""
        return self._restore_tail_parts("srs", b, h, w, n)

    def sample_restore_nhwc(self, x, y, n, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True, timesteps=None):
        """DDNM super-resolution steps t_start .. t_end (inclusive) in place on x [B,H,W,in_ch] (ddk_sampler_run_restore; DESIGN.md
        section 3.6).

        y: [B,H/n,W/n,in_ch] fp32 device tensor, copied into the plan's "srs" workspace by every call, so a loop over images replays
        one cached graph; n in {2, 4, 8} divides H and W.  tables / timesteps: as for sample_nhwc (plain, respaced or DDIM).
        Philox only: no injected noise."""
        return self._sample_restore("srs", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, n=n)

    def restore_masked_tail_parts(self, b, h, w, n):
        """Tiles per image of the fused tail of a masked restoration step on [b, h, w] with block n (1 included), or 0."""
        return self._restore_tail_parts("srm", b, h, w, n)

    def sample_restore_masked_nhwc(self, x, y, mask, n, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True, timesteps=None):
        """DDNM steps for A = mask o (n x n average pooling), t_start .. t_end (inclusive), in place on x [B,H,W,in_ch]
        (ddk_sampler_run_restore_masked).

        y: [B,H/n,W/n,in_ch], mask: [B,H/n,W/n] (nonzero = measured) fp32 device tensors, copied into the plan's "srm" workspace by
        every call, so a loop over images and masks replays one cached graph; n in {1, 2, 4, 8} divides H and W.  mask None (n >= 2
        only) is sample_restore_nhwc's chain.  tables / timesteps: as for sample_nhwc (plain, respaced or DDIM).  Philox only."""
        return self._sample_restore("srm", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, n=n, mask=mask)

    def restore_multistep_tail_parts(self, b, h, w, n):
        """Tiles per image of the fused tail of a restoration-solver step on [b, h, w] with block n (1 included), or 0."""
        return self._restore_tail_parts("srx", b, h, w, n)

    def sample_restore_multistep_nhwc(self, x, y, mask, n, tables, t_start, t_end=0, stream_id=0, use_graph=True, timesteps=None):
        """DDNM for A = mask o (n x n average pooling) on DPM-Solver++(2M) steps t_start .. t_end (inclusive), in place on x
        [B,H,W,in_ch] (ddk_sampler_run_restore_multistep).

        y, mask, n: as for sample_restore_masked_nhwc (mask None at n >= 2: every block measured); they are copied into the plan's
        "srx" workspace by every call, so a loop over images and masks replays one cached graph.  tables / timesteps: as for
        sample_multistep_nhwc.  Deterministic: no noise, no seed; the history is zeroed by every call."""
        return self._sample_restore("srx", x, y, tables, t_start, t_end, 0, stream_id, use_graph, timesteps, head=("c3",), n=n, mask=mask)

    def restore_noisy_tail_parts(self, b, h, w, n):
        """Tiles per image of the fused tail of a noisy restoration step on [b, h, w] with block n (1 included), or 0."""
        return self._restore_tail_parts("srn", b, h, w, n)

    def sample_restore_noisy_nhwc(self, x, y, mask, n, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True, timesteps=None):
        """DDNM+ steps for a noisy measurement of A = mask o (n x n average pooling), t_start .. t_end (inclusive), in place on x
        [B,H,W,in_ch] (ddk_sampler_run_restore_noisy).

        y, mask, n: as for sample_restore_masked_nhwc (mask None at n >= 2: every block measured); they are copied into the plan's
        "srn" workspace by every call.  tables: sample_restore_masked_nhwc's plus the per-row "lam" and "sgm" (respace.noisy_tables);
        they are in the graph key, so chains with different noise levels never replay each other's graph.  Philox only."""
        return self._sample_restore("srn", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, head=("lam", "sgm"), n=n, mask=mask)

    def restore_gray_tail_parts(self, b, h, w, n):
        """Tiles per image of the fused tail of a colourisation step on [b, h, w] with block n (1 included), or 0 (always 0 for a
        model that does not have 3 channels)."""
        return self._restore_tail_parts("srg", b, h, w, n)

    def sample_restore_gray_nhwc(self, x, y, mask, n, weights, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True,
                                 timesteps=None):
        """DDNM / DDNM+ steps for a grey measurement, A = mask o (n x n average pooling) o grey_w, t_start .. t_end (inclusive), in
        place on x [B,H,W,3] (ddk_sampler_run_restore_gray).

        y, mask: contiguous fp32 [B,H/n,W/n] (mask None: every block measured, at any n); weights "mean" or "luma"; they are copied
        into the plan's "srg" workspace by every call.  tables: sample_restore_noisy_nhwc's, "lam" and "sgm" included
        (respace.gray_tables); the tables, n, the mask's presence and the weights are in the graph key.  Philox only."""
        return self._sample_restore("srg", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, head=("lam", "sgm"), n=n, mask=mask,
                                    weights=weights)

    def restore_blur_tail_parts(self, b, h, w):
        """Tiles per image of the fused tail of a deblurring step on [b, h, w]: 0 for every shape (the operator couples a whole
        plane, the tail owns 128-pixel tiles), -1 for a shape the plan does not take."""
        return self._restore_tail_parts("srb", b, h, w)

    def sample_restore_blur_nhwc(self, x, y, P_h, P_w, Q_h, Q_w, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True,
                                 timesteps=None):
        """DDNM deblurring steps for a separable blur A(X) = A_h X A_w^T, t_start .. t_end (inclusive), in place on x [B,H,W,in_ch]
        (ddk_sampler_run_restore_blur).

        y: the blurred image, contiguous fp32 [B,H,W,in_ch]; P_h, Q_h [H,H] and P_w, Q_w [W,W]: the fp32 projections and truncated
        pseudo-inverses of the two axes (models/diffusion/blur.py blur_operands).  P_h and P_w are copied into the plan's "srb"
        workspace and Yp = Q_h y Q_w^T is formed there by every call, so a loop over images replays one cached graph.  H and W
        multiples of 16 in [16, 256].  tables / timesteps: as for sample_nhwc (plain, respaced or DDIM).  Philox only."""
        return self._sample_restore("srb", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, P_h=P_h, P_w=P_w, Q_h=Q_h, Q_w=Q_w)

    def sample_restore_sep_nhwc(self, x, y, P_h, P_w, Q_h, Q_w, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True,
                                timesteps=None):
        """DDNM steps for a size-changing separable operator A(X) = A_h X A_w^T, A_h [h,H] and A_w [w,W] (antialiased bicubic
        reduction, blur-then-decimate), t_start .. t_end (inclusive), in place on x [B,H,W,in_ch] (ddk_sampler_run_restore_sep;
        DESIGN.md section 3.15).

        y: the measurement, contiguous fp32 [B,h,w,in_ch]; P_h [H,H], P_w [W,W], Q_h [H,h], Q_w [W,w]: the fp32 projections and
        pseudo-inverses of the two axes (models/diffusion/blur.py separable_operands).  The steps are sample_restore_blur_nhwc's;
        Yp = Q_h y Q_w^T is formed in the plan's "srq" workspace by every call, so a loop over images replays one cached graph.
        H and W multiples of 16 in [16, 256], h and w multiples of 4 in [4, H] and [4, W].  Philox only."""
        return self._sample_restore("srq", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, P_h=P_h, P_w=P_w, Q_h=Q_h, Q_w=Q_w)

    def restore_cs_tail_parts(self, b, h, w):
        """Tiles per image of the fused tail of a compressed-sensing step on [b, h, w]: 0 for every shape (the operator couples a
        whole plane), -1 for a shape the plan does not take."""
        return self._restore_tail_parts("src", b, h, w)

    def sample_restore_cs_nhwc(self, x, y, perm, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True, timesteps=None):
        """DDNM compressed-sensing steps, A = the first m rows of the orthonormal Walsh-Hadamard transform of each permuted plane,
        t_start .. t_end (inclusive), in place on x [B,H,W,in_ch] (ddk_sampler_run_restore_cs).

        y: the measurements, contiguous fp32 [B,in_ch,m] (m is read from it); perm: contiguous int32 [H*W] on x's device, a
        permutation of the pixels (models/diffusion/hadamard.py cs_perm).  Both are copied into the plan's "src" workspace by every
        call, so a loop over images replays one cached graph.  H and W powers of two in [16, 256], m a multiple of 4 in [4, H*W].
        tables / timesteps: as for sample_nhwc (plain, respaced or DDIM).  Philox only."""
        return self._sample_restore("src", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, perm=perm)

    def restore_fft_tail_parts(self, b, h, w):
        """Tiles per image of the fused tail of a deconvolution step on [b, h, w]: 0 for every shape (the operator couples a whole
        plane), -1 for a shape the plan does not take."""
        return self._restore_tail_parts("srf", b, h, w)

    def sample_restore_fft_nhwc(self, x, y, mask, P, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True, timesteps=None):
        """DDNM deconvolution steps, A = circular convolution with a 2-D point-spread function, t_start .. t_end (inclusive), in
        place on x [B,H,W,in_ch] (ddk_sampler_run_restore_fft).

        y: the blurred images, contiguous fp32 with x's shape; mask: fp32 [H,W], 1 at the kept frequencies; P: fp32 [H,W,2], the
        truncated reciprocal spectrum (models/diffusion/psf.py psf_operands).  Mask and twiddles are copied into the plan's "srf"
        workspace and Yp = A+ y is formed there by every call, so a loop over images replays one cached graph.  H and W powers of two
        in [16, 256].  tables / timesteps: as for sample_nhwc (plain, respaced or DDIM).  Philox only."""
        return self._sample_restore("srf", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, mask=mask, P=P)

    def restore_fft_noisy_tail_parts(self, b, h, w):
        """As restore_fft_tail_parts, for the noisy deconvolution step: 0 for every shape, -1 for a shape the plan does not take."""
        return self._restore_tail_parts("sfn", b, h, w)

    def sample_restore_fft_noisy_nhwc(self, x, y, mask, P, gain, nsc, tables, t_start, t_end=0, seed=0, stream_id=0, use_graph=True,
                                      timesteps=None):
        """DDNM+ deconvolution steps for a blurred image with noise of standard deviation sigma_y, t_start .. t_end (inclusive), in
        place on x [B,H,W,in_ch] (ddk_sampler_run_restore_fft_noisy).

        y, mask, P: as sample_restore_fft_nhwc; gain: fp32 [H,W], 1 / |K^| at the kept frequencies and 0 elsewhere; nsc: fp32
        [t_start + 1], |c1| sigma_y per row (models/diffusion/psf.py psf_noisy_operands).  All are copied into the plan's "sfn"
        workspace and the spectrum of A+ y is formed there by every call.  The cached graph is keyed by the gain and nsc tensors:
        pass the same tensors to replay it.  tables / timesteps: as for sample_nhwc (respaced ancestral, or DDIM with eta > 0).
        Philox only."""
        return self._sample_restore("sfn", x, y, tables, t_start, t_end, seed, stream_id, use_graph, timesteps, mask=mask, P=P, gain=gain,
                                    nsc=nsc)

    # ---------------------------------------------------------------- likelihood sweep
    VLB_STREAM_BIT = 1 << 31     # the sweep's Philox stream id is stream_id | this (csrc/ddk_internal.h VLB_STREAM_BIT)

    def vlb_sweep_nhwc(self, x, tables, T, noise=None, seed=0, stream_id=0, use_graph=True):
        """test_losses_ sweep t = T-1 .. 0 on the clean sample x [B,H,W,in_ch] (not written).

        tables: dict with sqrt_acp, sqrt_1m_acp, c_recip, c_recipm1, c1, c2, post_logvar ([T] fp32 device tensors).
        noise: optional [T,B,H,W,in_ch] injected draws (draw k at t = T-1-k); else in-kernel Philox on (seed, stream_id | 2^31).
        Returns (vlb_t [B,T] in bits/dim, L_simple_t [T]), columns in the reference's order (k = T-1-t).
        """
        if self.packed is None:
            raise L.DDKError("UnetPlan.vlb_sweep before pack()")
        b, h, w, c = x.shape
        if c != self.in_ch:
            raise L.DDKError(f"expected {self.in_ch} input channels, got {c}")
        if not 0 <= int(stream_id) < self.VLB_STREAM_BIT:
            raise L.DDKError("vlb_sweep: stream_id must be in [0, 2^31)")
        if noise is not None and tuple(noise.shape) != (T, b, h, w, c):
            raise L.DDKError(f"injected noise must be {(T, b, h, w, c)}, got {tuple(noise.shape)}")
        lib = self._lib
        nbytes = lib.ddk_vlb_sweep_workspace_bytes(self.handle, b, h, w, T)
        if nbytes == 0:
            raise L.DDKError(f"vlb_sweep workspace query failed: {L.last_error()}")
        ws = self._workspace("vsw", nbytes, x.device)
        # the captured step holds the ADDRESS of x: a plan-owned copy per shape keeps it stable across batches
        skey = ("vsw", tuple(x.shape), str(x.device))
        xs = self._state.get(skey)
        if xs is None:
            xs = self._state[skey] = torch.empty_like(x)
        xs.copy_(x)
        vlb_t = torch.empty((b, T), device=x.device, dtype=torch.float32)
        l_simple_t = torch.empty((T,), device=x.device, dtype=torch.float32)

        def call(stream_ptr):
            a = L.VlbSweepArgs(self.handle, L.ptr(self.packed), L.ptr(xs), L.ptr(noise), L.ptr(tables["sqrt_acp"]),
                               L.ptr(tables["sqrt_1m_acp"]), L.ptr(tables["c_recip"]), L.ptr(tables["c_recipm1"]), L.ptr(tables["c1"]),
                               L.ptr(tables["c2"]), L.ptr(tables["post_logvar"]), b, h, w, T, seed, stream_id, int(use_graph),
                               L.ptr(ws), nbytes, L.ptr(vlb_t), L.ptr(l_simple_t))
            L.check(lib.ddk_vlb_sweep_run(C.byref(a), stream_ptr), "vlb_sweep_run")

        self._run_chain("vlb_sweep", call, ws, b, h, w, use_graph and T > 1)     # x is only read: a rerun needs no restore
        return vlb_t, l_simple_t


_side_streams = {}


def _side_stream(device):
    key = str(device)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]
