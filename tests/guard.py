"""Guard bands: parity and the buffer-contents table say what a kernel computes and what it reads before writing, not WHERE it stores,
nor whether a result depends on bytes beside an input.  torch's caching allocator rounds every block to 512 bytes and puts unrelated
blocks side by side, so a short overrun lands in slack or in a free cached block and nothing notices.  `guard_bands(word)` makes every
tensor the wrappers allocate, and every input moved to the device, an INTERIOR VIEW of a larger allocation

    [ band | tensor | band ]

whose bands hold the repeating 32-bit `word` (tests/poison.py's words).  A store outside the tensor changes a band; a result that
depends on what lies beside an input changes with the word.  One word cannot show everything (a stray store of 0.0 is invisible in a
band of zeros), hence three.

Band width.  Each band is at least twice the largest block a single workgroup of any kernel in csrc/ stores in one pass, so that a
workgroup that is one whole tile (or one record row, or one slab row) off still lands inside a band.  From the kernels' constants:

    im2col / halo convs   conv_igemm.hip   tiles up to 128 pixels x 128 channels x 4 B (T128x128, HALO_BN = 128)           64 KiB
    Winograd convs        conv_wino.hip    WBT = 32 tiles of 2 x 2 pixels x WBN = 64 channels (conv_wino2_kernel.inc and
                                           conv_winoT_kernel.inc: WT_NT = 128 channels) x 4 B                                64 KiB
                                           (the same 128 pixels over every channel of the widest layer, 256, would be      128 KiB)
    one-launch Blocks     conv_local.hip   H W = 64 pixels (conv_gn_wlocal_ok / conv_gn_local_ok) x 32 channels (the grid is
                                           B x N / 32 workgroups) x 4 B                                                       8 KiB
    manifold / MMD        manifold.hip     MF_TILE = 128: results per row, far below a tile of 128 x 128 x 4 B               64 KiB
    FFT plane form        fft_conv.hip     FC_PLANE_MAX = 16384 complex elements x 8 B, the whole plane of LDS              128 KiB
    Hadamard plane form   hadamard.hip     CS_PLANE_MAX = 32768 floats x 4 B                                                128 KiB

No workgroup can hold more than the CU's 160 KiB of LDS, and none stores more than 128 KiB in a pass: BAND = 2 x 128 KiB = 256 KiB
per side.  (The plane-form kernels store their plane with the channel stride of an NHWC image; what they store is at most 128 KiB, the
span it is spread over can be larger.  A store further out than a band is not seen: DESIGN.md says so.)  The width is a property of the
kernels, not a number to tune.

Offsets in a violation are relative to the interior: side "after" counts from the first byte past the tensor's end (0, 1, ...), side
"before" counts down from the byte just before its start (-1, -2, ...); first <= last on both sides."""
import collections
import os
import sys

import torch

import poison

BAND = 256 * 1024
ALIGN = 512
_HERE = os.path.abspath(__file__)
_TORCH = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep

Violation = collections.namedtuple("Violation", "site shape dtype side nbytes first last")
_Record = collections.namedtuple("_Record", "base off span site shape dtype kind")


class GuardError(AssertionError):
    """raised on exit from a block whose bands were written; .violations is the list g.check() returned"""

    def __init__(self, violations):
        super().__init__("bytes outside a tensor were written:\n" + "\n".join(map(format_violation, violations)))
        self.violations = violations


def format_violation(v):
    return (f"  {v.side} {tuple(v.shape)} {v.dtype} allocated at {v.site}: {v.nbytes} damaged bytes, "
            f"offsets {v.first} .. {v.last} relative to the interior")


def _site():
    f = sys._getframe(1)
    while f is not None:
        name = os.path.abspath(f.f_code.co_filename)
        if name != _HERE and not name.startswith(_TORCH):
            return f"{os.path.basename(name)}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return "?"


def _span_bytes(t):
    return (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


def _pattern(word, n, device):
    """n bytes of the repeating little-endian word, from a multiple of 4 on"""
    return torch.tensor([(word >> s) & 0xFF for s in (0, 8, 16, 24)], dtype=torch.uint8, device=device).repeat(-(-n // 4))[:n]


def active():
    """the open guard_bands block, or None"""
    a = poison._active[0]
    return a if isinstance(a, guard_bands) else None


def house_at_the_door():
    """from here on the open block (if any) hands the library a banded twin of every tensor that lies in no band: see _handed_over"""
    g = active()
    if g is not None:
        g.door = True


def rehouse(t):
    """g.rehouse(t) of the open block; t itself when none is open (so one builder serves the plain and the banded runs)"""
    g = active()
    return t if g is None else g.rehouse(t)


class guard_bands:
    """`with guard_bands(word, devices=("cuda",), skew=0) as g:` -- while open, on a listed device type

      * torch.empty, torch.empty_like, Tensor.new_empty, torch.zeros, torch.zeros_like, Tensor.new_zeros return, and
      * a host -> device transfer through Tensor.to / Tensor.cuda (source not on the device, result on it, a new tensor) returns

    an interior view of a larger allocation: same shape, dtype, strides (a dense permuted empty_like result included), device and
    contents (zeros are zero, a transfer keeps its data), starting `skew` bytes past a 512-byte boundary, with BAND bytes or more of
    the repeating 32-bit `word` on either side.  The zeros family keeps 512-byte alignment whatever the skew (the stricter
    alignments include/ddk.h documents belong to caller-zeroed buffers).  Zero-element requests and `out=` calls pass through.

    g keeps every banded allocation alive (nothing is recycled before the check) with its call site, the first frame outside this
    file and torch.  g.count: banded tensors, g.transfers: those that came through the transfer hook, g.bytes: interior bytes,
    g.kinds: count per class (empty / zeros / transfer / rehouse / door).  g.check() returns the list of Violations; it runs again on exit,
    which raises GuardError(list) unless another exception is already on its way.  g.rehouse(t) does by hand what the transfer hook
    does: for inputs made on the device and for in-place targets.

    On entry and on exit ddk.ops._scratch and the wrappers' shape-keyed table caches are cleared, so that cached scratch and tables
    are allocated again inside bands and none of them outlives the registry.  g.unbanded lists what the wrappers handed to the
    library from outside any band (see _handed_over).  The originals are restored on exit, also after an exception.  Nesting is refused (RuntimeError), with
    itself and with poisoned_allocations, which patches the same functions: the block occupies poison's own slot while it is open.

    Nothing is banded while torch.cuda.is_current_stream_capturing() is true, for poison.py's reason: the fill would be recorded into
    the graph.  Buffers a graph needs banded are allocated before the capture starts."""

    _NAMES = (("empty", torch, "empty"), ("empty", torch, "empty_like"), ("empty", torch.Tensor, "new_empty"),
              ("zeros", torch, "zeros"), ("zeros", torch, "zeros_like"), ("zeros", torch.Tensor, "new_zeros"),
              ("transfer", torch.Tensor, "to"), ("transfer", torch.Tensor, "cuda"))

    def __init__(self, word, devices=("cuda",), skew=0):
        if skew % 16 or not 0 <= skew < ALIGN:
            raise ValueError("skew must be a multiple of 16 below 512")
        self.word, self.devices, self.skew = int(word) & 0xFFFFFFFF, tuple(devices), int(skew)
        self.count = self.transfers = self.bytes = 0
        self.kinds = collections.Counter()
        self.violations = []
        self.unbanded, self.door = {}, False       # (site in the wrappers, shape, dtype) -> times: see _handed_over
        self._records, self._saved, self._pat, self._housed = [], None, {}, set()

    # ------------------------------------------------------------------ housing
    def _wanted(self, t):
        if not torch.is_tensor(t) or t.device.type not in self.devices or t.numel() == 0 or t.is_sparse or t.layout != torch.strided:
            return False
        return not (t.device.type == "cuda" and torch.cuda.is_current_stream_capturing())

    def _fill(self, base, lo, hi):
        """the word into bytes [lo, hi) of the allocation, in phase with the allocation's start"""
        a, b = min(-(-lo // 4) * 4, hi), max(hi // 4 * 4, lo)
        if a < b:
            base[a:b].view(torch.int32).fill_(poison._i32(self.word))
        for i in list(range(lo, a)) + list(range(max(b, a), hi)):
            base[i] = (self.word >> (8 * (i % 4))) & 0xFF

    def _house(self, t, kind, keep):
        """t's twin inside bands; keep: copy t's contents (else zero them for kind "zeros", else leave them as allocated)"""
        if not self._wanted(t):
            return t
        site = _site()
        empty = self._saved[(torch, "empty")]
        with torch.no_grad():
            span, es = _span_bytes(t), t.element_size()
            skew = 0 if kind == "zeros" else self.skew
            total = -(-(BAND + ALIGN + skew + span + BAND) // 4) * 4
            base = empty(total, dtype=torch.uint8, device=t.device)
            off = BAND + (-(base.data_ptr() + BAND)) % ALIGN + skew
            assert base.data_ptr() % 16 == 0 and off % es == 0
            self._fill(base, 0, off)
            self._fill(base, off + span, total)
            inner = empty(0, dtype=t.dtype, device=t.device).set_(base.untyped_storage(), off // es, t.shape, t.stride())
            if keep:
                inner.copy_(t)
            elif kind == "zeros":
                base[off:off + span].zero_()
        if t.requires_grad:
            inner.requires_grad_(True)
        self._records.append(_Record(base, off, span, site, tuple(t.shape), t.dtype, kind))
        self._housed.add(base.untyped_storage().data_ptr())
        self.count += 1
        self.transfers += kind == "transfer"
        self.kinds[kind] += 1
        self.bytes += t.numel() * t.element_size()
        return inner

    def rehouse(self, t):
        """t's contents in a banded tensor of the same shape, dtype, strides and device (t itself if it is not on a listed device)"""
        if torch.is_tensor(t) and t.grad_fn is not None:
            raise ValueError("rehouse takes leaves: a tensor with a grad_fn would lose its graph")
        return self._house(t, "rehouse", True)

    def _transfer(self, src, out):
        if out is src or not torch.is_tensor(out) or src.device.type == out.device.type or out.grad_fn is not None:
            return out
        return self._house(out, "transfer", True)

    def _handed_over(self, t):
        """the audit at the library's door (ddk.lib.ptr, through which the wrappers turn every tensor into a pointer): a tensor on a
        listed device that lies in no banded allocation is recorded in g.unbanded with the wrapper's line.  That is how a case that
        hands the library a tensor torch made on the device (a sum, a clone, an operand a wrapper derives with torch ops) is found
        instead of listed.  With g.door set (house_at_the_door()) such a tensor is not recorded but copied into a banded twin, and
        the twin is what the library gets: right for what the library only reads; one it writes loses its result, which the
        comparison with the plain run then shows.  Nothing happens while a stream is capturing, where nothing is banded either."""
        if not torch.is_tensor(t) or t.untyped_storage().data_ptr() in self._housed or not self._wanted(t):
            return t
        if self.door:
            return self._house(t.detach(), "door", True)
        key = (_site(), tuple(t.shape), t.dtype)
        self.unbanded[key] = self.unbanded.get(key, 0) + 1
        return t

    # ------------------------------------------------------------------ the check
    def _expected(self, device, lo, hi):
        """the bytes [lo, hi) of an untouched allocation hold (a band is never longer than BAND + ALIGN + skew + 4)"""
        if device not in self._pat:
            self._pat[device] = _pattern(self.word, BAND + 2 * ALIGN + 8, device)
        return self._pat[device][lo % 4:lo % 4 + hi - lo]

    def check(self):
        """the list of Violations over every banded allocation so far (empty: every band still holds the word)"""
        if any(r.base.is_cuda for r in self._records):
            torch.cuda.synchronize()
        found = []
        with torch.no_grad():
            for r in self._records:
                total = r.base.numel()
                for side, lo, hi in (("before", 0, r.off), ("after", r.off + r.span, total)):
                    bad = (r.base[lo:hi] != self._expected(r.base.device, lo, hi)).nonzero().reshape(-1)
                    if bad.numel():
                        first, last = int(bad[0]), int(bad[-1])
                        rel = (first, last) if side == "after" else (first - r.off, last - r.off)
                        found.append(Violation(r.site, r.shape, r.dtype, side, int(bad.numel()), *rel))
        self.violations = found
        return found

    # ------------------------------------------------------------------ patching
    @staticmethod
    def _clear_scratch():
        """ops._scratch and the wrappers' caches of device tables that are keyed by shape (FFT twiddles, bicubic taps): filled
        before the block they would be handed to the library from outside any band.  (The packed-weight cache and the multi_add
        tables are keyed by the address of a tensor the case makes anew inside the block.)"""
        ops = sys.modules.get("ddk.ops")
        if ops is not None:
            for cache in (ops._scratch, ops._FFT_TWIDDLES, ops._bicubic_cache):
                cache.clear()

    def __enter__(self):
        if poison._active[0] is not None:
            raise RuntimeError("guard_bands does not nest, with itself or with poisoned_allocations")
        self._own = {name for _, owner, name in self._NAMES if owner is torch.Tensor and name in torch.Tensor.__dict__}
        self._saved = {(owner, name): getattr(owner, name) for _, owner, name in self._NAMES}

        def allocator(kind, fn):
            def banded(*a, **k):
                out = fn(*a, **k)
                return out if "out" in k else self._house(out, kind, False)
            return banded

        def mover(fn):
            def moved(t, *a, **k):
                return self._transfer(t, fn(t, *a, **k))
            return moved

        poison._active[0] = self
        self._clear_scratch()
        self._lib = sys.modules.get("ddk.lib")
        if self._lib is not None:
            ptr = self._lib_ptr = self._lib.ptr

            def audited(t):
                return ptr(self._handed_over(t))
            self._lib.ptr = audited
        for kind, owner, name in self._NAMES:
            fn = self._saved[(owner, name)]
            setattr(owner, name, mover(fn) if kind == "transfer" else allocator(kind, fn))
        return self

    def __exit__(self, etype, *exc):
        try:
            found = self.check() if etype is None else []
        finally:
            for _, owner, name in self._NAMES:
                if owner is torch.Tensor and name not in self._own:
                    delattr(owner, name)              # it was inherited: leave no attribute of our own behind
                else:
                    setattr(owner, name, self._saved[(owner, name)])
            if self._lib is not None:
                self._lib.ptr = self._lib_ptr
            self._clear_scratch()
            self._records, self._housed = [], set()
            poison._active[0] = None
        if found:
            raise GuardError(found)
        return False
