"""Poisoned allocations: every buffer the wrappers hand to the library comes from torch.empty / torch.empty_like /
Tensor.new_empty, so its contract is "any contents".  `poisoned_allocations(word)` fills each such tensor with a repeating 32-bit
word before it is handed back; a result that changes with the word was read before it was written.

Three words, because no single one shows every dependence (fminf / fmaxf swallow a NaN, a zero hides an assumed-zero counter):

    NAN  0xFFFFFFFF  float32 NaN   int -1               unsigned 4294967295
    ZERO 0x00000000  float32 0.0   int 0                unsigned 0
    ONE  0x3F800000  float32 1.0   int 1065353216       unsigned 1065353216

The assertion to make is bit-equality of the results across the words, never "no NaN appeared"."""
import torch

NAN, ZERO, ONE = 0xFFFFFFFF, 0x00000000, 0x3F800000
WORDS = (NAN, ZERO, ONE)

_active = [None]


def _i32(word):
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= (1 << 31) else word


def fill_word(t, word):
    """Fill every byte of t's memory with the repeating 32-bit `word`: an int32 view when the byte size is a multiple of 4, else
    the word's low byte in every byte.  The fill goes through a flat byte view of the storage range the tensor spans, so a
    permuted (dense but not contiguous) empty_like result is covered whole, and so would be the gaps of a strided one."""
    if t.numel() == 0:
        return t
    es = t.element_size()
    span = (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * es
    raw = torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), t.storage_offset() * es, (span,))
    if span % 4 == 0 and raw.data_ptr() % 4 == 0:
        raw.view(torch.int32).fill_(_i32(word))
    else:
        raw.fill_(word & 0xFF)
    return t


class poisoned_allocations:
    """`with poisoned_allocations(word, devices=("cuda",)) as p:` -- while open, torch.empty, torch.empty_like and
    torch.Tensor.new_empty fill what they return on a listed device type with the repeating 32-bit `word`.  p.count / p.bytes:
    tensors and bytes poisoned.  The originals are restored on exit, also after an exception.  Nested use is refused
    (RuntimeError): the inner block would restore the outer block's patches.

    Nothing is poisoned while torch.cuda.is_current_stream_capturing() is true: the fill would be recorded into the graph and
    run at every replay, after the launches that wrote the buffer at capture time were recorded before it -- and it would change
    the graph under test.  Buffers a graph needs poisoned are allocated (and so poisoned) before the capture starts."""

    def __init__(self, word, devices=("cuda",)):
        self.word, self.devices = int(word) & 0xFFFFFFFF, tuple(devices)
        self.count = self.bytes = 0
        self._saved = None

    def _poison(self, t):
        if not torch.is_tensor(t) or t.device.type not in self.devices or t.numel() == 0:
            return t
        if t.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return t
        with torch.no_grad():
            fill_word(t, self.word)
        self.count += 1
        self.bytes += t.numel() * t.element_size()
        return t

    def __enter__(self):
        if _active[0] is not None:
            raise RuntimeError("poisoned_allocations does not nest")
        saved = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
        empty, empty_like, new_empty = saved

        def p_empty(*a, **k):
            return self._poison(empty(*a, **k))

        def p_empty_like(*a, **k):
            return self._poison(empty_like(*a, **k))

        def p_new_empty(t, *a, **k):
            return self._poison(new_empty(t, *a, **k))

        self._saved = saved
        _active[0] = self
        torch.empty, torch.empty_like, torch.Tensor.new_empty = p_empty, p_empty_like, p_new_empty
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.Tensor.new_empty = self._saved
        _active[0] = None
        return False


def repoison(word):
    """Fill every cached scratch tensor of ddk.ops._scratch with `word`: cached scratch is "any contents" as much as fresh scratch.
    Returns how many tensors it filled."""
    from ddk import ops
    n = 0
    for buf in ops._scratch.values():
        if torch.is_tensor(buf):
            fill_word(buf, word)
            n += 1
    return n
