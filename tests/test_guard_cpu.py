"""tests/guard.py on the CPU device: the harness the extent tests stand on hands back what the unpatched call would, puts it where it
says, fills its bands, sees a write into them (and only that), counts and restores as it says."""
import pytest
import torch

import guard
import poison
from guard import ALIGN, BAND, GuardError, guard_bands
from poison import NAN, ONE, WORDS, ZERO, poisoned_allocations

CPU = ("cpu",)
PATCHED = ((torch, "empty"), (torch, "empty_like"), (torch.Tensor, "new_empty"), (torch, "zeros"), (torch, "zeros_like"),
           (torch.Tensor, "new_zeros"), (torch.Tensor, "to"), (torch.Tensor, "cuda"))
MARK = 0x12345678          # every byte differs from the same byte of each of poison.WORDS


def _current():
    return [getattr(o, n) for o, n in PATCHED]


def _word_bytes(word, n):
    return torch.tensor([(word >> s) & 0xFF for s in (0, 8, 16, 24)], dtype=torch.uint8).repeat((n + 3) // 4)[:n]


def _bands(g, t):
    """(the bytes before t, the bytes after t) of the banded allocation t lives in"""
    rec = next(r for r in g._records if r.base.untyped_storage().data_ptr() == t.untyped_storage().data_ptr())
    assert rec.off == t.storage_offset() * t.element_size()
    return rec.base[:rec.off], rec.base[rec.off + rec.span:]


PERMUTED = torch.zeros(2, 3, 5, 7).permute(0, 2, 3, 1)         # dense, not contiguous: empty_like keeps the strides
FORMS = {      # every call form the product uses -> (call, banded?)
    "positional sizes": (lambda: torch.empty(3, 5, 7), True),
    "a tuple": (lambda: torch.empty((4, 6)), True),
    "dtype and device keywords": (lambda: torch.empty((2, 9), dtype=torch.int64, device="cpu"), True),
    "empty_like": (lambda: torch.empty_like(torch.ones(5, 3, dtype=torch.float64)), True),
    "empty_like of a permuted tensor": (lambda: torch.empty_like(PERMUTED), True),
    "new_empty": (lambda: torch.ones(2, dtype=torch.float64).new_empty((3, 4), dtype=torch.int32), True),
    "new_zeros": (lambda: torch.ones(2).new_zeros((7, 3)), True),
    "zeros": (lambda: torch.zeros(33, dtype=torch.uint8), True),
    "zeros with a tuple": (lambda: torch.zeros((3, 11), device="cpu"), True),
    "zeros_like": (lambda: torch.zeros_like(PERMUTED), True),
    "zero elements": (lambda: torch.empty(0, 4), False),
    "zero elements, zeros": (lambda: torch.zeros((3, 0)), False),
}


# ---------------------------------------------------------------- interior identity, alignment, contents
@pytest.mark.parametrize("skew", [0, 16])
@pytest.mark.parametrize("form", list(FORMS))
def test_the_interior_is_what_the_unpatched_call_returns(form, skew):
    call, banded = FORMS[form]
    plain = call()
    with guard_bands(ONE, CPU, skew=skew) as g:
        t = call()
        assert g.count == int(banded)
        if banded:
            zeros = "zeros" in form
            assert t.data_ptr() % ALIGN == (0 if zeros else skew), "the zeros family keeps 512-byte alignment"
            before, after = _bands(g, t)
            assert before.numel() >= BAND and after.numel() >= BAND
            assert t.untyped_storage().nbytes() >= 2 * BAND + t.numel() * t.element_size()
    assert (t.shape, t.stride(), t.dtype, t.device, t.is_contiguous()) == \
        (plain.shape, plain.stride(), plain.dtype, plain.device, plain.is_contiguous())
    if "zeros" in form and banded:
        assert int(t.count_nonzero()) == 0


def test_empty_like_of_a_permuted_tensor_keeps_its_strides():
    with guard_bands(NAN, CPU) as g:
        t = torch.empty_like(PERMUTED)
    assert t.stride() == PERMUTED.stride() and not t.is_contiguous() and g.bytes == PERMUTED.numel() * 4


@pytest.mark.parametrize("skew", [0, 16])
def test_rehouse_keeps_contents_and_layout(skew):
    src = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7).permute(0, 2, 3, 1)
    odd = torch.arange(13, dtype=torch.uint8)
    with guard_bands(ZERO, CPU, skew=skew) as g:
        t, u = g.rehouse(src), guard.rehouse(odd)
        assert guard.active() is g
        assert g.count == 2 and g.transfers == 0 and g.kinds == {"rehouse": 2}
        assert t.data_ptr() % ALIGN == skew and u.data_ptr() % ALIGN == skew
        for v in (t, u):
            for band in _bands(g, v):
                assert int(band.count_nonzero()) == 0
    assert torch.equal(t, src) and t.stride() == src.stride() and t.data_ptr() != src.data_ptr()
    assert torch.equal(u, odd)
    assert guard.active() is None and guard.rehouse(odd) is odd, "outside a block rehouse hands its argument back"


def test_a_transfer_within_the_device_is_not_a_transfer():
    src = torch.ones(5)
    with guard_bands(ONE, CPU) as g:
        assert src.to("cpu") is src
        d = src.to(torch.float64)          # a new tensor, but its source was on the device already
    assert g.count == 0 and g.transfers == 0 and d.dtype == torch.float64


def test_requires_grad_and_out_pass_through():
    buf = torch.ones(6)
    with guard_bands(ONE, CPU) as g:
        leaf = torch.zeros(4, requires_grad=True)
        same = torch.zeros(6, out=buf)
    assert leaf.requires_grad and leaf.is_leaf and g.count == 1
    assert same.data_ptr() == buf.data_ptr() and int(buf.count_nonzero()) == 0


# ---------------------------------------------------------------- the bands
@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (5, 3)), (torch.uint8, (13,)), (torch.uint8, (3, 13, 17, 3)), (torch.int64, (7,)),
                                         (torch.float64, (1,))])
def test_bands_hold_the_word(word, dtype, shape):
    with guard_bands(word, CPU, skew=16) as g:
        made = [torch.empty(shape, dtype=dtype), torch.zeros(shape, dtype=dtype), g.rehouse(torch.ones(shape, dtype=dtype))]
        for t in made:
            before, after = _bands(g, t)
            assert torch.equal(before, _word_bytes(word, before.numel()))
            lead = (-(before.numel() + t.numel() * t.element_size())) % 4           # the word stays in phase with the allocation
            assert torch.equal(after[lead:], _word_bytes(word, after.numel() - lead))
            assert torch.equal(after[:lead], _word_bytes(word, 4)[4 - lead:] if lead else after[:0])
        assert g.check() == []
    assert int(made[1].count_nonzero()) == 0 and bool((made[2] == 1).all())


# ---------------------------------------------------------------- seeded overruns: each write lies inside its own allocation
def _poke(t, offset_elems, n, value):
    """write n elements of t's dtype from `offset_elems` past t's first element, through as_strided (a torch op, inside t's storage)"""
    t.as_strided((n,), (1,), t.storage_offset() + offset_elems).fill_(value)


@pytest.mark.parametrize("word", WORDS)
def test_seeded_overruns_are_reported(word):
    with pytest.raises(GuardError) as caught:
        with guard_bands(word, CPU) as g:
            past = torch.empty((3, 6, 10, 3), dtype=torch.int32)          # one element past the end
            front = torch.zeros(100, dtype=torch.int32)                    # one element before the start
            far = torch.empty(777, dtype=torch.uint8)                      # 1000 bytes from 100 KiB past the end
            clean = torch.empty(64)
            assert g.check() == []
            _poke(past, past.numel(), 1, MARK)
            _poke(front, -1, 1, MARK)
            _poke(far, far.numel() + 100 * 1024, 1000, 0x5A)
            clean.fill_(3.0)
            past.fill_(7)
            found = g.check()
            assert g.count == 4
    assert caught.value.violations == found and "damaged bytes" in str(caught.value)
    by_shape = {v.shape: v for v in found}
    assert len(found) == 3 and (64,) not in by_shape, "an untouched tensor is not reported"
    v = by_shape[(3, 6, 10, 3)]
    assert (v.side, v.nbytes, v.first, v.last, v.dtype) == ("after", 4, 0, 3, torch.int32)
    v = by_shape[(100,)]
    assert (v.side, v.nbytes, v.first, v.last) == ("before", 4, -4, -1)
    v = by_shape[(777,)]
    assert (v.side, v.nbytes, v.first, v.last, v.dtype) == ("after", 1000, 100 * 1024, 100 * 1024 + 999, torch.uint8)
    for v in found:
        assert v.site.startswith("test_guard_cpu.py:") and "test_seeded_overruns_are_reported" in v.site, v.site


def test_a_write_of_the_word_itself_is_invisible_under_that_word_only():
    """why there are three words: a stray 0.0 does not show in a band of zeros, and shows under the other two"""
    seen = {}
    for word in WORDS:
        with guard_bands(word, CPU) as g:
            t = torch.empty(10)
            _poke(t, 10, 1, 0.0)
            seen[word] = len(g.check())
            t.as_strided((1,), (1,), t.storage_offset() + 10).view(torch.int32).fill_(poison._i32(word))          # put the band back: the exit checks again
    assert seen[ZERO] == 0 and seen[ONE] == 1 and seen[NAN] == 1


def test_the_call_site_skips_torch_frames():
    lin = torch.nn.Linear(3, 2)
    with guard_bands(ONE, CPU) as g:
        torch.nn.functional.one_hot(torch.tensor([1, 2]), 4)             # whatever torch allocates for itself is attributed to this line
        lin.weight.new_empty((2, 2))
        sites = [r.site for r in g._records]
    assert sites and all(s.startswith("test_guard_cpu.py:") for s in sites), sites


# ---------------------------------------------------------------- housekeeping
def test_patches_are_restored_after_exit_and_after_a_raise():
    saved, own = _current(), {n for o, n in PATCHED if o is torch.Tensor and n in torch.Tensor.__dict__}
    with guard_bands(ONE, CPU):
        now = _current()
        assert all(a is not b for a, b in zip(now, saved))
    assert _current() == saved
    with pytest.raises(ZeroDivisionError):
        with guard_bands(NAN, CPU) as g:
            t = torch.empty(3)
            _poke(t, 3, 1, 1.5)              # the exception in flight wins over the violation
            1 / 0
    assert _current() == saved and poison._active[0] is None
    assert {n for o, n in PATCHED if o is torch.Tensor and n in torch.Tensor.__dict__} == own, "no attribute of the harness is left on Tensor"
    with guard_bands(ZERO, CPU):             # and the helper is usable again
        pass


def test_nesting_is_refused_both_ways():
    saved = _current()
    with guard_bands(ONE, CPU) as outer:
        with pytest.raises(RuntimeError, match="does not nest"):
            with guard_bands(ZERO, CPU):
                pass
        with pytest.raises(RuntimeError, match="does not nest"):
            with poisoned_allocations(ZERO, CPU):
                pass
        torch.empty(2)
        assert outer.count == 1 and guard.active() is outer, "the outer block is still in force"
    with poisoned_allocations(ONE, CPU) as p:
        with pytest.raises(RuntimeError, match="does not nest"):
            with guard_bands(ZERO, CPU):
                pass
        assert (torch.empty(2) == 1).all() and p.count == 1 and guard.active() is None
    assert _current() == saved


def test_count_and_bytes_add_up():
    with guard_bands(ONE, CPU) as g:
        torch.empty(5)
        torch.empty((2, 3), dtype=torch.int64)
        torch.empty_like(torch.ones(7, dtype=torch.uint8))
        torch.ones(1).new_empty((4,))
        torch.zeros(9)
        torch.zeros_like(torch.ones(3, dtype=torch.float64))
        torch.ones(1).new_zeros((2, 2))
        g.rehouse(torch.ones(11))
        torch.empty(0)                     # nothing to house: not counted
        torch.ones(9)                      # not a patched entry
        if torch.cuda.is_available():
            torch.empty(3, device="cuda")  # not a listed device
    assert g.count == 8 and g.transfers == 0 and g.bytes == 5 * 4 + 6 * 8 + 7 + 4 * 4 + 9 * 4 + 3 * 8 + 4 * 4 + 11 * 4
    assert g.kinds == {"empty": 4, "zeros": 3, "rehouse": 1}
    before = (g.count, g.bytes)
    torch.empty(5)
    assert (g.count, g.bytes) == before, "nothing is counted after the block"


def test_cached_scratch_is_dropped_on_entry_and_exit():
    import sys
    ops = sys.modules.get("ddk.ops")
    if ops is None:
        from ddk import ops
    ops._scratch[("cpu", "test", 0)] = torch.ones(4)
    with guard_bands(ONE, CPU):
        assert ops._scratch == {}
        ops._scratch[("cpu", "test", 0)] = torch.empty(4)          # what a wrapper would cache: a banded view
    assert ops._scratch == {}


def test_skew_is_checked():
    for bad in (8, 512, -16):
        with pytest.raises(ValueError):
            guard_bands(ONE, CPU, skew=bad)


# ---------------------------------------------------------------- the audit at the library's door
def test_the_door_records_what_lies_in_no_band_and_houses_it_on_request():
    from ddk import lib
    saved = lib.ptr
    outside, other = torch.arange(6.0), torch.ones(2, 3, dtype=torch.int64)
    with guard_bands(ONE, CPU) as g:
        assert lib.ptr is not saved
        inside = torch.empty(4)
        assert g._handed_over(inside) is inside and g._handed_over(inside[1:]).data_ptr() == inside[1:].data_ptr() and g._handed_over(None) is None
        assert g.unbanded == {}
        assert g._handed_over(outside) is outside and g._handed_over(outside) is outside and g._handed_over(other) is other
        assert sorted((shape, n) for (site, shape, dtype), n in g.unbanded.items()) == [((2, 3), 1), ((6,), 2)]
        assert all(site.startswith("test_guard_cpu.py:") for site, _, _ in g.unbanded)
        with pytest.raises(lib.DDKError):
            lib.ptr(outside)                          # recorded once more, then the library refuses a host tensor as ever
        guard.house_at_the_door()
        twin = g._handed_over(outside)
        assert twin is not outside and torch.equal(twin, outside) and g.kinds["door"] == 1 and len(g.unbanded) == 3
        for band in _bands(g, twin):
            assert torch.equal(band, _word_bytes(ONE, band.numel()))
        assert g._handed_over(twin) is twin
    assert lib.ptr is saved
    guard.house_at_the_door()                         # no block open: nothing to do
