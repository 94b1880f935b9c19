"""tests/poison.py on the CPU device: the helper the buffer-contents tests stand on patches, fills, counts and restores as it says."""
import pytest
import torch

from poison import NAN, ONE, WORDS, ZERO, poisoned_allocations

CPU = ("cpu",)


def _bytes(t):
    """every byte of a dense tensor's memory, in address order"""
    order = sorted(range(t.dim()), key=lambda d: -t.stride(d))
    return t.permute(*order).contiguous().view(-1).view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


def _word_bytes(word, n):
    pat = torch.tensor([(word >> s) & 0xFF for s in (0, 8, 16, 24)], dtype=torch.uint8)      # little endian
    return pat.repeat((n + 3) // 4)[:n]


def test_entry_points_are_patched_and_restored():
    saved = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poisoned_allocations(ONE, CPU):
        assert torch.empty is not saved[0] and torch.empty_like is not saved[1] and torch.Tensor.new_empty is not saved[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == saved


def test_restored_after_a_raise():
    saved = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(ZeroDivisionError):
        with poisoned_allocations(NAN, CPU):
            torch.empty(3)
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == saved
    with poisoned_allocations(ZERO, CPU):         # and the helper is usable again
        pass


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize("shape", [(8,), (5,), (3, 7), (2, 3, 4), (1,), (6,), (7,)])
def test_fresh_tensors_hold_the_word(word, dtype, shape):
    with poisoned_allocations(word, CPU):
        made = [torch.empty(shape, dtype=dtype), torch.empty(*shape, dtype=dtype), torch.empty_like(torch.zeros(shape, dtype=dtype)),
                torch.zeros(2, dtype=torch.float64).new_empty(shape, dtype=dtype)]
    for t in made:
        assert t.shape == shape and t.dtype == dtype
        raw = _bytes(t)
        n = raw.numel()
        if n % 4 == 0:
            assert torch.equal(raw, _word_bytes(word, n))
            assert torch.equal(raw.view(torch.int32), torch.full((n // 4,), word - (1 << 32) if word >> 31 else word, dtype=torch.int32))
        else:                                      # only uint8 at these shapes: the word's low byte everywhere
            assert dtype == torch.uint8 and torch.equal(raw, torch.full((n,), word & 0xFF, dtype=torch.uint8))


def test_the_words_mean_what_the_table_says():
    with poisoned_allocations(NAN, CPU):
        assert torch.empty(4).isnan().all() and (torch.empty(4, dtype=torch.int32) == -1).all()
    with poisoned_allocations(ZERO, CPU):
        assert (torch.empty(4) == 0).all() and (torch.empty(4, dtype=torch.int64) == 0).all()
    with poisoned_allocations(ONE, CPU):
        assert (torch.empty(4) == 1).all() and (torch.empty(4, dtype=torch.int32) == 0x3F800000).all()


@pytest.mark.parametrize("word", WORDS)
def test_empty_like_of_a_permuted_tensor_is_covered(word):
    src = torch.zeros(2, 3, 5, 7).permute(0, 2, 3, 1)          # dense, not contiguous: empty_like keeps the strides
    with poisoned_allocations(word, CPU) as p:
        t = torch.empty_like(src)
    assert t.stride() == src.stride() and not t.is_contiguous()
    assert torch.equal(_bytes(t), _word_bytes(word, t.numel() * 4))
    assert p.count == 1 and p.bytes == t.numel() * 4
    sliced = torch.zeros(4, 6)[:, ::2]                         # not dense: empty_like hands back a contiguous tensor
    with poisoned_allocations(word, CPU):
        u = torch.empty_like(sliced)
    assert torch.equal(_bytes(u), _word_bytes(word, u.numel() * 4))


def test_count_and_bytes():
    with poisoned_allocations(ONE, CPU) as p:
        torch.empty(5)
        torch.empty((2, 3), dtype=torch.int64)
        torch.empty_like(torch.zeros(7, dtype=torch.uint8))
        torch.zeros(1).new_empty((4,))
        torch.empty(0)                     # nothing to fill: not counted
        torch.zeros(9)                     # not a patched entry
        if torch.cuda.is_available():
            torch.empty(3, device="cuda")  # not a listed device
    assert p.count == 4 and p.bytes == 5 * 4 + 6 * 8 + 7 + 4 * 4
    before = (p.count, p.bytes)
    torch.empty(5)
    assert (p.count, p.bytes) == before, "nothing is counted after the block"


def test_nested_use_is_refused():
    saved = torch.empty
    with poisoned_allocations(ONE, CPU) as outer:
        with pytest.raises(RuntimeError, match="does not nest"):
            with poisoned_allocations(ZERO, CPU):
                pass
        assert (torch.empty(2) == 1).all() and outer.count == 1, "the outer block is still in force"
    assert torch.empty is saved


def test_a_read_of_unwritten_memory_shows_as_different_bits():
    """the harness can see a dependence: a function that returns what torch.empty held differs between two words"""
    def leaky():
        return torch.empty(5).clone()

    def sound():
        out = torch.empty(5)
        out.copy_(torch.arange(5.0))
        return out.clone()

    got, ok = [], []
    for word in (ZERO, ONE):
        with poisoned_allocations(word, CPU):
            got.append(leaky())
            ok.append(sound())
    assert not torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
    assert torch.equal(ok[0].view(torch.int32), ok[1].view(torch.int32))
