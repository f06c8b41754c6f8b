"""tests/guarded.py on host memory: the layout it promises and what intact() reports (the GPU tests rely on both)."""
import numpy as np
import pytest

from tests import guarded


@pytest.mark.parametrize("poison", guarded.POISONS)
@pytest.mark.parametrize("n,told", [(1000, None), (1000, 250), (300000, 4096), (7, 3)])
def test_layout_poison_and_report(poison, n, told):
    g = guarded.scratch(n, told, poison, device="cpu")
    assert g.view.numel() == (told or n) and g.view.data_ptr() % guarded.ALIGN == 0
    assert g.off >= guarded.FRONT and g.big.numel() - g.off - n >= max(n, 64 << 10)  # the far guard holds a full-size layout
    word = g.big[g.off:g.off + 4].numpy().view(np.uint32)[0]  # (the interior is poisoned too, whatever the caller is told)
    assert word == (0x7FC00000 if poison == guarded.NAN else 0x5A5A5A5A)
    assert g.intact()
    g.view[0] = 1  # inside what the caller was told: no canary
    assert g.intact()
    end = g.off + g.view.numel()
    g.big[end + 5] = 1
    g.big[end + 9] = 1
    g.big[g.off - 3] = 1
    rep = g.intact()
    assert not rep and (rep.behind, rep.behind_first, rep.front, rep.front_first) == (2, 5, 1, 3)
    assert "+5" in str(rep) and "3 byte(s) before" in str(rep)
    assert g.refill().intact()


def test_a_write_that_restores_the_poison_byte_is_not_a_change_but_any_other_value_is():
    g = guarded.scratch(64, poison=guarded.NAN, device="cpu")
    end = g.off + 64
    g.big[end] = 0  # (byte 0 of the little-endian word 0x7FC00000 is 0)
    assert g.intact()
    g.big[end + 2] = 0  # (byte 2 is 0xC0)
    assert g.intact().behind_first == 2


def test_output_is_a_guarded_tensor():
    keep = []
    t = guarded.output((3, 5), guarded.BYTES, keep, device="cpu")
    assert t.shape == (3, 5) and t.guard is keep[0] and float(t[0, 0]) == float(np.array([0x5A5A5A5A], np.uint32).view(np.float32)[0])
    t.fill_(1.0)
    assert guarded.check(keep) == []
    t.guard.big[t.guard.off + 60] = 7  # the first byte behind 15 floats
    assert guarded.check(keep) and "+0" in guarded.check(keep)[0]


@pytest.mark.parametrize("poison", guarded.POISONS)
@pytest.mark.parametrize("shift", [0, 4, 12])
def test_operand_is_the_array_between_poison(poison, shift):
    a = np.arange(3 * 5, dtype=np.float32).reshape(3, 5) - 7
    keep = []
    t = guarded.operand(a, poison, keep, name="x", shift_bytes=shift, device="cpu")
    g = t.guard
    assert g is keep[0] and g.name == "x" and t.shape == (3, 5) and t.data_ptr() % guarded.ALIGN == shift
    assert np.array_equal(t.numpy().view(np.uint32), a.view(np.uint32))  # the contents, bit for bit
    word = 0x7FC00000 if poison == guarded.NAN else 0x5A5A5A5A
    raw = g.big.numpy()
    end = g.off + a.nbytes
    assert raw[g.off - 4:g.off].view(np.uint32)[0] == word and raw[end:end + 4].view(np.uint32)[0] == word  # the poison word on both sides
    assert np.all(raw[:g.off].view(np.uint32) == word) and np.all(raw[end:end + (64 << 10)].view(np.uint32) == word)
    assert guarded.check(keep) == []
    t[1, 2] = 3.0  # an in-out tensor: a store inside it is no canary
    assert guarded.check(keep) == []
    g.big[end:end + 4].view(t.dtype)[0] = 1.0  # a store one element behind the tensor
    msgs = guarded.check(keep)
    assert len(msgs) == 1 and msgs[0].startswith("x: ") and "+" in msgs[0] and "BEHIND" in msgs[0]
    # (1.0f = 00 00 80 3F: against 00 00 C0 7F byte 2 is the first that differs, against 5A 5A 5A 5A byte 0)
    assert g.intact().behind_first == (2 if poison == guarded.NAN else 0) and g.intact().front == 0


@pytest.mark.parametrize("dtype,values", [(np.int32, [-2 ** 31, -1, 0, 5, 2 ** 31 - 1]), (np.uint8, [0, 1, 0x5A, 200, 255, 7, 9])])
def test_operand_keeps_int32_and_uint8(dtype, values):
    import torch

    a = np.array(values, dtype)
    for shift in (0, 4, 12):
        keep = []
        t = guarded.operand(a, guarded.BYTES, keep, shift_bytes=shift, device="cpu")
        assert t.dtype == (torch.int32 if dtype == np.int32 else torch.uint8) and np.array_equal(t.numpy(), a)
        raw, g = t.guard.big.numpy(), t.guard
        assert np.all(raw[:g.off] == 0x5A) and np.all(raw[g.off + a.nbytes:] == 0x5A) and guarded.check(keep) == []
        g.big[g.off + a.nbytes] = 0  # one element (uint8) / the first byte of one element (int32) behind the tensor
        assert guarded.check(keep) and "+0 " in guarded.check(keep)[0]


def test_operand_refuses_other_dtypes():
    with pytest.raises(AssertionError):
        guarded.operand(np.zeros(3, np.float64), device="cpu")
