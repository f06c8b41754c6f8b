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
