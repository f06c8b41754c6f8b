"""Device buffers between two poisoned guard zones: what a HIP call does to memory it was not given, and whether it reads scratch that
nobody wrote.

The C ABI takes its scratch from the caller (`ws`, prepared-filter images, pool masks; sized by the *_bytes queries), and a caller carves
those buffers out of one arena: a store one float behind the promised size lands in its neighbour.  A plain
torch.empty() hides both kinds of error -- the caching allocator rounds sizes up, and recycled memory holds finite floats.  Here every
buffer is the interior of ONE larger allocation

    | front guard, >= 64 KiB | interior: n_bytes, 256-byte aligned | far guard, >= max(n_bytes, 64 KiB) |

filled with a poison as a whole; the caller is handed the first `told_bytes` of the interior and everything else is canary.  The far guard
is as large as the interior, so code that ignores a short `told_bytes` and lays out its full-size scratch still stays inside the
allocation: the mistake shows as a changed canary, never as a fault.

Two poisons, because each hides from one kind of reader: NAN (32-bit words 0x7FC00000) spreads through every sum but vanishes in a masked
select (`x > 0 ? x : 0`), BYTES (0x5A everywhere: 1.5e16 as a float, a huge index as an int) survives any select but could cancel.
operand() places an INPUT the same way (tests/test_gpu_operand_contract.py): its neighbours in memory are the poison, not whatever the
caching allocator last held there.
A plain module: the tests and the sweep scripts import it (`from tests import guarded`)."""
import numpy as np

FRONT = 64 << 10   # bytes in front of the interior
ALIGN = 256        # the interior starts on this boundary (+ shift_bytes)
NAN = "nan"        # 32-bit words 0x7FC00000: a quiet NaN
BYTES = "bytes"    # bytes 0x5A: the float 1.5e16
POISONS = (NAN, BYTES)
_PATTERN = {NAN: (0x00, 0x00, 0xC0, 0x7F), BYTES: (0x5A, 0x5A, 0x5A, 0x5A)}  # little endian


class Report:
    """what intact() found: counts and first offsets of changed canary bytes.  `front_first` counts backwards from the interior
    (1 = the byte just in front of it), `behind_first` forwards from the end of what the caller was told (0 = the first byte behind)."""

    def __init__(self, name, front, front_first, behind, behind_first):
        self.name, self.front, self.front_first, self.behind, self.behind_first = name, front, front_first, behind, behind_first

    def __bool__(self):
        return self.front == 0 and self.behind == 0

    def __str__(self):
        if self:
            return f"{self.name}: canary intact"
        parts = []
        if self.front:
            parts.append(f"{self.front} byte(s) changed IN FRONT, the nearest {self.front_first} byte(s) before the buffer")
        if self.behind:
            parts.append(f"{self.behind} byte(s) changed BEHIND, the first at offset +{self.behind_first} from the end of the buffer")
        return f"{self.name}: " + "; ".join(parts)


class Scratch:
    """one guarded allocation; `.view` is the uint8 tensor to hand to the call (`told_bytes or n_bytes` long)"""

    def __init__(self, n_bytes, told_bytes=None, poison=NAN, name="scratch", shift_bytes=0, device="cuda"):
        import torch

        n_bytes = int(n_bytes)
        self.n_bytes, self.told = n_bytes, n_bytes if told_bytes is None else int(told_bytes)
        assert 0 <= self.told <= n_bytes and poison in _PATTERN and shift_bytes % 4 == 0
        self.poison, self.name = poison, name
        far = max(n_bytes, 64 << 10)
        total = (FRONT + ALIGN + shift_bytes + n_bytes + far + 3) & ~3
        self.big = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.big.data_ptr()
        assert base % 4 == 0
        self.off = FRONT + (-(base + FRONT)) % ALIGN + shift_bytes
        self._pat = torch.tensor(_PATTERN[poison], dtype=torch.uint8, device=device)
        self._word = int(np.array(_PATTERN[poison], np.uint8).view(np.int32)[0])
        self.view = self.big[self.off:self.off + self.told]
        self.refill()

    def refill(self):
        """the poison everywhere, the interior included"""
        import torch

        self.big.view(torch.int32).fill_(self._word)
        return self

    def intact(self):
        """-> Report (truthy when no canary byte changed); synchronises"""
        import torch

        if self.big.is_cuda:
            torch.cuda.synchronize()
        changed = (self.big.view(-1, 4) != self._pat).view(-1)
        front, behind = changed[:self.off], changed[self.off + self.told:]
        nf, nb = int(front.sum().item()), int(behind.sum().item())
        ff = self.off - int(torch.nonzero(front)[-1].item()) if nf else None
        bf = int(torch.nonzero(behind)[0].item()) if nb else None
        return Report(self.name, nf, ff, nb, bf)


def scratch(n_bytes, told_bytes=None, poison=NAN, name="scratch", shift_bytes=0, device="cuda"):
    """GUARD | n_bytes | GUARD in one device allocation, all of it poisoned -> Scratch (hand `.view` to the call, ask `.intact()` after it)"""
    return Scratch(n_bytes, told_bytes, poison, name, shift_bytes, device)


def output(shape, poison=NAN, keep=None, name="output", dtype=None, shift_bytes=0, device="cuda"):
    """the same for an output tensor (fp32 unless dtype is given): -> a tensor of `shape` inside a guarded allocation; `.guard` is its
    Scratch, also appended to the list `keep` so that a test can ask every output of a call with check(keep)"""
    import torch

    dtype = torch.float32 if dtype is None else dtype
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    g = Scratch(n, None, poison, name, shift_bytes, device)
    t = g.view.view(dtype).view(*shape)
    t.guard = g
    if keep is not None:
        keep.append(g)
    return t


def operand(array, poison=NAN, keep=None, name="operand", shift_bytes=0, device="cuda"):
    """a read-only (or in-out) operand between poison: output(...) plus a copy-in -> a tensor of the array's shape and dtype (fp32, int32
    or uint8) whose every neighbour in memory is the poison; `.guard` is its Scratch, also appended to `keep`.  A kernel that lets a value
    from beyond the tensor into a result carries the poison there; a store through the input pointer changes a canary (check(keep))."""
    import torch

    a = np.ascontiguousarray(array)
    assert a.dtype in (np.float32, np.int32, np.uint8), a.dtype
    src = torch.from_numpy(a)
    t = output(a.shape, poison, keep, name, src.dtype, shift_bytes, device)
    t.copy_(src)
    return t


def check(guards):
    """-> [str(report) of every guard whose canary changed] (empty: all intact)"""
    return [str(r) for r in (g.intact() for g in guards) if not r]
