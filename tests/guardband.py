"""An arena with guard zones: the memory AROUND a kernel's outputs, owned and inspected by the test.

One torch.uint8 tensor is carved into regions (`Arena.place`).  Every region has a guard zone before and after it; guards and
not-yet-written outputs hold a position-dependent byte pattern, the flanks of an INPUT hold a poison byte that is extreme in every
type the library reads (POISONS: 0x7F = int8 127, fp16 NaN, bf16 / fp32 ~3.4e38; 0xFF = int8 -1, NaN in fp16 / bf16 / fp32 / e4m3).
`Arena.check` compares, on the arena's device, every guard with the regenerated pattern and every input with what was put there,
and reports per violated region its name, the side and the first / last changed offset relative to the region's first byte
(negative: before it; >= nbytes: behind it).

A wrong store lands in memory the test owns and is SEEN; nothing here puts a buffer at the end of an allocation or tries to make
the hardware fault.  Works on CPU tensors as well (tests/test_guardband_cpu.py)."""
import torch

KINDS = ("output", "input", "workspace")
POISONS = (0x7F, 0xFF)
MIN_GUARD = 1 << 20     # bytes: a guard is at least this ...
GUARD_ROWS = 128        # ... and at least this many rows of the region's pitch (nothing a stray 128-row tile covers escapes it)
_BASE_ALIGN = 4096      # arena offset 0 sits on such an address, so `align` up to this is honoured exactly
_CHUNK = 1 << 22


def pattern(start, n, device="cpu"):
    """The guard pattern of arena offsets start .. start + n - 1 (uint8).  Depends on the position only; walks through all 256 byte values
    within any 256 consecutive offsets and shifts from one 256-byte line to the next, so neither a constant fill (0, 0x5A, 0xFF) nor a
    copy of a neighbouring line reproduces it."""
    out = torch.empty((n,), dtype=torch.uint8, device=device)
    for a in range(0, n, _CHUNK):
        b = min(n, a + _CHUNK)
        i = torch.arange(start + a, start + b, dtype=torch.int64, device=device)
        out[a:b] = ((i * 131 + (i >> 8) * 29 + (i >> 16) * 7 + 0x3D) & 0xFF).to(torch.uint8)
    return out


def guard_bytes(pitch=0):
    return max(MIN_GUARD, GUARD_ROWS * int(pitch))


class Region:
    """[off, off + nbytes) of the arena; guards [g0, off) and [off + nbytes, g1)."""

    def __init__(self, arena, name, kind, off, nbytes, g0, g1):
        self.arena, self.name, self.kind, self.off, self.nbytes, self.g0, self.g1 = arena, name, kind, off, nbytes, g0, g1

    @property
    def ptr(self):
        return self.arena.base_ptr + self.off

    def bytes(self):
        return self.arena.buf[self.off:self.off + self.nbytes]

    def view(self, dtype, shape):
        """the region as a tensor (a view into the arena: writes through it are writes into the arena)"""
        n = 1
        for s in shape:
            n *= int(s)
        nb = n * torch.empty((), dtype=dtype).element_size()
        assert nb <= self.nbytes, (self.name, nb, self.nbytes)
        return self.arena.buf[self.off:self.off + nb].view(dtype).view(*shape)


class Report:
    def __init__(self, guards, inputs):
        self.guards = guards    # [{"region", "kind", "side": "before" | "after", "first", "last", "count"}]
        self.inputs = inputs    # [{"region", "first", "last", "count"}]

    @property
    def ok(self):
        return not self.guards and not self.inputs

    @property
    def inputs_intact(self):
        return not self.inputs

    def __str__(self):
        if self.ok:
            return "guards intact, inputs unchanged"
        lines = [f"guard {g['side']} {g['kind']} region '{g['region']}' changed: offsets {g['first']} .. {g['last']} relative to the region ({g['count']} bytes)"
                 for g in self.guards]
        lines += [f"input region '{i['region']}' changed: offsets {i['first']} .. {i['last']} ({i['count']} bytes)" for i in self.inputs]
        return "; ".join(lines)


class Arena:
    def __init__(self, nbytes, device="cpu", poison=POISONS[0]):
        self.device = torch.device(device)
        self._raw = torch.empty((int(nbytes) + _BASE_ALIGN,), dtype=torch.uint8, device=self.device)
        shift = (-self._raw.data_ptr()) % _BASE_ALIGN
        self.buf = self._raw[shift:shift + int(nbytes)]
        self.want = torch.empty_like(self.buf)      # what every byte outside an output / workspace region must still hold at check()
        self.base_ptr = self.buf.data_ptr()
        self.capacity = int(nbytes)
        self._pat = None
        self.reset(poison)

    def reset(self, poison=None):
        """forget every region (the bytes are rewritten as regions are placed)"""
        if poison is not None:
            assert 0 <= poison <= 0xFF
            self.poison = poison
        self.regions = []
        self.used = 0

    def _pattern(self, a, b):
        if self._pat is None or self._pat.numel() < b:      # the pattern is a function of the offset: keep the longest prefix ever needed
            self._pat = pattern(0, min(self.capacity, max(b, 2 * (0 if self._pat is None else self._pat.numel()))), self.device)
        return self._pat[a:b]

    def _fill(self, a, b, kind):
        if kind == "input":
            self.buf[a:b] = self.poison
            self.want[a:b] = self.poison
        else:
            p = self._pattern(a, b)
            self.buf[a:b] = p
            self.want[a:b] = p

    def place(self, nbytes, align=256, skew=0, kind="output", name=None, pitch=0, data=None):
        """A region of `nbytes` whose address is a multiple of `align` plus `skew`, a guard of guard_bytes(pitch) on both sides.
        kind "output": filled with the pattern (or with `data`: an output the kernel also reads, e.g. an in-place residual);
        "input": holds `data` (a tensor: its bytes are copied in), flanked by the poison, checked for equality by check();
        "workspace": like an output."""
        assert kind in KINDS, kind
        nbytes, align, skew = int(nbytes), int(align), int(skew)
        assert align >= 1 and _BASE_ALIGN % align == 0 and 0 <= skew, (align, skew)
        g = guard_bytes(pitch)
        g0 = self.used
        off = -(-(g0 + g) // align) * align + skew
        g1 = off + nbytes + g
        if g1 > self.capacity:
            raise MemoryError(f"guard-band arena of {self.capacity} bytes is too small for region '{name}' ({nbytes} bytes + 2 guards of {g})")
        r = Region(self, name or f"r{len(self.regions)}", kind, off, nbytes, g0, g1)
        self._fill(g0, off, kind)
        self._fill(off + nbytes, g1, kind)
        if data is not None:
            raw = data.contiguous().reshape(-1).view(torch.uint8) if data.numel() else torch.empty((0,), dtype=torch.uint8)
            assert raw.numel() == nbytes, (r.name, raw.numel(), nbytes)
            self.buf[off:off + nbytes] = raw.to(self.device)
            self.want[off:off + nbytes] = self.buf[off:off + nbytes]
        else:
            assert kind != "input", "an input region needs data"
            self._fill(off, off + nbytes, "output")
        self.regions.append(r)
        self.used = g1
        return r

    def _scan(self, a, b):
        """(first, last, count) of the changed bytes in [a, b), as arena offsets, or None"""
        if b <= a:
            return None
        idx = torch.nonzero(self.buf[a:b] != self.want[a:b]).reshape(-1)
        if idx.numel() == 0:
            return None
        return a + int(idx[0]), a + int(idx[-1]), int(idx.numel())

    def check(self):
        """Compare every guard and every input with what it must hold; one whole-arena comparison when nothing is wrong."""
        for r in self.regions:
            if r.kind != "input":   # whatever the kernel wrote into its own regions is not this check's business
                self.want[r.off:r.off + r.nbytes] = self.buf[r.off:r.off + r.nbytes]
        if torch.equal(self.buf[:self.used], self.want[:self.used]):
            return Report([], [])
        guards, inputs = [], []
        for r in self.regions:
            for side, a, b in (("before", r.g0, r.off), ("after", r.off + r.nbytes, r.g1)):
                hit = self._scan(a, b)
                if hit:
                    guards.append({"region": r.name, "kind": r.kind, "side": side, "first": hit[0] - r.off, "last": hit[1] - r.off, "count": hit[2]})
            if r.kind == "input":
                hit = self._scan(r.off, r.off + r.nbytes)
                if hit:
                    inputs.append({"region": r.name, "first": hit[0] - r.off, "last": hit[1] - r.off, "count": hit[2]})
        return Report(guards, inputs)
