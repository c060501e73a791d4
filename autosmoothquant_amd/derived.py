"""Operands derived from weights: the one statement of when they are built, rebuilt and left alone.

A derived operand is a tensor (or tuple of tensors) computed from weights and handed to a kernel in their place: a linear's offset image, GateUpSiLU's interleaved
gate || up operand and its image, MixtralLayer's expert-stack images and its w1 || w3 operand with its image.  A hipGraph captured on one bakes its buffers in, so:
  * it is keyed on its sources' storage, version counter and device: in-place torch writes, .to() and re-homed buffers are seen by the next eager `get`;
  * it is never built inside a capture (a buffer filled there would only exist after the first replay);
  * it is rebuilt INTO its buffers while they fit, so a captured graph keeps valid pointers and replays the new content;
  * a source without a version counter (an inference tensor) gets one only after `pin()`: writes are invisible, the caller owns the `refresh`;
  * running out of memory while building drops it and sets `failed`; the owner maps that to its switch and runs on plain operands;
  * `refresh` = forget the key, rebuild in place.
An operand derived from ANOTHER derived operand (the image of gate || up, of w1 || w3) is keyed on the original weights too and names what it reads as `inputs`: a
rebuild through the C-ABI bumps no version counter, so the intermediate operand cannot serve as the key.
"""
import torch


def _first(buffers):
    return buffers if isinstance(buffers, torch.Tensor) else buffers[0]


class DerivedOperand:
    """State only (no reference to the owner, so copies of a module rebuild for themselves): sources, builder and shape come with every call.
    build(*inputs, out=None or the buffers to fill) -> buffers; inputs default to the sources; shape is that of the first buffer (default: of the first source)."""
    __slots__ = ("key", "buffers", "retired", "pinned", "stale", "failed")

    def __init__(self):
        self.key = self.buffers = None
        self.retired = []      # buffers given up by adopt(): kept allocated, graphs captured on them replay on valid memory (no longer refreshed)
        self.pinned = self.stale = self.failed = False

    def _fit(self, buffers, sources, shape):
        b = _first(buffers)
        return b.device == sources[0].device and tuple(b.shape) == tuple(sources[0].shape if shape is None else shape)

    def get(self, sources, build, shape=None, inputs=None):
        """the current buffers, or None: unpinned sources without a version counter, a (re)build needed inside a capture, out of memory (`failed` is set).
        A hit costs the key and one comparison -- no other torch call (a forward takes this path per module and call)."""
        key = ()   # (formed here and nowhere else, inline: a call more is a tenth of the hit path)
        for t in sources:
            try:
                key += (t.data_ptr(), t._version, t.device)
            except RuntimeError:   # an inference tensor has no version counter: writes into it cannot be seen
                key += (t.data_ptr(), None, t.device)
        if key == self.key and not self.stale:
            return self.buffers
        if None in key and not self.pinned:
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        old = self.buffers
        try:
            self.buffers = build(*(sources if inputs is None else inputs), out=old if old is not None and self._fit(old, sources, shape) else None)
        except torch.cuda.OutOfMemoryError:
            self.key = self.buffers = None
            self.failed = True
            return None
        self.key, self.stale, self.failed = key, False, False
        return self.buffers

    def pin(self):
        """opt in for sources without a version counter: the caller refreshes after writing them"""
        self.pinned = True

    def invalidate(self):
        """the next eager get rebuilds into the same buffers"""
        self.stale = True

    def refresh(self, sources, build, shape=None, inputs=None):
        """invalidate + get; False when nothing is held, and inside a capture (nothing is built there: the operand stays stale for the next eager get)"""
        if self.buffers is None:
            return False
        self.stale = True
        return self.get(sources, build, shape, inputs) is not None

    def adopt(self, buffers, sources, build, shape=None, inputs=None):
        """make `buffers` (someone else's memory, e.g. a slice of a stacked operand) this operand's and build into them now; None when they do not fit"""
        if not self._fit(buffers, sources, shape):
            return None
        if self.buffers is not None and _first(self.buffers).data_ptr() != _first(buffers).data_ptr():
            self.retired.append(self.buffers)
        self.buffers, self.stale = buffers, True
        return self.get(sources, build, shape, inputs)


def scale_vector(cache, vals, sizes, device, capturing=False):
    """Host scalars as one fp32 device vector: vals[i] repeated sizes[i] times.  cache: the (key, vector) pair this returned last time, or None; returns the pair to keep
    (the same one while values, sizes and device are unchanged), or None when a new vector would have to be built inside a capture."""
    key = (vals, sizes, str(device))
    if cache is None or cache[0] != key:
        if capturing:
            return None
        cache = (key, torch.cat([torch.full((int(n),), v, dtype=torch.float32) for v, n in zip(vals, sizes)]).to(device))
    return cache
