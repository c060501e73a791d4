"""The int8 attention core of a SmoothQuant decoder in two launches of asq_bmm_i8:

    P = rne(127 * softmax(q_scale * k_scale * sm_scale * (q . k^T)))     BMM_S8T_S8N_SOFTMAX_S8T: int8, 0 .. 127, the scores stay on chip
    O = sat_i8(rne(v_scale / (127 * out_scale) * (P . v)))               pv_bmm's alpha on ops.bmm_i8_kn: v is read as it is stored, [batch, Sk, d]

Grouped-query attention (q [..., Hq, Sq, d] over k, v [..., Hkv, Sk, d], Hq = r * Hkv) takes the same two launches and never expands k or v: the r heads of a
group become rows of one product, or share b through ASQ_BMM_B_GROUP (forward, _forward_gqa).  With layout="bshd" the operands are [B, S, H, d], as the
q/k/v projections write them, a token-by-token KV cache holds them and o_proj reads them: the same two launches on token-major addresses (_forward_bshd).

The reference stops at the two matmul modules and leaves the softmax between them to the caller (fp32 scores, eager softmax, a cast);
here the first product carries it as its epilogue.  The state dict is the two scalar buffers ``qk_bmm.a`` and ``pv_bmm.a`` (host-pinned,
following the module dtype, as in layers/nn/bmm.py).

What feeds it for a RoPE model (LLaMA, Mixtral, Baichuan-7B) is RopeQuantQKV: rotary embedding, the per-tensor int8 quantisers of q, k and v and the append to an
Int8KVCache in one launch (ops.rope_quantize_qkv), straight from the q/k/v projections' [B, S, H, d] outputs into the operands of layout="bshd".

A batch of sequences of different lengths takes a decode step in two launches: RopeQuantQKV with a RaggedInt8KVCache appends one token per sequence at its own
position (ops.rope_quantize_qkv_at), Int8Attention.decode attends over each sequence's own number of keys on the cache where it lies (ops.attn_decode_i8).

The same step on a paged cache -- fixed-size pages handed out from one pool, a block table per sequence, what a vLLM-style server keeps -- is RopeQuantQKV with a
PagedInt8KVCache (ops.rope_quantize_qkv_paged) and Int8Attention.decode_paged (ops.attn_decode_i8_paged): the same two launches, the same bytes.

A step that carries several tokens per sequence -- draft tokens to verify, a prompt chunk, a mixed batch -- is the same append followed by Int8Attention.extend /
extend_paged (ops.attn_extend_i8 / _paged): every token under a causal mask over its sequence's keys up to its own, one launch; cache.rewind drops what was rejected."""
import torch

from ... import ops
from .bmm import BMM_S8T_S8N_S8T, BMM_S8T_S8N_SOFTMAX_S8T


def _q8_tokens(q8, one):
    """q8 of Int8Attention's cache methods is the append's [B, Sq, Hq, d] (one: a decode step, Sq = 1); the ops check the rest"""
    if not torch.is_tensor(q8) or q8.dim() != 4 or (one and q8.shape[1] != 1):
        raise ValueError(f"q8 must be [B, {1 if one else 'Sq'}, Hq, d], got {list(getattr(q8, 'shape', []))}")


class Int8Attention(torch.nn.Module):
    def __init__(self, qk_alpha=1.0, pv_alpha=1.0, causal=True):
        super().__init__()
        self.qk_bmm = BMM_S8T_S8N_SOFTMAX_S8T(qk_alpha, causal)
        self.pv_bmm = BMM_S8T_S8N_S8T(pv_alpha)

    @property
    def causal(self):
        return self.qk_bmm.causal

    @staticmethod
    def from_scale(q_scale, k_scale, v_scale, out_scale, sm_scale=1.0, causal=True):
        mod = Int8Attention(causal=causal)
        mod.qk_bmm = BMM_S8T_S8N_SOFTMAX_S8T._with_alpha(q_scale * k_scale * sm_scale)
        mod.qk_bmm.causal = bool(causal)
        mod.pv_bmm = BMM_S8T_S8N_S8T._with_alpha(v_scale / (127 * out_scale))
        return mod

    def forward(self, q, k, v, layout="bhsd"):
        """q int8 [..., Sq, d], k and v int8 [..., Sk, d] with equal leading dims (flattened to the batch) -> int8 [..., Sq, d].
        Causal masking is bottom-right aligned (query m sees keys n <= m + Sk - Sq), so a decode step with a KV cache sees every key.
        P . V reads v where it is (ASQ_BMM_B_KN): no transposed copy; only a non-contiguous v is made contiguous first.
        Grouped-query attention: q [..., Hq, Sq, d] over k and v [..., Hkv, Sk, d] with equal dims before the heads and Hq = r * Hkv; query head h
        uses KV head h // r.  K and V are never expanded: see _forward_gqa.
        layout="bshd": q [B, Sq, Hq, d], k and v [B, Sk, Hkv, d] -> [B, Sq, Hq, d], the layout q/k/v projections write and o_proj reads; see _forward_bshd."""
        if layout == "bshd":
            return self._forward_bshd(q, k, v)
        if layout != "bhsd":
            raise ValueError(f"layout must be 'bhsd' or 'bshd', got {layout!r}")
        if q.dim() < 2 or k.shape != v.shape or q.shape[-1] != k.shape[-1]:
            raise ValueError(f"shape mismatch: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        lead, sq, d, sk = q.shape[:-2], q.shape[-2], q.shape[-1], k.shape[-2]
        gqa = lead != k.shape[:-2]
        if gqa and (q.dim() < 3 or k.dim() != q.dim() or q.shape[:-3] != k.shape[:-3] or k.shape[-3] == 0 or q.shape[-3] % k.shape[-3] != 0):
            raise ValueError(f"shape mismatch: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        v3 = v.reshape(-1, sk, d)
        if not v3.is_contiguous():
            v3 = v3.contiguous()
        if gqa:
            return self._forward_gqa(q, k.reshape(-1, sk, d), v3, q.shape[-3] // k.shape[-3]).view(*lead, sq, d)
        p = self.qk_bmm(q.reshape(-1, sq, d), k.reshape(-1, sk, d))
        return ops.bmm_i8_kn(p, v3, torch.int8, self.pv_bmm._alpha()).view(*lead, sq, d)

    def _forward_gqa(self, q, k3, v3, r):
        """r > 1 query heads per KV head; k3, v3 [B * Hkv, Sk, d] -> [B * Hkv, r * Sq, d], which is [B * Hq, Sq, d].
        fold (not causal, or Sq == 1): the rows of a product are independent, so the r heads of a group are the r * Sq rows of ONE ungrouped product per KV
        head -- K and V are read once per KV head, and a decode step fills r of the narrow kernels' 16 rows.  A causal module with Sq == 1 sees every key
        (bottom-right alignment); the flag is dropped for the call, since with M = r rows it would hide keys.
        grouped (causal, Sq > 1): the mask depends on a row's position in its own head, so the heads stay batch entries and share b (b_group = r)."""
        sq, d = q.shape[-2], q.shape[-1]
        qk_alpha, pv_alpha = self.qk_bmm._alpha(), self.pv_bmm._alpha()
        if not self.causal or sq == 1:
            p = ops.bmm_i8_softmax_q8(q.reshape(-1, r * sq, d), k3, qk_alpha, False)
            return ops.bmm_i8_kn(p, v3, torch.int8, pv_alpha)
        p = ops.bmm_i8_softmax_q8(q.reshape(-1, sq, d), k3, qk_alpha, True, b_group=r)
        return ops.bmm_i8_kn(p, v3, torch.int8, pv_alpha, b_group=r)

    def _forward_bshd(self, q, k, v):
        """q [B, Sq, Hq, d], k and v [B, Sk, Hkv, d], Hq = r * Hkv, each contiguous -> [B, Sq, Hq, d]: the two launches read the projections where they lie and
        write o_proj's input in place (ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN), bit-identical to the head-major forward on permuted copies.  No operand is
        copied; only P, [B * Hq, Sq, Sk], is dense.
        Sq > 1, or r == 1: the heads are batch entries, sharing K / V through b_group = r when r > 1.
        Sq == 1 and r > 1 (a decode step): the r heads of a group are the r dense rows of q.view(B * Hkv, r, d), folded as in _forward_gqa -- only K and V are
        token-major (heads = Hkv, no group), the causal flag is dropped, and the dense [B * Hkv, r, d] result is [B, 1, Hq, d].
        With B == 1 the first Sk tokens of a preallocated [1, Smax, Hkv, d] cache are contiguous: a single-sequence decode step takes cache[:, :Sk] as it is."""
        if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3] or k.shape[2] == 0 or q.shape[2] % k.shape[2] != 0:
            raise ValueError(f"shape mismatch: q {tuple(q.shape)} must be [B, Sq, Hq, d], k {tuple(k.shape)} and v {tuple(v.shape)} [B, Sk, Hkv, d] with Hq a multiple of Hkv")
        bsz, sq, hq, d = q.shape
        hkv = k.shape[2]
        r = hq // hkv
        qk_alpha, pv_alpha = self.qk_bmm._alpha(), self.pv_bmm._alpha()
        if not q.is_contiguous():   # (k and v: the ops look; q is viewed below)
            raise ValueError("q, k and v must be contiguous in the bshd layout (make a slice of a fused q|k|v buffer contiguous first)")
        if hkv == 1 and (hq == 1 or sq == 1):   # one head per sequence is the dense layout itself: [B, S, 1, d] = [B, S, d]
            return self.forward(q.view(bsz, hq, sq, d), k.reshape(bsz, 1, -1, d), v.reshape(bsz, 1, -1, d)).view(bsz, sq, hq, d)
        if sq == 1 and r > 1:
            p = ops.bmm_i8_softmax_q8(q.view(bsz * hkv, r, d), k, qk_alpha, False, heads=hkv)
            return ops.bmm_i8_kn(p, v, torch.int8, pv_alpha, heads=hkv).view(bsz, 1, hq, d)
        p = ops.bmm_i8_softmax_q8(q, k, qk_alpha, self.causal, b_group=r)
        return ops.bmm_i8_kn(p, v, torch.int8, pv_alpha, b_group=r, out_token=True, heads=hq)

    def decode(self, q8, k_cache, v_cache, kv_len=None, max_len=None):
        """One decode step of a ragged batch in ONE launch (ops.attn_decode_i8): q8 int8 [B, 1, Hq, d] -> [B, 1, Hq, d] over k_cache / v_cache [B, Smax, Hkv, d], read
        where they lie (a RaggedInt8KVCache's k and v, or [:, :n] views), sequence b attending its first kv_len[b] keys (int32 [B] on the device; None: max_len
        each) with qk_bmm's and pv_bmm's alphas.  A decode step sees every key it is given, so the causal flag does not apply.  max_len: a bound on the lengths
        (cache.bound()), the caches' rows when absent.  With few sequences x KV heads (a single sequence) the launch leaves most of the chip idle: forward(layout=
        "bshd") remains the route there."""
        _q8_tokens(q8, one=True)
        return ops.attn_decode_i8(q8, k_cache, v_cache, kv_len, self.qk_bmm._alpha(), self.pv_bmm._alpha(), max_len=max_len)

    def decode_paged(self, q8, k_pool, v_pool, block_table, kv_len=None, max_len=None):
        """decode on a paged cache, ONE launch (ops.attn_decode_i8_paged): q8 int8 [B, 1, Hq, d] -> [B, 1, Hq, d] over k_pool / v_pool [num_pages, page_size, Hkv, d]
        (a PagedInt8KVCache's k and v), key n of sequence b in page block_table[b, n // page_size] (int32 [B, T] on the device).  kv_len and max_len as in decode
        (max_len: T * page_size when absent).  The output bytes are decode's on a contiguous cache holding the same keys."""
        _q8_tokens(q8, one=True)
        return ops.attn_decode_i8_paged(q8, k_pool, v_pool, block_table, kv_len, self.qk_bmm._alpha(), self.pv_bmm._alpha(), max_len=max_len)

    def extend(self, q8, k_cache, v_cache, kv_len=None, q_len=None, max_len=None):
        """A step of several tokens per sequence under a causal mask in ONE launch (ops.attn_extend_i8): q8 int8 [B, Sq, Hq, d] -> [B, Sq, Hq, d], the append's q8 over the
        caches the append has just written (kv_len includes the new tokens).  Sequence b brings q_len[b] tokens (int32 [B] on the device, right-padded; None: Sq each);
        token s sits at key position kv_len[b] - q_len[b] + s and sees the keys up to and including its own; padded tokens get zero rows.  The verification of draft
        tokens (followed by cache.rewind of the rejected ones), a prompt chunk, a mixed batch.  With Sq * r <= 16 the step costs about one decode launch; a long prefill
        stays with forward(layout="bshd")."""
        _q8_tokens(q8, one=False)
        return ops.attn_extend_i8(q8, k_cache, v_cache, kv_len, self.qk_bmm._alpha(), self.pv_bmm._alpha(), q_len=q_len, max_len=max_len)

    def extend_paged(self, q8, k_pool, v_pool, block_table, kv_len=None, q_len=None, max_len=None):
        """extend on a paged cache, ONE launch (ops.attn_extend_i8_paged): the pools and the table as in decode_paged, q8, q_len and the per-token rule as in extend.  The
        output bytes are extend's on a contiguous cache holding the same keys."""
        _q8_tokens(q8, one=False)
        return ops.attn_extend_i8_paged(q8, k_pool, v_pool, block_table, kv_len, self.qk_bmm._alpha(), self.pv_bmm._alpha(), q_len=q_len, max_len=max_len)


class Int8KVCache:
    """A preallocated int8 KV cache in the token-major layout: k and v [B, Smax, Hkv, d] and the number of tokens held, `length` (one position for the whole batch).
    Plain tensor bookkeeping, on any device: slot(S) -> the views k[:, length:length + S], v[...] that the next S tokens are written into (ValueError past
    max_len), advance(S) -> length += S, view() -> k[:, :length], v[:, :length], reset() -> length = 0.  Nothing is copied; every view aliases the buffers.
    With B == 1 view() is contiguous and is what Int8Attention(layout="bshd") takes as it is; see RopeQuantQKV for B > 1."""

    def __init__(self, batch, max_len, kv_heads, head_dim, device=None):
        self.k = torch.zeros((batch, max_len, kv_heads, head_dim), dtype=torch.int8, device=device)
        self.v = torch.zeros_like(self.k)
        self.length = 0

    @property
    def max_len(self):
        return self.k.shape[1]

    def slot(self, S):
        if S < 0 or self.length + S > self.max_len:
            raise ValueError(f"Int8KVCache: {S} more tokens after {self.length} do not fit max_len {self.max_len}")
        return self.k[:, self.length:self.length + S], self.v[:, self.length:self.length + S]

    def advance(self, S):
        self.slot(S)
        self.length += S

    def view(self):
        return self.k[:, :self.length], self.v[:, :self.length]

    def reset(self):
        self.length = 0


class _SequenceLengths:
    """The length bookkeeping RaggedInt8KVCache and PagedInt8KVCache share: `kv_len` int32 [batch] on the cache's device -- allocated once and only written in place by
    stream-ordered ops, so a captured step replays as the lengths move -- and its host mirror `lengths`, a list of ints, which serves every bounds check (ValueError, no
    device sync).  `max_len`, the rows a sequence can hold, is the subclass's.  A step S is an int (every sequence) or one int per sequence.  _steps checks and changes
    nothing, so a caller that runs its checks before _move keeps "a refused call changes no state"."""

    def _init_lengths(self, batch, device):
        self.kv_len = torch.zeros((batch,), dtype=torch.int32, device=device)
        self.lengths = [0] * batch

    def _steps(self, S, who, back=False):
        """S as a list of ints; ValueError under `who`'s name for a wrong count, a negative step and one beyond max_len (back: beyond the sequence's length)"""
        steps = [S] * len(self.lengths) if isinstance(S, int) else [int(s) for s in S]
        if len(steps) != len(self.lengths) or any(s < 0 or (s > n if back else n + s > self.max_len) for s, n in zip(steps, self.lengths)):
            if back:
                raise ValueError(f"{who}: {steps} tokens cannot be taken back from {len(self.lengths)} sequences of lengths {self.lengths}")
            raise ValueError(f"{who}: {steps} more tokens after {self.lengths} do not fit {len(self.lengths)} sequences of max_len {self.max_len}")
        return steps

    def _move(self, S, steps, back=False):
        """lengths += steps (back: -=): one stream-ordered add_ (sub_) on kv_len -- of the int S as the caller gave it, else of the steps sent over without a sync"""
        delta = S if isinstance(S, int) else torch.tensor(steps, dtype=torch.int32).to(self.kv_len.device, non_blocking=True)
        if back:
            self.kv_len.sub_(delta)
            self.lengths = [n - s for n, s in zip(self.lengths, steps)]
        else:
            self.kv_len.add_(delta)
            self.lengths = [n + s for n, s in zip(self.lengths, steps)]

    def _reset_lengths(self, b):
        """sequence b, or with None every sequence, back to length 0 -> the indices reset"""
        if b is None:
            self.kv_len.zero_()
            seqs = range(len(self.lengths))
        else:
            b = range(len(self.lengths))[b]   # (IndexError outside, a negative index counts from the end)
            self.kv_len[b:b + 1].zero_()
            seqs = (b,)
        for i in seqs:
            self.lengths[i] = 0
        return seqs

    def bound(self):
        return max(self.lengths, default=0)


class RaggedInt8KVCache(_SequenceLengths):
    """Int8KVCache with a length per sequence: k and v [B, Smax, Hkv, d], `kv_len` int32 [B] on the cache's device -- what the kernels read: the append position of
    ops.rope_quantize_qkv_at, the number of keys of ops.attn_decode_i8, so a captured step replays as the lengths move -- and its host mirror `lengths`, a list of
    ints, which serves the bounds checks (ValueError, no device sync).
    advance(S): S an int (every sequence) or B ints -> lengths += S, one stream-ordered add_ on kv_len.  rewind(S): lengths -= S, one stream-ordered sub_ (the rejected
    tokens of a speculative step; ValueError, nothing changed, for a negative step or one beyond a length).  reset(b=None): every sequence, or sequence b, back to 0.
    rewind and reset forget, they do not clear.  bound() = max(lengths): a tighter max_len for attn_decode_i8 than the capacity."""

    def __init__(self, batch, max_len, kv_heads, head_dim, device=None):
        self.k = torch.zeros((batch, max_len, kv_heads, head_dim), dtype=torch.int8, device=device)
        self.v = torch.zeros_like(self.k)
        self._init_lengths(batch, device)

    @property
    def max_len(self):
        return self.k.shape[1]

    def advance(self, S):
        self._move(S, self._steps(S, "RaggedInt8KVCache"))

    def rewind(self, S):
        self._move(S, self._steps(S, "RaggedInt8KVCache", back=True), back=True)

    def reset(self, b=None):
        self._reset_lengths(b)


class PagedInt8KVCache(_SequenceLengths):
    """A paged int8 KV cache: pools k and v [num_pages, page_size, Hkv, d] (page_size a multiple of 16), `block_table` int32 [batch, ceil(max_len / page_size)] and
    `kv_len` int32 [batch] on the cache's device -- what ops.rope_quantize_qkv_paged and ops.attn_decode_i8_paged read; both are allocated once and only written in
    place, so a captured step keeps reading the same addresses -- and their host mirrors: `lengths`, the page list of every sequence `pages`, and the free list `free`
    (pages are handed out in ascending order at first, a freed page is the next one reused).  Memory follows the real lengths: a sequence holds ceil(n / page_size)
    pages once reserve() has covered its n tokens.
    reserve(S): the pages the next S tokens (an int, or one per sequence) need, taken from the free list and written into the table; ValueError before anything is
    touched when the pool or max_len does not suffice.  advance(S): lengths += S within what is reserved.  rewind(S): lengths -= S (the rejected tokens of a speculative
    step), the pages wholly behind ceil(length / page_size) back to the free list, newest first.  reset(b=None): every sequence, or sequence b, back to 0, its pages
    back to the free list.  rewind and reset forget, they do not clear; stale table entries stay behind the length, where no kernel reads them.  bound() = max(lengths).
    gather(b) -> sequence b's keys and values as contiguous [n_b, Hkv, d] tensors by plain torch indexing: for tests and for callers that want a sequence as one
    tensor (a step of several tokens runs on the pool in place: Int8Attention.extend_paged).  A refused call changes no state."""

    def __init__(self, num_pages, page_size, kv_heads, head_dim, batch, max_len, device=None):
        if num_pages < 0 or page_size <= 0 or page_size % 16 or batch < 0 or max_len < 0:
            raise ValueError(f"PagedInt8KVCache: {num_pages} pages of {page_size} rows (a positive multiple of 16) for {batch} sequences of max_len {max_len}")
        self.k = torch.zeros((num_pages, page_size, kv_heads, head_dim), dtype=torch.int8, device=device)
        self.v = torch.zeros_like(self.k)
        self.block_table = torch.zeros((batch, -(-max_len // page_size)), dtype=torch.int32, device=device)
        self._init_lengths(batch, device)
        self.max_len = max_len
        self.pages = [[] for _ in range(batch)]
        self.free = list(range(num_pages - 1, -1, -1))   # a stack: pop() hands out page 0 first, a freed page next

    @property
    def page_size(self):
        return self.k.shape[1]

    def reserve(self, S):
        steps = self._steps(S, "PagedInt8KVCache.reserve")
        need = [max(0, -(-(n + s) // self.page_size) - len(pg)) for n, s, pg in zip(self.lengths, steps, self.pages)]
        if sum(need) > len(self.free):
            raise ValueError(f"PagedInt8KVCache.reserve: {steps} more tokens after {self.lengths} need {sum(need)} more pages, {len(self.free)} are free")
        rows, cols, ids = [], [], []
        for b, m in enumerate(need):
            for _ in range(m):
                rows.append(b), cols.append(len(self.pages[b])), ids.append(self.free.pop())
                self.pages[b].append(ids[-1])
        if ids:   # one stream-ordered scatter of the changed entries
            dev = self.block_table.device
            self.block_table.index_put_((torch.tensor(rows).to(dev, non_blocking=True), torch.tensor(cols).to(dev, non_blocking=True)),
                                        torch.tensor(ids, dtype=torch.int32).to(dev, non_blocking=True))

    def _unreserve(self, held):
        """give back, newest first, the pages beyond held[b] per sequence: the free list is what it was before the reserve() that took them (their table entries stay,
        behind the lengths)"""
        for pg, m in zip(reversed(self.pages), reversed(held)):
            while len(pg) > m:
                self.free.append(pg.pop())

    def advance(self, S):
        steps = self._steps(S, "PagedInt8KVCache.advance")
        if any(n + s > len(pg) * self.page_size for n, s, pg in zip(self.lengths, steps, self.pages)):
            raise ValueError(f"PagedInt8KVCache.advance: {steps} more tokens after {self.lengths} go beyond the reserved pages {[len(pg) for pg in self.pages]}")
        self._move(S, steps)

    def rewind(self, S):
        self._move(S, self._steps(S, "PagedInt8KVCache.rewind", back=True), back=True)
        self._unreserve([-(-n // self.page_size) for n in self.lengths])

    def reset(self, b=None):
        for i in self._reset_lengths(b):
            self.free.extend(reversed(self.pages[i]))
            self.pages[i] = []

    def gather(self, b):
        n = self.lengths[b]
        idx = torch.tensor(self.pages[b][:-(-n // self.page_size)], dtype=torch.long).to(self.k.device)
        return self.k[idx].flatten(0, 1)[:n].contiguous(), self.v[idx].flatten(0, 1)[:n].contiguous()


class RopeQuantQKV(torch.nn.Module):
    """Rotary embedding of q and k, the static per-tensor int8 quantisers of q, k and v (x / scale in x's dtype, round, clamp) and the KV-cache append as ONE launch
    (ops.rope_quantize_qkv): every byte is what ops.rope followed by ops.quantize_act(., "per-tensor-div", scale) gives.  The state dict is the three scalar buffers
    ``q_scale``, ``k_scale`` and ``v_scale`` (host-pinned, following the module dtype, as ``a`` in layers/nn/bmm.py); the kernel receives fp32(scale.item()).

    forward(q, k, v, cos, sin, pos=0, cache=None) -> (q8, k8, v8): q [B, S, Hq, d], k and v [B, S, Hkv, d] as the projections write them (dense or slices of a fused
    q || k || v output), cos / sin [T, d/2] tables indexed by absolute position.  Without a cache the tokens sit at positions pos .. pos + S - 1 and k8 / v8 are fresh
    dense tensors.  With an Int8KVCache the position is cache.length (`pos` is not used), k / v are written into cache.slot(S), the cache advances, and k8 / v8 are
    cache.view(): all tokens so far, which Int8Attention(...)(q8, k8, v8, layout="bshd") consumes -- a prefill and every decode step alike.

    Int8Attention's bshd path needs contiguous K / V, which a cache view is for B == 1 (the single-sequence decode step attention.py documents); for B > 1 an Int8KVCache
    still appends correctly (the cache's batch pitch goes to the kernel), but its views are made contiguous before forward(layout="bshd") takes them.

    With a RaggedInt8KVCache (B >= 1 sequences of different lengths) token (b, s) sits at position cache.kv_len[b] + s, read on the device (ops.rope_quantize_qkv_at; `pos`
    is not used); the cache then advances by `advance` -- S tokens per sequence when absent, an int or B ints otherwise -- and the call returns (q8, cache.k, cache.v),
    the whole caches, which Int8Attention.decode(q8, cache.k, cache.v, cache.kv_len) reads in place.  A padded prefill is one call on a fresh cache with S = the longest
    prompt and advance = the true lengths: the next appends overwrite the pad rows, which no decode step reads.

    With a PagedInt8KVCache the same, on pages: the cache reserves the pages the S written rows need (ValueError before anything is launched when the pool or max_len
    does not suffice), the append goes through ops.rope_quantize_qkv_paged, the cache advances, and the call returns (q8, cache.k, cache.v), the pools, which
    Int8Attention.decode_paged(q8, cache.k, cache.v, cache.block_table, cache.kv_len) reads in place."""

    _SCALES = ("q_scale", "k_scale", "v_scale")

    def __init__(self, q_scale=1.0, k_scale=1.0, v_scale=1.0):
        super().__init__()
        for name, s in zip(self._SCALES, (q_scale, k_scale, v_scale)):
            self.register_buffer(name, s.detach().clone() if torch.is_tensor(s) else torch.tensor(s))
        self._pin()

    def _pin(self):
        for name in self._SCALES:
            t = self._buffers.get(name)
            if t is not None and t.device.type != "cpu":
                self._buffers[name] = t.detach().to("cpu")

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._pin()
        return self

    def _scales(self):
        self._pin()   # a device tensor assigned from outside: one copy, then host reads are free
        return tuple(self._buffers[name].item() for name in self._SCALES)

    def forward(self, q, k, v, cos, sin, pos=0, cache=None, advance=None):
        qs, ks, vs = self._scales()
        if cache is None:
            return ops.rope_quantize_qkv(q, k, v, cos, sin, qs, ks, vs, pos=pos)
        S = q.shape[1] if torch.is_tensor(q) and q.dim() == 4 else 0
        if isinstance(cache, RaggedInt8KVCache):
            cache._steps(S, "RaggedInt8KVCache")                # the S written rows fit every sequence ...
            steps = cache._steps(S if advance is None else advance, "RaggedInt8KVCache")   # ... and so does what the cache advances by (ValueError before anything is launched)
            q8, _, _ = ops.rope_quantize_qkv_at(q, k, v, cos, sin, qs, ks, vs, cache.kv_len, cache.k, cache.v)
            cache.advance(S if advance is None else steps)
            return q8, cache.k, cache.v
        if isinstance(cache, PagedInt8KVCache):
            cache._steps(S, "PagedInt8KVCache.reserve")
            steps = cache._steps(S if advance is None else advance, "PagedInt8KVCache.advance")
            if any(a > S for a in steps):
                raise ValueError(f"PagedInt8KVCache: advance {steps} goes beyond the {S} rows written")
            held = [len(pg) for pg in cache.pages]
            cache.reserve(S)
            try:
                q8, _, _ = ops.rope_quantize_qkv_paged(q, k, v, cos, sin, qs, ks, vs, cache.kv_len, cache.block_table, cache.k, cache.v, max_len=cache.max_len)
            except Exception:
                cache._unreserve(held)   # a refused append keeps no page
                raise
            cache.advance(S if advance is None else steps)
            return q8, cache.k, cache.v
        k_out, v_out = cache.slot(S)
        q8, _, _ = ops.rope_quantize_qkv(q, k, v, cos, sin, qs, ks, vs, pos=cache.length, k_out=k_out, v_out=v_out)
        cache.advance(S)
        k8, v8 = cache.view()
        return q8, k8, v8
