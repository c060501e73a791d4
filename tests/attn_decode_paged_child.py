"""The paged decode tests' helper and device runs, as functions (tests/test_hip_attn_decode_paged.py calls them at the default 8 waves) and as a script:

    ASQ_DECODE_WAVES=4 python tests/attn_decode_paged_child.py 4

scatter() lays a contiguous [B, rows, Hkv, D] cache out as a pool of pages under a seeded page permutation, the pages of different sequences interleaved; the
unused pages, the rows of each last page at and behind n_b and the pitch gap hold the "wins its row outright" key of attn_decode_ref.poisoned and V of +-127.
The library reads ASQ_DECODE_WAVES once per process (tests/attn_decode_child.py), so the 4-wave and 16-wave kernels need a process of their own: as a script this
runs the key-position walk built for its own number of waves at page size 16 through the paged entry, bit-equal to the expected bytes (WALK[2] and WALK[3] have D > 128:
at 16 waves they take the documented fallback to 8).  The first failing message goes to stdout and the exit code is 1."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import attn_decode_ref as R  # noqa: E402
from bmm_ref import assert_bits_equal  # noqa: E402

DEV = "cuda:0"
EXACT_PVS = (1.0 / 127, 0.003)
SPARE_PAGES, SPARE_COLS = 3, 2


def scatter(qn, kn, vn, n_b, P, ml, seed, gap=0, behind=0, share=None):
    """kn, vn: [B, >= n_b rows, Hkv, D] numpy caches, sequence b holding n_b[b] keys; ml: the max_len the table is sized for (ceil(ml / P) entries wide, inside a table
    SPARE_COLS wider).  -> (k_pool, v_pool as [num_pages, P, Hkv, D] device views of pools with P + gap rows per page, the [B, T] device view of the table, the host table).
    behind: the id written into every entry behind a sequence's last page (the spare columns included).  share = (b, b2, pages): sequence b2's first `pages` entries
    name sequence b's pages (the caller has made those keys equal)."""
    B, _, hkv, d = kn.shape
    r = qn.shape[1] // hkv
    width = -(-ml // P)
    used = [-(-int(n) // P) for n in n_b]
    num_pages = sum(used) + SPARE_PAGES
    rng = np.random.default_rng(seed)
    perm = list(rng.permutation(num_pages))
    rows = P + gap

    def poison(b):
        j = np.arange(rows)
        return np.stack([np.clip(127 * np.sign(qn[b, g * r + j % r].astype(np.int64)), -128, 127) for g in range(hkv)], axis=1).astype(np.int8)      # [rows, Hkv, D]

    pois = [poison(b) for b in range(B)]
    kp = np.stack([pois[p % B] for p in range(num_pages)])
    vp = (127 * rng.choice([-1, 1], kp.shape)).astype(np.int8)
    tab = np.full((B, width + SPARE_COLS), behind, dtype=np.int64)
    for j in range(max(used, default=0)):
        for b in range(B):
            if j >= used[b]:
                continue
            if share is not None and b == share[1] and j < share[2]:
                tab[b, j] = tab[share[0], j]
                continue
            page = perm.pop()
            tab[b, j] = page
            m = min(P, int(n_b[b]) - j * P)
            kp[page] = pois[b]
            kp[page, :m], vp[page, :m] = kn[b, j * P:j * P + m], vn[b, j * P:j * P + m]
    host = tab.astype(np.int32)
    k_pool, v_pool = (torch.from_numpy(x).to(DEV)[:, :P] for x in (kp, vp))
    return k_pool, v_pool, torch.from_numpy(host).to(DEV)[:, :width], host


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def run_paged(q, k_pool, v_pool, table, lengths, qk_alpha, pv_alpha, max_len, kv_len="lengths"):
    from autosmoothquant_amd import ops
    if isinstance(kv_len, str):
        kv_len = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    out = ops.attn_decode_i8_paged(q, k_pool, v_pool, table, kv_len, qk_alpha, pv_alpha, max_len=max_len)
    assert out.dtype == torch.int8 and out.shape == q.shape and out.is_contiguous()
    return out.cpu().numpy()


def exact(made, P, want, what, seed, gap=0):
    """a constructed case of attn_decode_ref (q, k, v, lengths, alpha, max_len, ...) scattered with page size P, bit for bit against want(pv_alpha)"""
    qn, kn, vn, lengths, alpha, ml = made[:6]
    kp, vp, tab, _ = scatter(qn, kn, vn, lengths, P, ml, seed, gap=gap, behind=-1)
    q, = dev(qn)
    for pv in EXACT_PVS:
        assert_bits_equal(run_paged(q, kp, vp, tab, lengths, alpha, pv, ml), want(pv), f"{what}, page size {P}, pv_alpha {pv}")


def walk(i, nw, P):
    hkv, r, d, tail = R.WALK[i]
    n, C, pos = R.walk_positions(r, nw, tail)
    made = R.walk_case(i, nw)
    print(f"walk {R.WALK[i][:3]} for {nw} waves, page size {P}: {n} keys in chunks of {C}, hot keys at {pos}")
    exact(made, P, lambda pv: R.one_hot_expected(made[2], made[6], pv), f"key-position walk {R.WALK[i][:3]} for {nw} waves (sequence b: the hot key at {pos}[b])", 52800 + i)


def two_weights(i, neg, P):
    made = R.two_weight_case(i, neg)
    r = made[0].shape[1] // made[1].shape[2]
    exact(made, P, lambda pv: R.two_weight_expected(made[2], made[6], r, pv), f"two weights {R.WALK[i][:3]}, qk_alpha {made[4]:+.4f} (34 v[A] + 93 v[B])", 52810 + i)


def main(argv):
    nw = int(argv[1])
    assert nw in (4, 16), nw
    assert os.environ.get("ASQ_DECODE_WAVES") == str(nw), f"ASQ_DECODE_WAVES is {os.environ.get('ASQ_DECODE_WAVES')!r}, not {nw}"
    assert not any(m.startswith("autosmoothquant_amd") for m in sys.modules), "the package was imported before the override was checked"
    try:
        for i in range(4):
            walk(i, nw, 16)
    except AssertionError as e:
        print(f"FAILED at {nw} waves: {e}")
        return 1
    print(f"{nw} waves: all passed")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
