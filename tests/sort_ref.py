"""Plain numpy references for csrc/radix_sort.h (tests/test_radix_sort.py): the stable LSD sort of (u32 key, u32 value)
pairs, the per-row exclusive scan of the digit histograms, and the weight sum the one-sweep histogram leaves."""
import numpy as np

SENTINEL = 0xFFFFFFFF


def sort_mask(bits: int) -> int:
    """Both sort forms work in whole 8-bit digits: `bits` key bits mean ceil(bits / 8) passes, so the low
    8 * ceil(bits / 8) bits decide the order (bits = 10 sorts by 16 bits, bits = 17 by 24)."""
    return (1 << (8 * ((bits + 7) // 8))) - 1


def ref_sort(keys, vals, n: int, bits: int, drop: bool):
    """(sorted keys, sorted values) of the first n elements; drop: the elements keyed 0xFFFFFFFF leave first.
    Stable by key & sort_mask(bits); the keys come out unmasked; vals None: the values are the original indices."""
    keys = np.asarray(keys, dtype=np.uint32)[:n]
    vals = np.arange(n, dtype=np.uint32) if vals is None else np.asarray(vals, dtype=np.uint32)[:n]
    if drop:
        keep = keys != np.uint32(SENTINEL)
        keys, vals = keys[keep], vals[keep]
    order = np.argsort(keys & np.uint32(sort_mask(bits)), kind="stable")
    return keys[order], vals[order]


def ref_scan(rows, used: int):
    """rows: [R, stride] u32. Returns (rows with the first `used` entries of every row replaced by their exclusive
    cumulative sum modulo 2^32 and the later entries unchanged, the per-row total modulo 2^32 of those entries)."""
    rows = np.asarray(rows, dtype=np.uint32)
    out = rows.copy()
    inc = np.cumsum(rows[:, :used].astype(np.uint64), axis=1)          # < 2^13 * 2^32: exact in 64 bits
    totals = (inc[:, -1] if used else np.zeros(rows.shape[0], np.uint64)) & np.uint64(0xFFFFFFFF)
    out[:, :used] = ((inc - rows[:, :used]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out, totals.astype(np.uint32)


def ref_weight(rects, keys, n: int) -> int:
    """64-bit sum of (w * h) over the first n elements whose key is not the sentinel; a rectangle is packed as
    x0 | y0 << 8 | (w - 1) << 16 | (h - 1) << 24."""
    r = np.asarray(rects, dtype=np.uint32)[:n].astype(np.uint64)
    keep = np.asarray(keys, dtype=np.uint32)[:n] != np.uint32(SENTINEL)
    w = (((r >> np.uint64(16)) & np.uint64(255)) + np.uint64(1)) * ((r >> np.uint64(24)) + np.uint64(1))
    return int(w[keep].sum(dtype=np.uint64))
