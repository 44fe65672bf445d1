"""The definition of a bitmap carried through a compaction (coltt_hnsw_compact_carry), in numpy, and the tombstone patterns its tests share."""
import numpy as np

TILE_SLOTS = 32768          # the output tile of filter_carry_kernel / filter_compact_kernel: FEX_TILE_WORDS words
N_BIG = 3 * TILE_SLOTS + 37


def pack(flags):
    """bool [n] -> uint32 words, bit s % 32 of word s // 32"""
    n = len(flags)
    pad = np.zeros(((n + 31) // 32) * 32, np.uint8)
    pad[:n] = flags
    return np.packbits(pad, bitorder="little").view(np.uint32).copy() if n else np.zeros(0, np.uint32)


def unpack(words, n):
    """uint32 words -> bool [n]; words the bitmap lacks read as 0"""
    w = np.zeros((n + 31) // 32, np.uint32)
    m = min(len(w), len(words))
    w[:m] = np.asarray(words, np.uint32)[:m]
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def carry_numpy(words, dead, n):
    """(out words, allowed, live): the bits of the live slots, in their order, repacked"""
    live = ~np.asarray(dead, bool)[:n]
    kept = unpack(words, n)[live]
    return pack(kept), int(kept.sum()), int(live.sum())


def dead_patterns(n):
    rng = np.random.default_rng(4000 + n)
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": (np.arange(n) & 1).astype(bool)}
    run = np.zeros(n, bool)
    # a dead run of 40 000 — longer than one output tile — from slot 20 000 on: the survivors around it land in output tile 0 and the run's
    # source words straddle the boundary between the first two source tiles
    run[min(n, 20000):min(n, 60000)] = True
    pats["run-40000"] = run
    for p in (0.01, 0.5, 0.99):
        pats[f"random-{p}"] = rng.random(n) < p
    return pats
