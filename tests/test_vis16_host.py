"""The 16-bit visited set of the row-filter walk is EXACT (coltt_amd/csrc/vis16.hpp).

The header is compiled with the host compiler — the very functions the kernel runs, with the sequential compare-and-swap — and driven against a
Python set: membership answers, the stash, the overflow report and the decoding of (bucket, entry) back to the slot."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEN, NEW, FULL = 0, 1, 2
BBITS = 10           # the library's table: 1024 buckets of 8 entries
STASH = 16
OCC, SECOND, TAG_MASK = 0x8000, 0x4000, 0x3FFF


@pytest.fixture(scope="module")
def v16(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "the header is checked as compiled code: g++ is needed"
    d = tmp_path_factory.mktemp("v16")
    src = d / "v16.cpp"
    src.write_text('#include "vis16.hpp"\n'
                   'using namespace coltt;\n'
                   'extern "C" uint32_t v16_hash(uint32_t s, uint32_t b) { return vis16_hash(s, b); }\n'
                   'extern "C" uint32_t v16_unhash(uint32_t h, uint32_t b) { return vis16_unhash(h, b); }\n'
                   'extern "C" uint32_t v16_g(uint32_t t, uint32_t b) { return vis16_g(t, b); }\n'
                   'extern "C" uint32_t v16_decode(uint32_t bucket, uint32_t e, uint32_t b) { return vis16_decode(bucket, e, b); }\n'
                   'extern "C" uint32_t v16_consts(int i) { const uint32_t c[] = {VIS16_STASH, VIS16_BUCKET_BITS, VIS16_MAX_SLOTS, VIS16_OCC, VIS16_SECOND, VIS16_TAG_MASK}; return c[i]; }\n'
                   '// out[i] = the answer for slots[i]; *hwm = the largest stash count seen\n'
                   'extern "C" void v16_insert_many(uint32_t* tab, uint32_t* stash, uint32_t* n, uint32_t b, const uint32_t* slots, uint32_t cnt, int32_t* out, uint32_t* hwm) {\n'
                   '  for (uint32_t i = 0; i < cnt; i++) { out[i] = vis16_insert(tab, stash, *n, b, slots[i]); if (*n > *hwm) *hwm = *n; }\n'
                   '}\n')
    so = d / "libv16.so"
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "coltt_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    for f in ("v16_hash", "v16_unhash", "v16_g"):
        getattr(L, f).restype = C.c_uint32; getattr(L, f).argtypes = [C.c_uint32, C.c_uint32]
    L.v16_decode.restype = C.c_uint32; L.v16_decode.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.v16_consts.restype = C.c_uint32; L.v16_consts.argtypes = [C.c_int]
    L.v16_insert_many.restype = None
    L.v16_insert_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


class Table:
    def __init__(self, L, bbits=BBITS):
        self.L, self.bbits = L, bbits
        raw = np.zeros((4 << bbits) + 4, np.uint32)          # the kernel's table is 16-byte aligned (one bucket = one 128-bit read)
        off = (-raw.ctypes.data % 16) // 4
        self.tab = raw[off:off + (4 << bbits)]
        assert self.tab.ctypes.data % 16 == 0
        self._raw = raw
        self.stash = np.zeros(STASH, np.uint32)
        self.n = np.zeros(1, np.uint32)
        self.hwm = np.zeros(1, np.uint32)

    def insert(self, slots):
        slots = np.ascontiguousarray(slots, np.uint32)
        out = np.empty(slots.size, np.int32)
        self.L.v16_insert_many(self.tab.ctypes.data, self.stash.ctypes.data, self.n.ctypes.data, self.bbits, slots.ctypes.data, slots.size, out.ctypes.data, self.hwm.ctypes.data)
        return out

    def entries(self):
        """(bucket, entry) of every occupied entry"""
        e = self.tab.view(np.uint16).reshape(-1, 8)
        b, i = np.nonzero(e & OCC)
        return b, e[b, i], e


def test_constants(v16):
    assert [v16.v16_consts(i) for i in range(6)] == [STASH, BBITS, 1 << 24, OCC, SECOND, TAG_MASK]


def test_hash_is_a_bijection_and_g_is_never_zero(v16):
    rng = np.random.default_rng(1)
    for bbits in (4, 7, 10):
        top = 1 << (14 + bbits)
        s = np.unique(np.concatenate([rng.integers(0, top, 20000, dtype=np.uint64), [0, 1, top - 1, top // 2]])).astype(np.uint32)
        h = np.array([v16.v16_hash(int(x), bbits) for x in s], np.uint32)
        assert h.max() < top and np.unique(h).size == s.size
        assert np.array_equal(np.array([v16.v16_unhash(int(x), bbits) for x in h], np.uint32), s)
        g = np.array([v16.v16_g(t, bbits) for t in range(1 << 14)], np.uint32)
        assert g.min() >= 1 and g.max() < (1 << bbits)


def test_random_slots_against_a_set(v16):
    rng = np.random.default_rng(2)
    t = Table(v16)
    # 5 000 distinct slots up to 2^24 - 1 (the ends included), every third one offered again in between
    base = np.unique(np.concatenate([rng.integers(0, 1 << 24, 5000, dtype=np.uint64), [0, (1 << 24) - 1]])).astype(np.uint32)
    rng.shuffle(base)
    seq = np.concatenate([base[:2500], base[:2500:3], base[2500:], base[::3]])
    got = t.insert(seq)
    seen = set(); want = []
    for s in seq.tolist():
        want.append(SEEN if s in seen else NEW); seen.add(s)
    assert np.array_equal(got, np.array(want, np.int32))
    # every member answers "seen", and strangers are inserted (never mistaken for a member)
    assert np.all(t.insert(base) == SEEN)
    strangers = np.setdiff1d(rng.integers(0, 1 << 24, 400, dtype=np.uint64).astype(np.uint32), base)
    assert np.all(t.insert(strangers) == NEW) and np.all(t.insert(strangers) == SEEN)


def _one_bucket_pair(v16, bbits, count):
    """`count` slots that all live in one bucket pair (b1, b2), by inverting the hash: tags with one g, first bucket b1 or b2 alternately"""
    g = np.array([v16.v16_g(t, bbits) for t in range(1 << 14)], np.uint32)
    g0 = int(np.bincount(g).argmax())
    tags = np.nonzero(g == g0)[0]
    assert tags.size * 2 >= count
    b1 = 5 % (1 << bbits); b2 = b1 ^ g0
    slots = []
    for i in range(count):
        b = b1 if i % 2 == 0 else b2
        slots.append(v16.v16_unhash((b << 14) | int(tags[i // 2]), bbits))
    assert len(set(slots)) == count
    return np.array(slots, np.uint32), b1, b2


@pytest.mark.parametrize("bbits", [10, 4])
def test_one_bucket_pair_fills_then_the_stash_then_overflows(v16, bbits):
    slots, b1, b2 = _one_bucket_pair(v16, bbits, 16 + STASH + 3)
    t = Table(v16, bbits)
    assert np.all(t.insert(slots[:16]) == NEW) and t.n[0] == 0          # two buckets of 8
    b, e, grid = t.entries()
    assert sorted(set(b.tolist())) == sorted({b1, b2}) and np.all(grid[b1] & OCC) and np.all(grid[b2] & OCC)
    assert np.all(t.insert(slots[16:16 + STASH]) == NEW) and t.n[0] == STASH   # ... then the stash
    assert np.array_equal(np.sort(t.stash), np.sort(slots[16:16 + STASH]))
    assert np.all(t.insert(slots[16 + STASH:]) == FULL) and t.n[0] == STASH    # ... then the overflow is reported, nothing is dropped silently
    assert np.all(t.insert(slots[:16 + STASH]) == SEEN)                        # every member is still a member
    assert np.all(t.insert(slots[16 + STASH:]) == FULL)                        # and a slot that found no room was not recorded
    # a slot elsewhere is not disturbed
    other = v16.v16_unhash(((b1 ^ 1) << 14) | 7, bbits)
    assert t.insert([other])[0] == NEW and t.insert([other])[0] == SEEN


def test_decoding_is_the_identity_over_a_full_table(v16):
    rng = np.random.default_rng(3)
    for bbits, top in ((10, 1 << 24), (5, 1 << 19)):
        t = Table(v16, bbits)
        members = set()
        # offer slots until the stash is full too: the table is then as full as two choices get it
        while True:
            s = rng.integers(0, top, 4096, dtype=np.uint64).astype(np.uint32)
            r = t.insert(s)
            members.update(s[r != FULL].tolist())
            if np.any(r == FULL):
                break
        b, e, grid = t.entries()
        assert b.size > 0.8 * (8 << bbits)
        dec = [v16.v16_decode(int(bb), int(ee), bbits) for bb, ee in zip(b.tolist(), e.tolist())]
        assert len(set(dec)) == len(dec)
        assert set(dec) | set(t.stash[:t.n[0]].tolist()) == members and not (set(dec) & set(t.stash[:t.n[0]].tolist()))
        # occupied entries are a prefix of their bucket
        occ = (grid & OCC) != 0
        assert np.all(occ[:, :-1] >= occ[:, 1:])
        # an entry sits in the first or the second bucket of its slot, as its bit says
        for bb, ee, s in zip(b.tolist(), e.tolist(), dec):
            h = v16.v16_hash(s, bbits)
            b1 = h >> 14
            assert (ee & TAG_MASK) == (h & TAG_MASK) and bb == (b1 ^ v16.v16_g(h & TAG_MASK, bbits) if ee & SECOND else b1)


def test_fill_to_the_capacity_rule(v16):
    """6 080 random slots of a 10 M index (the most the walk's capacity rule lets in: vis_count + 64 <= 6 144): the stash is enough"""
    rng = np.random.default_rng(4)
    worst = 0
    for trial in range(40):
        t = Table(v16)
        slots = rng.choice(10_000_000, 6080, replace=False).astype(np.uint32)
        r = t.insert(slots)
        assert np.all(r == NEW), trial
        assert t.hwm[0] <= STASH
        worst = max(worst, int(t.hwm[0]))
        assert np.all(t.insert(slots) == SEEN)
    print("stash high-water mark over 40 fills of 6080:", worst)
