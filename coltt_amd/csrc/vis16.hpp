// vis16.hpp — an EXACT visited set in 16 bits per entry (hnsw_walk2.hpp: VIS_LDS16; the row-filter walk's LDS table at half the bytes of hnsw_dev.hpp: vis_insert).
// Plain C++ on purpose (no HIP header): tests/test_vis16_host.py compiles this file with g++ and drives the very code the kernel runs.
//
// A slot that already knows which bucket it sits in does not need 32 bits to say which of fewer than 2^24 graph slots it holds.
//   table   2^B buckets (B = 10 in the library: VIS16_BUCKET_BITS) of 8 entries of 16 bits: one bucket = 16 bytes = one ds_read_b128
//   hash    h = (slot * VIS16_MUL) & (2^(14+B) - 1): VIS16_MUL is odd, so h is a BIJECTION on the slots below 2^(14+B) (2^24 at B = 10)
//   place   first bucket b1 = h >> 14, tag = h & 0x3fff, second bucket b2 = b1 ^ g(tag) with g a function of the tag alone, never 0
//   entry   bit 15 occupied | bit 14 "this is the slot's SECOND bucket" | the tag.  An empty entry is 0.
// Given the bucket it lies in, an entry names exactly one slot: (bucket, bit 14, tag) -> b1 = bucket or bucket ^ g(tag) -> h -> slot (vis16_decode).  Two
// different slots never look alike in the same bucket: equal (bit 14, tag) in one bucket gives equal b1, hence equal h.  Membership is therefore exact —
// no fingerprints, no verification read.
// Entries are only ever added, each into the FIRST empty entry of its bucket, so the occupied entries of a bucket are a prefix: the load of a bucket is
// the number of its occupied bits and the first empty entry sits at that index.
// Test-and-set (vis16_test_and_set): read both buckets (independent reads), compare the 16 halfwords against the slot's two encodings; if absent, claim the
// first empty entry of the less loaded bucket with a 32-bit compare-and-swap on the dword that holds it, re-reading that bucket when the swap loses
// (another lane took the entry, or changed the other half of the dword).  No two lanes of a chunk insert the same slot (a row lists a neighbour once):
// the argument vis_insert rests on.  Both buckets full: the caller keeps the slot, as 32 bits, in a stash of VIS16_STASH words that is searched only while
// it is not empty; a full stash is the table's overflow (the walk's err 8).
// Two choices among 8-entry buckets: 100 trials each of random slots of a 10 M index in 1024 buckets never left a bucket pair full at 4 100 and 5 000
// entries, and in 3 % of the trials by ONE entry at 6 080 (the capacity rule's limit).  A 5-bit displacement field on linear probing overflows in 44 % of
// the trials at 5 000.
#pragma once
#include <cstdint>
#include "row_filter.hpp"   // COLTT_RF_HD

namespace coltt {

constexpr uint32_t VIS16_MUL = 0x3779B1u;        // odd (0x9E3779B1 mod 2^24)
constexpr uint32_t vis16_inverse(uint32_t a) { uint32_t x = a; for (int i = 0; i < 5; i++) x *= 2u - a * x; return x; }   // a x = 1 mod 2^32, hence mod every 2^k
constexpr uint32_t VIS16_MUL_INV = vis16_inverse(VIS16_MUL);
static_assert(VIS16_MUL * VIS16_MUL_INV == 1u, "the hash must be invertible");
constexpr uint32_t VIS16_TAG_BITS = 14, VIS16_TAG_MASK = 0x3fffu, VIS16_OCC = 0x8000u, VIS16_SECOND = 0x4000u;
constexpr uint32_t VIS16_BUCKET_BITS = 10;       // the library's table: 1024 buckets, 8192 entries, 16 KiB
constexpr uint32_t VIS16_MAX_SLOTS = 1u << (VIS16_TAG_BITS + VIS16_BUCKET_BITS);   // slots at or above this are not representable
constexpr uint32_t VIS16_STASH = 16;             // words
enum { VIS16_SEEN = 0, VIS16_NEW = 1, VIS16_FULL = 2 };

COLTT_RF_HD inline uint32_t vis16_table_words(uint32_t bbits) { return 4u << bbits; }
COLTT_RF_HD inline uint32_t vis16_hash(uint32_t slot, uint32_t bbits) { return (slot * VIS16_MUL) & ((1u << (VIS16_TAG_BITS + bbits)) - 1u); }
COLTT_RF_HD inline uint32_t vis16_unhash(uint32_t h, uint32_t bbits) { return (h * VIS16_MUL_INV) & ((1u << (VIS16_TAG_BITS + bbits)) - 1u); }
// the offset of the second bucket: a function of the tag alone, in [1, 2^B)
COLTT_RF_HD inline uint32_t vis16_g(uint32_t tag, uint32_t bbits) {
  const uint32_t g = ((tag * 0x9E37u) >> 6) & ((1u << bbits) - 1u);
  return g ? g : 1u;
}
// the slot an occupied entry of `bucket` stands for
COLTT_RF_HD inline uint32_t vis16_decode(uint32_t bucket, uint32_t entry, uint32_t bbits) {
  const uint32_t tag = entry & VIS16_TAG_MASK;
  const uint32_t b1 = (entry & VIS16_SECOND) ? bucket ^ vis16_g(tag, bbits) : bucket;
  return vis16_unhash((b1 << VIS16_TAG_BITS) | tag, bbits);
}

struct alignas(16) Vis16Bucket { uint32_t w0, w1, w2, w3; };
COLTT_RF_HD inline Vis16Bucket vis16_read(const uint32_t* tab, uint32_t b) { return *reinterpret_cast<const Vis16Bucket*>(tab + (size_t)b * 4); }
// the same bucket read again after a lost swap: the compiler must not serve it from the first read
COLTT_RF_HD inline Vis16Bucket vis16_reread(const uint32_t* tab, uint32_t b) {
  const volatile uint32_t* p = tab + (size_t)b * 4;
  Vis16Bucket r; r.w0 = p[0]; r.w1 = p[1]; r.w2 = p[2]; r.w3 = p[3];
  return r;
}
// is some halfword of x zero (exact as an existence test: a borrow only ever leaves a zero halfword)
COLTT_RF_HD inline uint32_t vis16_zero_half(uint32_t x) { return (x - 0x00010001u) & ~x & 0x80008000u; }
COLTT_RF_HD inline bool vis16_has(const Vis16Bucket& k, uint32_t enc) {
  const uint32_t p = enc * 0x00010001u;
  return (vis16_zero_half(k.w0 ^ p) | vis16_zero_half(k.w1 ^ p) | vis16_zero_half(k.w2 ^ p) | vis16_zero_half(k.w3 ^ p)) != 0u;
}
// occupied entries of a bucket (a prefix, see above): also the index of its first empty entry
COLTT_RF_HD inline uint32_t vis16_load(const Vis16Bucket& k) {
  return (uint32_t)(__builtin_popcount(k.w0 & 0x80008000u) + __builtin_popcount(k.w1 & 0x80008000u) + __builtin_popcount(k.w2 & 0x80008000u) + __builtin_popcount(k.w3 & 0x80008000u));
}
COLTT_RF_HD inline uint32_t vis16_word(const Vis16Bucket& k, uint32_t d) { return d == 0u ? k.w0 : (d == 1u ? k.w1 : (d == 2u ? k.w2 : k.w3)); }
// compare-and-swap on one dword of the table; returns what was there (the host's is the sequential one: the test drives one insertion at a time)
COLTT_RF_HD inline uint32_t vis16_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, v);
#else
  const uint32_t old = *p;
  if (old == expect) *p = v;
  return old;
#endif
}

// test-and-set on the table alone: VIS16_SEEN (a member), VIS16_NEW (inserted) or VIS16_FULL (absent, and both of its buckets are full: the caller's stash)
COLTT_RF_HD inline int vis16_test_and_set(uint32_t* tab, uint32_t bbits, uint32_t slot) {
  const uint32_t h = vis16_hash(slot, bbits), tag = h & VIS16_TAG_MASK;
  const uint32_t b1 = h >> VIS16_TAG_BITS, b2 = b1 ^ vis16_g(tag, bbits);
  const uint32_t e1 = VIS16_OCC | tag, e2 = VIS16_OCC | VIS16_SECOND | tag;
  Vis16Bucket A = vis16_read(tab, b1), B = vis16_read(tab, b2);
  if (vis16_has(A, e1) || vis16_has(B, e2)) return VIS16_SEEN;
  for (int tries = 0; tries < 64; tries++) {   // every lost swap is another lane's entry: at most 16 per bucket pair
    const uint32_t la = vis16_load(A), lb = vis16_load(B);
    if (la >= 8u && lb >= 8u) return VIS16_FULL;
    const bool second = lb < la;   // the less loaded bucket; the first one on a tie
    const uint32_t b = second ? b2 : b1, l = second ? lb : la, enc = second ? e2 : e1;
    const uint32_t d = l >> 1;
    const uint32_t cur = second ? vis16_word(B, d) : vis16_word(A, d);
    if (vis16_cas(tab + (size_t)b * 4 + d, cur, cur | (enc << ((l & 1u) * 16u))) == cur) return VIS16_NEW;
    if (second) B = vis16_reread(tab, b2); else A = vis16_reread(tab, b1);
  }
  return VIS16_FULL;
}

// the stash: the slots whose two buckets were full, as 32-bit words stash[0, n)
COLTT_RF_HD inline bool vis16_stash_has(const uint32_t* stash, uint32_t n, uint32_t slot) {
  bool f = false;
  for (uint32_t i = 0; i < n; i++) f = f || stash[i] == slot;
  return f;
}
// One insertion at a time through table and stash — the order of search_level2's chunk step (stash first while it is not empty, then the table, then the
// stash's tail).  VIS16_FULL here means the stash is full as well: the overflow.
COLTT_RF_HD inline int vis16_insert(uint32_t* tab, uint32_t* stash, uint32_t& n, uint32_t bbits, uint32_t slot) {
  if (n && vis16_stash_has(stash, n, slot)) return VIS16_SEEN;
  const int r = vis16_test_and_set(tab, bbits, slot);
  if (r != VIS16_FULL) return r;
  if (n >= VIS16_STASH) return VIS16_FULL;
  stash[n++] = slot;
  return VIS16_NEW;
}

}  // namespace coltt
