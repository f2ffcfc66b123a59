// The open-addressing tables of the vocabulary kernels (vocab.hip: the fit; vocab_apply.hip: a saved vocabulary):
// the empty marker, the hash of a raw 64-bit value, the claim of a key's slot and the read-only lookup.
// Slot = vocab_hash(key) & (capacity - 1), linear probing.
#pragma once
#include <stdint.h>

#include "common.h"

namespace mapx {

constexpr int64_t kVocabEmpty = INT64_MIN;       // key value no column may hold

__device__ inline uint64_t vocab_hash(uint64_t x) {   // splitmix64 finaliser: raw ids are hashes or small ints
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

enum VocabClaim { kVocabClaimed, kVocabHeld, kVocabFull };

// Finds or claims the slot of key k (not kVocabEmpty) among the `cap` (a power of two) slots of tkey: a volatile read,
// atomicCAS on the key word where the slot looks empty.  *slot = the key's slot; kVocabClaimed: this call put the key
// there, kVocabHeld: the slot held it already, kVocabFull: `cap` probes met other keys only (*slot is not the key's).
__device__ inline VocabClaim vocab_claim(int64_t* __restrict__ tkey, int64_t cap, int64_t k, uint64_t* slot) {
  const uint64_t mask = (uint64_t)cap - 1;
  uint64_t s = vocab_hash((uint64_t)k) & mask;
  for (int64_t probes = 0; probes < cap; ++probes) {
    unsigned long long* cell = reinterpret_cast<unsigned long long*>(tkey + s);
    long long seen = (long long)*reinterpret_cast<volatile unsigned long long*>(cell);
    if (seen == kVocabEmpty)
      seen = (long long)atomicCAS(cell, (unsigned long long)kVocabEmpty, (unsigned long long)k);
    if (seen == kVocabEmpty || seen == k) {
      *slot = s;
      return seen == k ? kVocabHeld : kVocabClaimed;
    }
    s = (s + 1) & mask;
  }
  return kVocabFull;
}

// rank of `v` among field f's keys, or nf (<oov>).  Plain loads; the walk ends at an empty slot and, whatever the
// table holds, after `cap` slots.
__device__ inline int32_t vocab_apply_probe(const int64_t* __restrict__ tkey, const int32_t* __restrict__ trank,
                                            int64_t t0, int64_t cap, int64_t nf, int64_t v) {
  const uint64_t mask = (uint64_t)cap - 1;
  uint64_t s = vocab_hash((uint64_t)v) & mask;
  for (int64_t probes = 0; probes < cap; ++probes) {
    const int64_t k = tkey[t0 + s];
    if (k == v) return trank[t0 + s];
    if (k == kVocabEmpty) break;
    s = (s + 1) & mask;
  }
  return (int32_t)nf;
}

}  // namespace mapx
