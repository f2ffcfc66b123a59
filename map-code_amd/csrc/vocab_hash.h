// The open-addressing tables of the vocabulary kernels (vocab.hip: the fit; vocab_apply.hip: a saved vocabulary):
// the empty marker and the hash of a raw 64-bit value.  Slot = vocab_hash(key) & (capacity - 1), linear probing.
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

}  // namespace mapx
