// counter_rng.h -- the counter-based generator of the node2vec kernels (walk.hip, sgns.hip), of proximity.hip's random sets, of
// perm_null.h's seeded permutations (one tag per null) and of resample.hip's bootstrap draws and sign flips.
//
// Every random number is a pure function of (seed, stream tag, three 64-bit counters): no state is carried between draws, so
// walks and SGNS are bitwise reproducible run to run, independent of the launch shape, and replayable by a numpy statement of
// the same arithmetic (tests/node2vec_mirror.py).  The mixer is the SplitMix64 finaliser; a key is absorbed one word at a time:
//   h = seed;  for x in (tag, a, b, c):  h = mix64(h + x + 0x9E3779B97F4A7C15)
// uniform fp64 in [0, 1) = (h >> 11) * 2^-53, uniform fp32 in [0, 1) = (h >> 40) * 2^-24, uniform uint32 = h >> 32.
#pragma once
#include <stdint.h>

namespace gss {

enum RngTag : uint64_t {
  kRngWalk = 1,    // (walk, step, attempt)
  kRngPerm = 2,    // (iteration, node, 0): sort keys of the per-iteration start order (computed on the host)
  kRngWindow = 3,  // (epoch, token, 0)
  kRngKeep = 4,    // (epoch, token, 0)
  kRngNeg = 5,     // (epoch, center token, context token * 64 + k)
  kRngInit = 6,    // (node, component, 0)
  kRngProxFrom = 7,  // proximity random sets of the from-side (drug targets): (set, sample, member * 32 + attempt)
  kRngProxTo = 8,    // proximity random sets of the to-side (disease genes): (set, sample, member * 32 + attempt)
  kRngClassPerm = 9, // class coherence null: (sample, drug, 0): sort keys of the sample's permutation of the drug pool
  kRngBootDraw = 10, // bootstrap of the per-indication metrics: (replicate, place, 0): the upper 32 bits pick the place's value out of n
  kRngSignFlip = 11, // sign-flip null of a paired difference: (replicate, place, 0): the top bit negates the place's value
  kRngMantelPerm = 12, // Mantel null: (replicate, row, 0): sort keys of the replicate's relabelling of one matrix's rows and columns
  kRngEnrichPerm = 13, // enrichment null: (sample, place, 0): sort keys of the sample's permutation of the universe's places
};

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__host__ __device__ __forceinline__ uint64_t rng_key(uint64_t seed, uint64_t tag, uint64_t a, uint64_t b, uint64_t c) {
  const uint64_t k = 0x9E3779B97F4A7C15ull;
  uint64_t h = mix64(seed + tag + k);
  h = mix64(h + a + k);
  h = mix64(h + b + k);
  return mix64(h + c + k);
}

__host__ __device__ __forceinline__ double rng_unit_f64(uint64_t h) { return (double)(h >> 11) * 0x1.0p-53; }
__host__ __device__ __forceinline__ float rng_unit_f32(uint64_t h) { return (float)(h >> 40) * 0x1.0p-24f; }
__host__ __device__ __forceinline__ uint32_t rng_u32(uint64_t h) { return (uint32_t)(h >> 32); }

}  // namespace gss
