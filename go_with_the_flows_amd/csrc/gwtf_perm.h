// gwtf_perm.h -- the keyed bijection on [0, P) the stored-cloud sampler draws without replacement with (gwtf_clouds.hip; the rule is
// the header comment of GwtfStoredCloudArgs in include/gwtf.h).  A six-round Feistel network on the smallest even-width domain
// 2^(2h) >= P, walked along its cycle until it lands below P.  tests/cloud_store_ref.py restates it in numpy; the host export
// gwtf_perm_index evaluates this same function on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gwtf_perm {

constexpr int kRounds = 6;
constexpr int kWalkCap = 1024;                 // steps; a walk that long is a coding error, never a draw (each step ends w.p. > 1/4)
constexpr uint32_t kNoIndex = 0xffffffffu;

// murmur3's 32-bit finaliser
__host__ __device__ inline uint32_t fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// Half width h of the domain 2^(2h): b = max(1, ceil(log2 P)), h = (b + 1) / 2; 1 <= h <= 16 for 1 <= P < 2^31.
__host__ __device__ inline int half_bits(uint32_t P) {
  const int b = P > 2u ? 32 - __builtin_clz(P - 1u) : 1;
  return (b + 1) >> 1;
}

// The image of t in [0, P) under the permutation keyed by keys[0..5]; kNoIndex for t >= P, P outside [1, 2^31) or a walk past the cap.
__host__ __device__ inline uint32_t feistel_index(const uint32_t* keys, uint32_t t, uint32_t P) {
  if (P < 1u || P > 0x7fffffffu || t >= P) return kNoIndex;
  const int h = half_bits(P);
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = t;
  for (int step = 0; step < kWalkCap; ++step) {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (int i = 0; i < kRounds; ++i) {
      const uint32_t n = L ^ (fmix32(R ^ keys[i]) >> (32 - h));
      L = R; R = n;
    }
    x = (L << h) | R;
    if (x < P) return x;
  }
  return kNoIndex;
}

}  // namespace gwtf_perm
