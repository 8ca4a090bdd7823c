// gwtf_philox.h -- the counter-based generator the device samplers share (gwtf_clouds.hip, gwtf_route.hip): Philox4x32-10 and the
// Box-Muller pair.  tests/clouds_ref.py restates both in numpy and golden g22_clouds pins their bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gwtf_rng {

struct Philox4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Salmon et al., SC'11; Random123 reference constants)
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

// (w0, w1) -> two standard normals: u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f, u2 = (float)(wb >> 8) * 0x1p-24f;
  const float rad = sqrtf(-2.0f * logf(u1)), ang = 6.28318530717958647692f * u2;
  z0 = rad * cosf(ang);
  z1 = rad * sinf(ang);
}

}  // namespace gwtf_rng
