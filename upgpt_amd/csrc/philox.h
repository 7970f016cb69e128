// The device functions of the keyed noise (include/upk.h): Philox4x32-10 and the words -> normals transform, shared by
// rng.hip (the noise tables) and loss.hip (the draw inside upk_q_sample_keyed_f32).  Both files are compiled with
// -ffp-contract=off, so the same words give the same bits in either.
#pragma once
#include "common.h"

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += W0, k1 += W1;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// (w_a, w_b) -> (z_a, z_b): include/upk.h.  u1, u2 and 2 u2 are exact in fp32; the angle 2 pi u2 is never rounded
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& za, float& zb) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  za = r * c, zb = r * s;
}
