// gsr_rng.h -- the counter-based generator of the library: Philox-4x32-10 (Salmon et al., SC'11) + Box-Muller. A value is a
// pure function of (key, counter): no state, no launch geometry. Users and their counters (SEMANTICS.md "Seeded noise"):
//   densify.hip          (row, copy, 0, 0)         three normals per child
//   K1 / K8 scale noise  (i, 0, stream, 1)         normals 0..2 of the block
//   K1 / K8 SH noise     (i, j, stream, 2)         element e of the [K,3] row = normal e % 4 of block j = e / 4
// Consumers are built with -ffp-contract=off: every site that evaluates a block gets the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }   // (0, 1)

// One Philox block -> four standard normals (two Box-Muller pairs). |n| <= sqrt(-2 ln 2^-25) = 5.89.
__device__ __forceinline__ void normals4(const uint32_t r[4], float n[4]) {
  const float ra = sqrtf(-2.0f * logf(u01(r[0]))), ta = 6.283185307179586f * u01(r[1]);
  const float rb = sqrtf(-2.0f * logf(u01(r[2]))), tb = 6.283185307179586f * u01(r[3]);
  n[0] = ra * cosf(ta);
  n[1] = ra * sinf(ta);
  n[2] = rb * cosf(tb);
  n[3] = rb * sinf(tb);
}

constexpr uint32_t kNoiseTagScale = 1u, kNoiseTagSh = 2u;
// the four normals of block (i, j) of (seed, stream, tag)
__device__ __forceinline__ void noise_block(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t tag, uint32_t i,
                                            uint32_t j, float n[4]) {
  uint32_t r[4];
  philox4x32_10(i, j, stream, tag, seed_lo, seed_hi, r);
  normals4(r, n);
}

}  // namespace
