// chain_draw.hpp — the sampled chains' draw, written once for the host
// (aicp_hip_chain_uniform, pm_config.cpp) and the device (kernels_chain.hip).
//
// libpointmatcher's RandomSampling and MaxDensity filters draw std::rand(), a sequential stream
// the reference reseeds from the clock; here the draw of a point is a pure function of (seed,
// slot, i): slot = 4 * side + the filter's position in its list, i = the point's index in the
// cloud as that filter receives it. No state, no dependence on the launch shape.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define AICP_CHAIN_HD __host__ __device__
#else
#define AICP_CHAIN_HD
#endif

namespace aicp {

// splitmix64's finaliser
AICP_CHAIN_HD inline uint64_t chain_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// k * 2^-24, k the top 24 bits of two finaliser rounds over seed, slot and i: exact in float, [0, 1)
AICP_CHAIN_HD inline float chain_uniform(uint64_t seed, uint32_t slot, uint32_t i) {
  const uint64_t a = chain_mix64(seed + 0x9e3779b97f4a7c15ull * ((uint64_t)slot + 1ull));
  const uint64_t b = chain_mix64(a + 0x9e3779b97f4a7c15ull * ((uint64_t)i + 1ull));
  return (float)(uint32_t)(b >> 40) * 5.9604644775390625e-08f;  // 2^-24
}

}  // namespace aicp
