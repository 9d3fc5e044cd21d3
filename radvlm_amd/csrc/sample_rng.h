// The counter-based uniform of seeded sampling and of speculative sampling (sample.hip, spec.hip): one definition for the device and
// for the host functions rv_sample_uniform24 / rv_sample_uniform24_tagged.
#pragma once
#include <stdint.h>

__host__ __device__ inline uint64_t sm_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the top 24 bits of portable_rng._stream(seed, tag, t + 1)[t]; tag 0 is the plain sampler's stream
__host__ __device__ inline uint32_t sm_uniform24(uint64_t seed, uint64_t tag, int32_t t) {
    const uint64_t base = sm_splitmix64(seed * 1000003ull + tag);
    return (uint32_t)(sm_splitmix64((uint64_t)(int64_t)t * 0xD1342543DE82EF95ull + base) >> 40);
}
