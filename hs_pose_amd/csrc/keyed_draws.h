// keyed_draws.h -- the keyed counter-based generator every device draw is made from (include/hsp.h states the construction in
// the hsp_sample_ids section; the sections "keyed draws of a step" give each stream's words): uint32 arithmetic only.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace hsp {

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t absorb(uint32_t h, uint32_t w) { return fmix32((h ^ w) + 0x9e3779b9u); }

// kj of instance j under the key {seed, call}
__device__ __forceinline__ uint32_t instance_key(const unsigned long long* __restrict__ key, int j) {
    const unsigned long long seed = key[0], call = key[1];
    uint32_t kj = absorb(0u, (uint32_t)seed);
    kj = absorb(kj, (uint32_t)(seed >> 32));
    kj = absorb(kj, (uint32_t)call);
    kj = absorb(kj, (uint32_t)(call >> 32));
    return absorb(kj, (uint32_t)j);
}

// P(s) for s < c, c >= 1: the cycle-walked 4-round Feistel permutation of [0, c) with round keys absorb(k, 0..3)
__device__ __forceinline__ uint32_t feistel_permute(uint32_t s, uint32_t c, uint32_t k) {
    const uint32_t k0 = absorb(k, 0u), k1 = absorb(k, 1u), k2 = absorb(k, 2u), k3 = absorb(k, 3u);
    const int bits = c <= 1u ? 0 : 32 - __clz((int)(c - 1u));
    const int half = max(1, (bits + 1) / 2);
    const uint32_t mask = (1u << half) - 1u;
    uint32_t x = s;
    do {
        uint32_t L = x >> half, R = x & mask, t;
        t = L ^ (fmix32(R ^ k0) & mask); L = R; R = t;
        t = L ^ (fmix32(R ^ k1) & mask); L = R; R = t;
        t = L ^ (fmix32(R ^ k2) & mask); L = R; R = t;
        t = L ^ (fmix32(R ^ k3) & mask); L = R; R = t;
        x = (L << half) | R;
    } while (x >= c);
    return x;
}

// the two exact conversions of a 32-bit word to a uniform in [0, 1)
__device__ __forceinline__ float word_to_f32(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }      // 2^-24
__device__ __forceinline__ double word_to_f64(uint32_t w) { return (double)w * 2.3283064365386962890625e-10; }       // 2^-32

}  // namespace hsp
