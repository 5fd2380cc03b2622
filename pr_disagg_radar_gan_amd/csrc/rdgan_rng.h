// Counter-based RNG for dropout masks and the RandomWeightedAverage alpha.
// Mirror of oracle/rng.py (same constants, same bit-exact definition): the reference draws
// these from TensorFlow's unseeded global RNG (gan_train_cwgangp_pixelnorm.py:223,289-301),
// so no bit pattern is pinned by the reference; both sides of the parity tests use this one.
#pragma once
#include <stdint.h>

#define RD_STREAM_D1 1u
#define RD_STREAM_ALPHA 5u
#define RD_STREAM_RAINFARM 6u       // phases of the RainFARM generation (rdgan_rainfarm.hip.h)
#define RD_STREAM_BOOTSTRAP 7u      // resample indices of the bootstrapped means (rdgan_crps.hip.h)
#define RD_STREAM_VERIFY 8u         // tie-breaking ranks of the verification (rdgan_verify.hip.h)
#define RD_STREAM_ANALOG 9u         // picks among the nearest library days (rdgan_analog.hip.h)
#define RD_STREAM_CASCADE 10u       // types, weight bins and weights of the random cascade (rdgan_cascade.hip.h)
#define RD_DROP_THRESHOLD 64u         // 0.25 * 2^8: a byte of the hash word decides one element

#if defined(__HIPCC__)
#define RD_HD __host__ __device__
#else
#define RD_HD
#endif

RD_HD static inline uint32_t rd_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
RD_HD static inline uint32_t rd_make_key(uint64_t seed, uint32_t stream) {
  uint32_t lo = (uint32_t)(seed & 0xFFFFFFFFull), hi = (uint32_t)(seed >> 32);
  return rd_mix32(lo ^ rd_mix32(hi ^ 0x9E3779B9u)) + stream * 0x85EBCA6Bu;
}
RD_HD static inline uint32_t rd_bits(uint32_t key, uint32_t idx) { return rd_mix32(rd_mix32(idx) ^ key); }
RD_HD static inline float rd_uniform(uint32_t key, uint32_t idx) { return (float)(rd_bits(key, idx) >> 8) * (1.0f / 16777216.0f); }
// inverted dropout, rate 0.25: 0 or 1/0.75.  ONE hash word decides the four elements idx & ~3 ... idx | 3 (a byte each: keep iff
// byte >= 64, P = 192/256): the epilogues handle four consecutive channels per lane, so the two rd_mix32 -- four quarter-rate
// v_mul_lo_u32 -- are paid once per four elements instead of once per element (round 3; the 24-bit-per-element form cost the
// first critic layer's forward 0.18 ms of pure VALU time at 6144 samples).
RD_HD static inline uint32_t rd_drop_word(uint32_t key, uint32_t idx) { return rd_bits(key, idx >> 2); }
RD_HD static inline int rd_drop_keep(uint32_t word, uint32_t e) { return ((word >> (8u * (e & 3u))) & 0xFFu) >= RD_DROP_THRESHOLD; }
RD_HD static inline float rd_drop_scale(uint32_t key, uint32_t idx) {
  return rd_drop_keep(rd_drop_word(key, idx), idx) ? (1.0f / 0.75f) : 0.0f;
}
// Per-member keys (the RainFARM phases): member m of a seeded ensemble draws u(m, e) = rd_uniform(rd_member_key(base, m), e) with
// base = rd_make_key(seed, RD_STREAM_RAINFARM) and e the element's index inside the member ((t nd + i) nd + j for a (24, nd, nd)
// day).  A value depends on (seed, m, e) only -- not on how members are split into launches or calls -- and m is 64-bit, so
// ensembles far beyond 2^32 elements in all never reuse a counter.
//     rd_member_key(base, m) = mix(base ^ mix(lo32(m) ^ mix(hi32(m) ^ 0x9E3779B9)))
RD_HD static inline uint32_t rd_member_key(uint32_t base, uint64_t member) {
  return rd_mix32(base ^ rd_mix32((uint32_t)member ^ rd_mix32((uint32_t)(member >> 32) ^ 0x9E3779B9u)));
}
