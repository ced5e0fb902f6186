// Counter-based dropout shared by both regimes of the Chinese text branch (bert_f32.hip, bert_f16.hip, bert_tower.hip): Philox4x32-10
// (Salmon et al., SC'11).  The keep decision of element `idx` of dropout site `site` is word (idx & 3) of
// Philox(key = seed, counter = (idx >> 2, site)): a pure function of (seed, site, idx), so the backward regenerates it and
// no mask is stored.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
struct Drop { unsigned k0, k1, site, thresh; float scale; };     // keep <=> word >= thresh;  scale = 1 / (1 - p)
inline bool drop_p_ok(float p) { return p >= 0.f && p < 1.f; }   // the probabilities every entry point takes (a NaN is refused)
inline Drop make_drop(float p, long seed, int site) {
  Drop d;
  d.k0 = (unsigned)((unsigned long)seed & 0xffffffffu); d.k1 = (unsigned)((unsigned long)seed >> 32);
  d.site = (unsigned)site;
  const double t = (double)p * 4294967296.0;
  d.thresh = t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
  d.scale = 1.0f / (1.0f - p);
  return d;
}
__device__ __forceinline__ void drop_words(const Drop& d, unsigned long quad, unsigned (&w)[4]) {
  philox4x32_10(d.k0, d.k1, (unsigned)(quad & 0xffffffffu), (unsigned)(quad >> 32), d.site, 0u, w);
}
__device__ __forceinline__ bool drop_keep(const Drop& d, unsigned long idx) {
  unsigned w[4];
  drop_words(d, idx >> 2, w);
  const unsigned s = (unsigned)(idx & 3);
  return (s == 0 ? w[0] : s == 1 ? w[1] : s == 2 ? w[2] : w[3]) >= d.thresh;
}

}  // namespace
