// The fp16 regime of the Chinese text branch (bert_f32.hip is the fp32 one): selected by the parameters' dtypes
// (module_cross.convert_bert_weights: every nn.Linear weight and bias fp16; the embedding tables and every LayerNorm
// parameter fp32), as convert_weights selects the fp16 CLIP towers.  Embedding + LayerNorm + site-0 dropout stay the fp32
// kernels of bert_f32.hip, followed by ONE cast; from there the residual stream and every saved activation are fp16.  GEMMs:
// hmmc_gemm_f16 (fp32 accumulation, bias / residual in the epilogue); LayerNorm and reductions: the fp16 kernels of
// norm_elem.hip with fp32 statistics.  New kernels here: key-masked MFMA attention with in-kernel dropout, erf-GELU, dropout
// and the pooler's tanh on fp16 tensors; hmmc_bert_f16_fwd / hmmc_bert_f16_bwd are the one sequence of bert_tower.hip with
// f32 = false.  No atomics, fixed summation order: bit-identical from run to run.
//
// ROUNDING POINTS (tests/bert16_ref.py restates exactly these; everything between two of them is fp32):
//   x0 = fp16(dropout_0(LN(word + pos + type)))                         one cast after the fp32 embedding kernels
//   every GEMM: C = fp16(acc + bias), with a residual C = fp16(resid + fp16(acc + bias))      (hmmc_gemm_f16's epilogues)
//   attention, forward:  S = Q K^T / 8 and the softmax P in fp32; Pd = fp16(P o keep / (1 - p)) (= fp16(P) without dropout)
//                        multiplies V; O = fp16(Pd V); lse = max + log(sum) fp32
//   attention, backward: P = exp(S - lse) fp32 again; dPd = dO V^T fp32; dP = dPd o keep / (1 - p) fp32;
//                        delta = rowsum(P o dP) fp32; dS = fp16(P o (dP - delta) / 8) multiplies K and Q;
//                        Pd = fp16(P o keep / (1 - p)) multiplies dO; dQ, dK, dV = fp16(their fp32 sums)
//   dropout sites 2 + 3i, 3 + 3i: y = fp16(x o keep / (1 - p) + resid); backward dx = fp16(dy o keep / (1 - p))
//   LayerNorm: fp32 statistics and arithmetic on fp16 rows, y and dx rounded once (norm_elem.hip)
//   erf-GELU: g = fp16(gelu(h)), dh = fp16(dg gelu'(h)), fp32 erf
//   pooler: z = fp16(x W^T + b) (the GEMM), y = fp16(tanh(z)); dz = fp16(dy (1 - y^2))
//   bias gradients: fp32 column sums of the fp16 gradient, rounded once; weight gradients: fp16(fp32 sums)
#include "attn_common.h"
#include "bert_regime.h"
#include "philox.h"
#include <algorithm>

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// ---------------------------------------------------------------- key-masked fp16 attention, head dim 64, L <= 64
// attention_f16.hip's design: one wave per (sequence, head), S^T = K Q^T so that a lane holds 4 consecutive keys of one
// query, no workgroup barrier.  What is new: the key mask is a 64-bit wave-uniform word (bit j: key j valid AND j < L); K
// and V rows whose bit is clear enter as ZEROS (whatever bits they hold - a NaN would otherwise reach a sum through 0 x NaN),
// their scores become -inf (forward) / their probabilities 0 (backward); dropout on the probabilities from philox.h with the
// element index ((n*H + h)*L + i)*64 + j, so a lane's 4 consecutive keys are the 4 words of one Philox call.
struct MAttnArgs {
  const half_t* qkv; const long* mask; half_t* out; float* lse;
  const half_t* dout; half_t* dqkv; float* dbias;
  int nseq, L, H;
  Drop dr;
};

template <int KT>
__device__ __forceinline__ void zero_dead_rows(u4v (&raw)[2 * KT], unsigned long vbits, int lane) {
  const u4v z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 2 * KT; ++i)
    if (!((vbits >> ((lane >> 3) + 8 * i)) & 1ul)) raw[i] = z;
}
__device__ __forceinline__ unsigned long key_bits(const long* mask, long n, int L, int lane) {
  return __ballot(lane < L && mask[n * L + (lane < L ? lane : 0)] != 0);
}

constexpr int MFWD_WPB = 4;
template <int KT, bool DROP>
__global__ __launch_bounds__(64 * MFWD_WPB, 2) void mattn16_fwd_kernel(MAttnArgs p) {
  constexpr int LP = 16 * KT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long pair = (long)blockIdx.x * MFWD_WPB + wid;
  if (pair >= (long)p.nseq * p.H) return;
  const int n = (int)(pair / p.H), h = (int)(pair % p.H);
  const int D = p.H * DH, L = p.L;
  const long ld = 3L * D;
  const half_t* q = p.qkv + (long)n * L * ld + h * DH;
  const half_t* k = q + D;
  const half_t* v = q + 2 * D;
  half_t* vtile = reinterpret_cast<half_t*>(smem) + wid * (LP * LDS_STRIDE + 16 * LDS_STRIDE);
  half_t* scr = vtile + LP * LDS_STRIDE;
  const int g = lane >> 4, c = lane & 15;
  const unsigned long vbits = key_bits(p.mask, n, L, lane);

  h8 kf[KT][2], qf[KT][2], vf[KT][2];
  {
    u4v rk[2 * KT], rq[2 * KT], rv[2 * KT];
    load_rows<KT>(k, ld, L, rk, lane);
    load_rows<KT>(q, ld, L, rq, lane);
    load_rows<KT>(v, ld, L, rv, lane);
    zero_dead_rows<KT>(rk, vbits, lane);
    zero_dead_rows<KT>(rv, vbits, lane);
    rows_to_frags<KT>(vtile, rk, kf, lane);
    rows_to_frags<KT>(vtile, rq, qf, lane);
    rows_to_frags<KT>(vtile, rv, vf, lane);      // V last: the tile then holds it for the transposed reads
  }
  h8 vT[4][KT / 2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int ks = 0; ks < KT / 2; ++ks) vT[dt][ks] = tr_frag(vtile, ks * 32, ks * 32 + 16, dt * 16, lane);

  half_t* o = p.out + (long)n * L * D + h * DH;
  const unsigned long row0 = ((unsigned long)n * p.H + h) * L;
#pragma unroll
  for (int qt = 0; qt < KT; ++qt) {
    const int qi = qt * 16 + c;
    f4 s[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      f4 z = {0.f, 0.f, 0.f, 0.f};
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][0], qf[qt][0], z, 0, 0, 0);
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][1], qf[qt][1], s[kt], 0, 0, 0);
    }
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * 16 + 4 * g + r;
        const float val = ((vbits >> key) & 1ul) ? s[kt][r] * 0.125f : -INFINITY;
        s[kt][r] = val;
        m = fmaxf(m, val);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(s[kt][r] - m);
        s[kt][r] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if (g == 0 && qi < L) p.lse[row0 + qi] = m + __logf(sum);
    h4 pt[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      unsigned w[4] = {0u, 0u, 0u, 0u};
      if constexpr (DROP) drop_words(p.dr, (row0 + (unsigned long)qi) * 16 + kt * 4 + g, w);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv = s[kt][r] * inv;
        if constexpr (DROP) pv = w[r] >= p.dr.thresh ? pv * p.dr.scale : 0.f;
        pt[kt][r] = (half_t)pv;
      }
    }
    f4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      acc[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KT / 2; ++ks)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vT[dt][ks], cat4(pt[2 * ks], pt[2 * ks + 1]), acc[dt], 0, 0, 0);
    }
    store_rows(o, D, acc, qt * 16, L, scr, lane);
  }
}

// Backward: attention_f16.hip's two phases.  Phase 1 (keys on the lane's rows) forms delta and dQ and, with dropout, leaves
// every query's 64 keep bits in LDS (two words per query), so phase 2 (queries on the lane's rows: dV, then dK) tests a bit
// instead of running Philox once per element.
constexpr int MBWD_WPB = 2;
template <int KT, bool DROP>
__global__ __launch_bounds__(64 * MBWD_WPB, 2) void mattn16_bwd_kernel(MAttnArgs p) {
  constexpr int LP = 16 * KT;
  constexpr int WAVE_LDS = LP * LDS_STRIDE * 2 + 16 * LDS_STRIDE * 2 + 2 * LP * 4 + LP * 8;   // tile, store scratch, lse, delta, keep bits
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long pair = (long)blockIdx.x * MBWD_WPB + wid;
  if (pair >= (long)p.nseq * p.H) return;
  const int n = (int)(pair / p.H), h = (int)(pair % p.H);
  const int D = p.H * DH, L = p.L;
  const long ld = 3L * D;
  const half_t* q = p.qkv + (long)n * L * ld + h * DH;
  const half_t* k = q + D;
  const half_t* v = q + 2 * D;
  const half_t* dO = p.dout + (long)n * L * D + h * DH;
  half_t* dq = p.dqkv + (long)n * L * ld + h * DH;
  half_t* dk = dq + D;
  half_t* dv = dq + 2 * D;
  half_t* xt = reinterpret_cast<half_t*>(smem + wid * WAVE_LDS);
  half_t* scr = xt + LP * LDS_STRIDE;
  float* lse_s = reinterpret_cast<float*>(smem + wid * WAVE_LDS + LP * LDS_STRIDE * 2 + 16 * LDS_STRIDE * 2);
  float* del_s = lse_s + LP;
  unsigned* keep_s = reinterpret_cast<unsigned*>(del_s + LP);      // [LP][2]: keys 0..31 | 32..63 of query i
  const int g = lane >> 4, c = lane & 15;
  const unsigned long row0 = ((unsigned long)n * p.H + h) * L;
  const float* lse_g = p.lse + row0;
  const unsigned long vbits = key_bits(p.mask, n, L, lane);

  h8 qf[KT][2], kf[KT][2], vf[KT][2], df[KT][2];
  {
    u4v rq[2 * KT], rk[2 * KT], rv[2 * KT], rd[2 * KT];
    load_rows<KT>(q, ld, L, rq, lane);
    load_rows<KT>(v, ld, L, rv, lane);
    load_rows<KT>(dO, D, L, rd, lane);
    load_rows<KT>(k, ld, L, rk, lane);
    zero_dead_rows<KT>(rv, vbits, lane);
    zero_dead_rows<KT>(rk, vbits, lane);
    rows_to_frags<KT>(xt, rq, qf, lane);
    rows_to_frags<KT>(xt, rv, vf, lane);
    rows_to_frags<KT>(xt, rd, df, lane);
    rows_to_frags<KT>(xt, rk, kf, lane);         // K last: phase 1 reads K^T from the tile
  }
  float lse_c[KT];                               // lse of query qt*16 + c; +inf past L: its probabilities vanish
#pragma unroll
  for (int t = 0; t < KT; ++t) lse_c[t] = (t * 16 + c < L) ? lse_g[t * 16 + c] : INFINITY;
  if (g == 0) {
#pragma unroll
    for (int t = 0; t < KT; ++t) lse_s[t * 16 + c] = LOG2E * lse_c[t];
  }

  float* dbias = p.dbias ? p.dbias + (long)n * 3 * D + h * DH : nullptr;   // + type * D
  f4 csum[4];
  // ---- phase 1: keys on the lane's rows -> delta, the keep bits and dQ (the tile holds K)
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) csum[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qt = 0; qt < KT; ++qt) {
    const int qi = qt * 16 + c;
    f4 s[KT], dp[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      f4 z = {0.f, 0.f, 0.f, 0.f};
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][0], qf[qt][0], z, 0, 0, 0);
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][1], qf[qt][1], s[kt], 0, 0, 0);
      dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[kt][0], df[qt][0], z, 0, 0, 0);
      dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[kt][1], df[qt][1], dp[kt], 0, 0, 0);
    }
    float dl = 0.f;
    unsigned klo = 0u, khi = 0u;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      unsigned w[4] = {0u, 0u, 0u, 0u};
      if constexpr (DROP) drop_words(p.dr, (row0 + (unsigned long)qi) * 16 + kt * 4 + g, w);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * 16 + 4 * g + r;
        float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][r], 0.125f * LOG2E, -LOG2E * lse_c[qt]));
        pv = ((vbits >> key) & 1ul) ? pv : 0.f;
        s[kt][r] = pv;
        if constexpr (DROP) {
          const bool keep = w[r] >= p.dr.thresh;
          dp[kt][r] = keep ? dp[kt][r] * p.dr.scale : 0.f;
          if (keep) { if (kt < 2) klo |= 1u << (key & 31); else khi |= 1u << (key & 31); }
        }
        dl += pv * dp[kt][r];
      }
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    if (g == 0) del_s[qi] = dl;
    if constexpr (DROP) {
      klo |= __shfl_xor(klo, 16, 64); klo |= __shfl_xor(klo, 32, 64);
      khi |= __shfl_xor(khi, 16, 64); khi |= __shfl_xor(khi, 32, 64);
      if (g == 0) { keep_s[2 * qi] = klo; keep_s[2 * qi + 1] = khi; }
    }
    h4 ds16[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) ds16[kt][r] = (half_t)(s[kt][r] * (dp[kt][r] - dl) * 0.125f);
    f4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      acc[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KT / 2; ++ks)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tr_frag(xt, ks * 32, ks * 32 + 16, dt * 16, lane),
                                                         cat4(ds16[2 * ks], ds16[2 * ks + 1]), acc[dt], 0, 0, 0);
    }
    store_rows(dq, ld, acc, qt * 16, L, scr, lane);
    if (dbias) add_rounded(csum, acc);           // rows past L are exact zeros (their dS is)
  }
  if (dbias) store_colsum(dbias, csum, lane);

  // ---- phase 2: queries on the lane's rows.  pass 0: dV^T = dO^T Pd; pass 1: dK^T = Q^T dS; one key tile at a time
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0) frags_to_tile<KT>(xt, df, lane); else frags_to_tile<KT>(xt, qf, lane);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) csum[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int key = kt * 16 + c;
      const bool kvalid = (vbits >> key) & 1ul;
      h4 b16[KT];                                // Pd (pass 0) or dS (pass 1) of key tile kt, [qt]
#pragma unroll
      for (int qt = 0; qt < KT; ++qt) {
        f4 z = {0.f, 0.f, 0.f, 0.f};
        f4 sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[qt][0], kf[kt][0], z, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[qt][1], kf[kt][1], sc, 0, 0, 0);
        f4 dp = z;
        if (pass == 1) {
          dp = __builtin_amdgcn_mfma_f32_16x16x32_f16(df[qt][0], vf[kt][0], z, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_f16(df[qt][1], vf[kt][1], dp, 0, 0, 0);
        }
        const f4 lr = *reinterpret_cast<const f4*>(lse_s + qt * 16 + 4 * g);
        const f4 dr = *reinterpret_cast<const f4*>(del_s + qt * 16 + 4 * g);
        u4v kb0 = {0u, 0u, 0u, 0u}, kb1 = {0u, 0u, 0u, 0u};      // (lo, hi) of queries 4g, 4g+1 | 4g+2, 4g+3
        if constexpr (DROP) {
          kb0 = *reinterpret_cast<const u4v*>(keep_s + 2 * (qt * 16 + 4 * g));
          kb1 = *reinterpret_cast<const u4v*>(keep_s + 2 * (qt * 16 + 4 * g) + 4);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[r], 0.125f * LOG2E, -lr[r]));      // lse_s holds lse * log2(e)
          pv = kvalid ? pv : 0.f;
          float dpv = dp[r];
          if constexpr (DROP) {
            const u4v kb = r < 2 ? kb0 : kb1;
            const unsigned word = kb[2 * (r & 1) + (kt >= 2 ? 1 : 0)];
            const bool keep = (word >> (key & 31)) & 1u;
            if (pass == 0) pv = keep ? pv * p.dr.scale : 0.f; else dpv = keep ? dpv * p.dr.scale : 0.f;
          }
          b16[qt][r] = pass == 0 ? (half_t)pv : (half_t)(pv * (dpv - dr[r]) * 0.125f);
        }
      }
      f4 acc[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        acc[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KT / 2; ++ks)
          acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tr_frag(xt, ks * 32, ks * 32 + 16, dt * 16, lane),
                                                           cat4(b16[2 * ks], b16[2 * ks + 1]), acc[dt], 0, 0, 0);
      }
      store_rows(pass == 0 ? dv : dk, ld, acc, kt * 16, L, scr, lane);
      if (dbias) add_rounded(csum, acc);         // masked keys and keys past L are exact zeros (Pd and dS are)
      __builtin_amdgcn_sched_barrier(0);         // one key tile at a time, as in attention_f16.hip
    }
    if (dbias) store_colsum(dbias + (pass == 0 ? 2 : 1) * D, csum, lane);
  }
}

// ---------------------------------------------------------------- elementwise kernels on fp16 tensors, 8 halves per access
__device__ __forceinline__ float gelu_erf(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  return cdf + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
__global__ __launch_bounds__(256) void gelu16_fwd_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const h8 v = *reinterpret_cast<const h8*>(x + i * 8);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)gelu_erf((float)v[j]);
    *reinterpret_cast<h8*>(y + i * 8) = o;
  }
}
__global__ __launch_bounds__(256) void gelu16_bwd_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                         half_t* __restrict__ dx, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const h8 v = *reinterpret_cast<const h8*>(x + i * 8), d = *reinterpret_cast<const h8*>(dy + i * 8);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)d[j] * gelu_erf_grad((float)v[j]));
    *reinterpret_cast<h8*>(dx + i * 8) = o;
  }
}

// y = fp16(x o keep * scale + resid): elements 8i .. 8i+7 are Philox quads 2i and 2i+1 of hmmc_dropout_fwd's numbering.
// y may alias x.
__global__ __launch_bounds__(256) void dropout16_kernel(const half_t* x, const half_t* __restrict__ resid, half_t* y, long n8, Drop d) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    unsigned w[2][4];
    drop_words(d, (unsigned long)(2 * i), w[0]);
    drop_words(d, (unsigned long)(2 * i + 1), w[1]);
    const h8 v = *reinterpret_cast<const h8*>(x + i * 8);
    h8 r = {};
    if (resid) r = *reinterpret_cast<const h8*>(resid + i * 8);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((w[j >> 2][j & 3] >= d.thresh ? (float)v[j] * d.scale : 0.f) + (float)r[j]);
    *reinterpret_cast<h8*>(y + i * 8) = o;
  }
}
// the p = 0 form with a residual: y = fp16(x + resid), no multiplication
__global__ __launch_bounds__(256) void add16_kernel(const half_t* x, const half_t* __restrict__ resid, half_t* y, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const h8 v = *reinterpret_cast<const h8*>(x + i * 8), r = *reinterpret_cast<const h8*>(resid + i * 8);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)v[j] + (float)r[j]);
    *reinterpret_cast<h8*>(y + i * 8) = o;
  }
}

// pooler: y = fp16(tanh(y)) in place; dz = fp16(dy (1 - y^2))
__global__ __launch_bounds__(256) void tanh16_kernel(half_t* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = (half_t)tanhf((float)y[i]);
}
__global__ __launch_bounds__(256) void tanh16_bwd_kernel(const half_t* __restrict__ dy, const half_t* __restrict__ y,
                                                         half_t* __restrict__ dz, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float t = (float)y[i];
    dz[i] = (half_t)((float)dy[i] * (1.0f - t * t));
  }
}

int mattn16_args_ok(const void* qkv, const long* mask, int b, int L, int H, float p) {
  if (!qkv || !mask || b <= 0 || L <= 0 || H <= 0 || !drop_p_ok(p)) return HMMC_ERR_ARG;
  if (L > MATTN_F16_MAXL || (long)b * L * 3 * DH * H > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  return HMMC_OK;
}

}  // namespace

extern "C" int hmmc_masked_attention_f16_fwd(const void* qkv, const long* key_mask, void* out, float* lse, int b, int L, int H, float p,
                                             long seed, int site, hipStream_t stream) {
  if (!out || !lse) return HMMC_ERR_ARG;
  CK(mattn16_args_ok(qkv, key_mask, b, L, H, p));
  MAttnArgs a{};
  a.qkv = (const half_t*)qkv; a.mask = key_mask; a.out = (half_t*)out; a.lse = lse; a.nseq = b; a.L = L; a.H = H;
  a.dr = make_drop(p, seed, site);
  const long pairs = (long)b * H;
  const dim3 grid((unsigned)((pairs + MFWD_WPB - 1) / MFWD_WPB)), block(64 * MFWD_WPB);
  const size_t lds2 = MFWD_WPB * (32 + 16) * LDS_STRIDE * 2, lds4 = MFWD_WPB * (64 + 16) * LDS_STRIDE * 2;
  if (p > 0.f) {
    if (L <= 32) hipLaunchKernelGGL((mattn16_fwd_kernel<2, true>), grid, block, lds2, stream, a);
    else hipLaunchKernelGGL((mattn16_fwd_kernel<4, true>), grid, block, lds4, stream, a);
  } else {
    if (L <= 32) hipLaunchKernelGGL((mattn16_fwd_kernel<2, false>), grid, block, lds2, stream, a);
    else hipLaunchKernelGGL((mattn16_fwd_kernel<4, false>), grid, block, lds4, stream, a);
  }
  return hmmc_launch_status();
}

extern "C" int hmmc_masked_attention_f16_bwd(const void* qkv, const long* key_mask, const float* lse, const void* dout, void* dqkv,
                                             float* dbias_partial, int b, int L, int H, float p, long seed, int site,
                                             hipStream_t stream) {
  if (!lse || !dout || !dqkv) return HMMC_ERR_ARG;
  CK(mattn16_args_ok(qkv, key_mask, b, L, H, p));
  MAttnArgs a{};
  a.qkv = (const half_t*)qkv; a.mask = key_mask; a.lse = (float*)lse; a.dout = (const half_t*)dout; a.dqkv = (half_t*)dqkv;
  a.dbias = dbias_partial; a.nseq = b; a.L = L; a.H = H;
  a.dr = make_drop(p, seed, site);
  const long pairs = (long)b * H;
  const dim3 grid((unsigned)((pairs + MBWD_WPB - 1) / MBWD_WPB)), block(64 * MBWD_WPB);
  const size_t lds2 = MBWD_WPB * ((32 + 16) * LDS_STRIDE * 2 + 2 * 32 * 4 + 32 * 8);
  const size_t lds4 = MBWD_WPB * ((64 + 16) * LDS_STRIDE * 2 + 2 * 64 * 4 + 64 * 8);
  if (p > 0.f) {
    if (L <= 32) hipLaunchKernelGGL((mattn16_bwd_kernel<2, true>), grid, block, lds2, stream, a);
    else hipLaunchKernelGGL((mattn16_bwd_kernel<4, true>), grid, block, lds4, stream, a);
  } else {
    if (L <= 32) hipLaunchKernelGGL((mattn16_bwd_kernel<2, false>), grid, block, lds2, stream, a);
    else hipLaunchKernelGGL((mattn16_bwd_kernel<4, false>), grid, block, lds4, stream, a);
  }
  return hmmc_launch_status();
}

extern "C" int hmmc_gelu_erf_f16_fwd(const void* x, void* y, long n, hipStream_t stream) {
  if (!x || !y || n <= 0) return HMMC_ERR_ARG;
  if ((n & 7) || (((uintptr_t)x | (uintptr_t)y) & 15)) return HMMC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gelu16_fwd_kernel, dim3(nblk(n / 8)), dim3(256), 0, stream, (const half_t*)x, (half_t*)y, n / 8);
  return hmmc_launch_status();
}

extern "C" int hmmc_gelu_erf_f16_bwd(const void* x, const void* dy, void* dx, long n, hipStream_t stream) {
  if (!x || !dy || !dx || n <= 0) return HMMC_ERR_ARG;
  if ((n & 7) || (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15)) return HMMC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gelu16_bwd_kernel, dim3(nblk(n / 8)), dim3(256), 0, stream, (const half_t*)x, (const half_t*)dy, (half_t*)dx, n / 8);
  return hmmc_launch_status();
}

extern "C" int hmmc_dropout_f16_fwd(const void* x, const void* resid, void* y, long n, float p, long seed, int site,
                                    hipStream_t stream) {
  if (!x || !y || n <= 0 || !drop_p_ok(p)) return HMMC_ERR_ARG;
  if ((n & 7) || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)resid) & 15)) return HMMC_ERR_UNSUPPORTED;
  if (p == 0.f) {
    if (!resid) {
      if (x != y) HIPCK(hipMemcpyAsync(y, x, (size_t)n * 2, hipMemcpyDeviceToDevice, stream));
      return HMMC_OK;
    }
    hipLaunchKernelGGL(add16_kernel, dim3(nblk(n / 8)), dim3(256), 0, stream, (const half_t*)x, (const half_t*)resid, (half_t*)y, n / 8);
  } else {
    hipLaunchKernelGGL(dropout16_kernel, dim3(nblk(n / 8)), dim3(256), 0, stream, (const half_t*)x, (const half_t*)resid, (half_t*)y,
                       n / 8, make_drop(p, seed, site));
  }
  return hmmc_launch_status();
}

extern "C" int hmmc_dropout_f16_bwd(const void* dy, void* dx, long n, float p, long seed, int site, hipStream_t stream) {
  return hmmc_dropout_f16_fwd(dy, nullptr, dx, n, p, seed, site, stream);
}

int bert_tanh_f16(void* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(tanh16_kernel, dim3(nblk(n)), dim3(256), 0, s, (half_t*)y, n);
  return hmmc_launch_status();
}
int bert_tanh_bwd_f16(const void* dy, const void* y, void* dz, long n, hipStream_t s) {
  hipLaunchKernelGGL(tanh16_bwd_kernel, dim3(nblk(n)), dim3(256), 0, s, (const half_t*)dy, (const half_t*)y, (half_t*)dz, n);
  return hmmc_launch_status();
}
