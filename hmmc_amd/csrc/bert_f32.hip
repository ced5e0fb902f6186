// The Chinese text branch: an fp32 post-LN BERT encoder (reference modules/module_cross.py:257-265,273-277: HuggingFace
// BertModel behind AutoModel - embeddings + LayerNorm, nlayers x [self-attention with a key-padding mask, dense + residual +
// LayerNorm, dense + erf-GELU, dense + residual + LayerNorm], tanh pooler; dropout after the embedding LayerNorm, on the
// attention probabilities and after both output projections).  Everything is fp32: the GEMMs are hmmc_gemm_f32 (exact f32
// MFMA), nothing is rounded to fp16.  New kernels here: embedding + LayerNorm in one pass, key-masked attention with
// dropout on the probabilities, counter-based dropout, the pooler's tanh; bert_tower.hip SEQUENCES them, and the fp16
// regime's kernels of bert_f16.hip, behind hmmc_bert_fwd / hmmc_bert_bwd.  No atomics, fixed summation order: bit-identical
// from run to run.
#include "bert_regime.h"
#include "philox.h"
#include <algorithm>

namespace {

// ---------------------------------------------------------------- dropout (the generator: philox.h)
// y = x o keep * scale (+ resid); four consecutive elements per Philox call.  y may alias x.
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, const float* __restrict__ resid, float* y, long n4, Drop d) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    unsigned w[4];
    drop_words(d, (unsigned long)i, w);
    f4 v = *reinterpret_cast<const f4*>(x + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = w[j] >= d.thresh ? v[j] * d.scale : 0.f;
    if (resid) v += *reinterpret_cast<const f4*>(resid + i * 4);
    *reinterpret_cast<f4*>(y + i * 4) = v;
  }
}
// the p = 0 form: no multiplication at all
__global__ __launch_bounds__(256) void copy_add_kernel(const float* x, const float* __restrict__ resid, float* y, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f4 v = *reinterpret_cast<const f4*>(x + i * 4);
    if (resid) v += *reinterpret_cast<const f4*>(resid + i * 4);
    *reinterpret_cast<f4*>(y + i * 4) = v;
  }
}

// ---------------------------------------------------------------- embedding + LayerNorm, one pass, a wave per row
// e[r] = word[ids[r]] + pos[r % L] + type[0];  y[r] = LN(e[r]);  D <= 1024, D % 4 == 0.
// An id outside [0, vocab) never indexes the table: its word row counts as zero and *err is set (hmmc_text_embed's rule).
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const long* __restrict__ ids, const float* __restrict__ word,
                                                            const float* __restrict__ pos, const float* __restrict__ type0,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ e, float* __restrict__ y, float* __restrict__ mean,
                                                            float* __restrict__ rstd, long rows, int L, int D, long vocab,
                                                            float eps, int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
    const long id = ids[r];
    const bool ok = id >= 0 && id < vocab;
    if (!ok && lane == 0 && err) *err = 1;
    const float* wr = word + (ok ? id : 0) * (long)D;
    const float* pr = pos + (long)(r % L) * D;
    f4 v[4];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane * 4 + 256 * k;
      v[k] = f4{0.f, 0.f, 0.f, 0.f};
      if (c < D) {
        f4 w = *reinterpret_cast<const f4*>(wr + c);
        if (!ok) w = f4{0.f, 0.f, 0.f, 0.f};
        v[k] = w + *reinterpret_cast<const f4*>(pr + c) + *reinterpret_cast<const f4*>(type0 + c);
        s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
      }
    }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane * 4 + 256 * k;
      if (c < D) {
        const f4 t = v[k] - mu;
        q += (t[0] * t[0] + t[1] * t[1]) + (t[2] * t[2] + t[3] * t[3]);
      }
    }
    const float rs = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane * 4 + 256 * k;
      if (c < D) {
        if (e) *reinterpret_cast<f4*>(e + r * D + c) = v[k];
        const f4 g = *reinterpret_cast<const f4*>(gamma + c), b = *reinterpret_cast<const f4*>(beta + c);
        *reinterpret_cast<f4*>(y + r * D + c) = (v[k] - mu) * rs * g + b;
      }
    }
  }
}

// ---------------------------------------------------------------- key-masked fp32 attention, head dim 64
// qkv: [b*L, 3*D] (Q | K | V), mask: int64 [b, L] (nonzero = valid key), out: [b*L, D], probs: [b, H, L, L] = the probabilities
// AFTER dropout (what multiplies V), praw (DROP only): the softmax itself.  K and V rows of masked keys are never used: they
// are staged as zeros, so whatever they hold (finite or not) cannot reach a result.  Dot products and the sums over keys run in
// four interleaved partial sums (a shorter rounding chain than one running sum).
__device__ __forceinline__ float dot64(const float* a, const float* b) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int d = 0; d < 64; d += 4) { s0 += a[d] * b[d]; s1 += a[d + 1] * b[d + 1]; s2 += a[d + 2] * b[d + 2]; s3 += a[d + 3] * b[d + 3]; }
  return (s0 + s1) + (s2 + s3);
}

// L <= 64: one wave per (sequence, head)
template <bool DROP>
__global__ __launch_bounds__(64) void mattn_fwd_kernel(const float* __restrict__ qkv, const long* __restrict__ mask,
                                                       float* __restrict__ out, float* __restrict__ probs,
                                                       float* __restrict__ praw, int L, int H, Drop dr) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x;
  const int D = H * 64;
  float* q = sm; float* k = q + L * 65; float* v = k + L * 65; float* p = v + L * 65;   // p: [L][L]
  int* valid = (int*)(p + L * L);
  if (lane < L) valid[lane] = mask[(long)b * L + lane] != 0;
  __syncthreads();
  for (int idx = lane; idx < L * 64; idx += 64) {
    const int f = idx >> 6, d = idx & 63;
    const float* base = qkv + ((long)b * L + f) * 3 * D + hd * 64 + d;
    const bool ok = valid[f];
    q[f * 65 + d] = base[0] * 0.125f;
    k[f * 65 + d] = ok ? base[D] : 0.f;
    v[f * 65 + d] = ok ? base[2 * D] : 0.f;
  }
  __syncthreads();
  for (int idx = lane; idx < L * L; idx += 64) {
    const int i = idx / L, j = idx % L;
    p[idx] = valid[j] ? dot64(q + i * 65, k + j * 65) : -INFINITY;
  }
  __syncthreads();
  const unsigned long pbase = (unsigned long)blockIdx.x * L * L;
  if (lane < L) {
    float* row = p + lane * L;
    float m = -INFINITY;
    for (int j = 0; j < L; ++j) m = fmaxf(m, row[j]);
    float s = 0.f;
    for (int j = 0; j < L; ++j) { const float e = row[j] == -INFINITY ? 0.f : expf(row[j] - m); row[j] = e; s += e; }
    for (int j = 0; j < L; ++j) row[j] = row[j] / s;
  }
  __syncthreads();
  float* pg = probs + pbase;
  for (int idx = lane; idx < L * L; idx += 64) {
    float pj = p[idx];
    if (DROP) {
      praw[pbase + idx] = pj;
      pj = drop_keep(dr, pbase + idx) ? pj * dr.scale : 0.f;
      p[idx] = pj;
    }
    pg[idx] = pj;
  }
  __syncthreads();
  for (int i = 0; i < L; ++i) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; ++j) o[j & 3] += p[i * L + j] * v[j * 65 + lane];
    out[((long)b * L + i) * D + hd * 64 + lane] = (o[0] + o[1]) + (o[2] + o[3]);
  }
}

// dPd[i][j] = <dO[i], V[j]>; delta[i] = sum_j Pd o dPd (= sum_j P o dP); dS = P o (dPd o keep * scale - delta) / 8;
// dQ = dS K; dK = dS^T Q; dV = Pd^T dO.  Masked keys: P = Pd = 0 exactly, so their dK / dV are exactly zero.
template <bool DROP>
__global__ __launch_bounds__(64) void mattn_bwd_kernel(const float* __restrict__ qkv, const long* __restrict__ mask,
                                                       const float* __restrict__ probs, const float* __restrict__ praw,
                                                       const float* __restrict__ dout, float* __restrict__ dqkv, int L, int H,
                                                       Drop dr) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x;
  const int D = H * 64;
  float* q = sm; float* k = q + L * 65; float* v = k + L * 65; float* dO = v + L * 65;
  float* p = dO + L * 65; float* ds = p + L * L;                 // p: Pd;  ds: dPd, then dS
  float* pr = DROP ? ds + L * L : p;                             // the softmax itself
  int* valid = (int*)(ds + (DROP ? 2 : 1) * L * L);              // behind the last float array either way
  if (lane < L) valid[lane] = mask[(long)b * L + lane] != 0;
  __syncthreads();
  for (int idx = lane; idx < L * 64; idx += 64) {
    const int f = idx >> 6, d = idx & 63;
    const float* base = qkv + ((long)b * L + f) * 3 * D + hd * 64 + d;
    const bool ok = valid[f];
    q[f * 65 + d] = base[0];
    k[f * 65 + d] = ok ? base[D] : 0.f;
    v[f * 65 + d] = ok ? base[2 * D] : 0.f;
    dO[f * 65 + d] = dout[((long)b * L + f) * D + hd * 64 + d];
  }
  const unsigned long pbase = (unsigned long)blockIdx.x * L * L;
  for (int idx = lane; idx < L * L; idx += 64) {
    p[idx] = probs[pbase + idx];
    if (DROP) pr[idx] = praw[pbase + idx];
  }
  __syncthreads();
  for (int idx = lane; idx < L * L; idx += 64) {
    const int i = idx / L, j = idx % L;
    ds[idx] = dot64(dO + i * 65, v + j * 65);
  }
  __syncthreads();
  if (lane < L) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; ++j) t[j & 3] += p[lane * L + j] * ds[lane * L + j];
    const float dot = (t[0] + t[1]) + (t[2] + t[3]);
    for (int j = 0; j < L; ++j) {
      float dp = ds[lane * L + j];
      if (DROP) dp = drop_keep(dr, pbase + (unsigned long)(lane * L + j)) ? dp * dr.scale : 0.f;
      ds[lane * L + j] = pr[lane * L + j] * (dp - dot) * 0.125f;
    }
  }
  __syncthreads();
  for (int i = 0; i < L; ++i) {
    float dq[4] = {0.f, 0.f, 0.f, 0.f}, dk[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; ++j) {
      dq[j & 3] += ds[i * L + j] * k[j * 65 + lane];
      dk[j & 3] += ds[j * L + i] * q[j * 65 + lane];
      dv[j & 3] += p[j * L + i] * dO[j * 65 + lane];
    }
    float* o = dqkv + ((long)b * L + i) * 3 * D + hd * 64 + lane;
    o[0] = (dq[0] + dq[1]) + (dq[2] + dq[3]);
    o[D] = (dk[0] + dk[1]) + (dk[2] + dk[3]);
    o[2 * D] = (dv[0] + dv[1]) + (dv[2] + dv[3]);
  }
}

// 65 <= L <= 256: one 256-thread workgroup per (sequence, head), K and V in LDS ([L][65]), a wave per query row
constexpr int MA_MAXL = MATTN_F32_MAXL;
template <bool DROP>
__global__ __launch_bounds__(256) void mattn_long_fwd_kernel(const float* __restrict__ qkv, const long* __restrict__ mask,
                                                             float* __restrict__ out, float* __restrict__ probs,
                                                             float* __restrict__ praw, int L, int H, Drop dr) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int D = H * 64;
  float* k = sm; float* v = k + L * 65; float* prow = v + L * 65;            // prow: [4][MA_MAXL], qrow: [4][64]
  float* qrow = prow + 4 * MA_MAXL;
  int* valid = (int*)(qrow + 4 * 64);                                        // [MA_MAXL]
  for (int j = threadIdx.x; j < L; j += 256) valid[j] = mask[(long)b * L + j] != 0;
  __syncthreads();
  for (int idx = threadIdx.x; idx < L * 64; idx += 256) {
    const int f = idx >> 6, d = idx & 63;
    const float* base = qkv + ((long)b * L + f) * 3 * D + hd * 64 + d;
    const bool ok = valid[f];
    k[f * 65 + d] = ok ? base[D] : 0.f;
    v[f * 65 + d] = ok ? base[2 * D] : 0.f;
  }
  __syncthreads();
  float* pw = prow + w * MA_MAXL;
  float* qw = qrow + w * 64;
  const unsigned long pbase = (unsigned long)blockIdx.x * L * L;
  for (int i = w; i < L; i += 4) {
    qw[lane] = qkv[((long)b * L + i) * 3 * D + hd * 64 + lane] * 0.125f;
    __builtin_amdgcn_wave_barrier();
    float sc[4];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = lane + 64 * t;
      float s = -INFINITY;
      if (j < L && valid[j]) s = dot64(qw, k + j * 65);
      sc[t] = s;
      m = fmaxf(m, s);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) { sc[t] = (sc[t] == -INFINITY) ? 0.f : expf(sc[t] - m); sum += sc[t]; }
    const float tot = wave_sum(sum);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = lane + 64 * t;
      if (j < L) {
        float pj = sc[t] / tot;
        const unsigned long at = pbase + (unsigned long)i * L + j;
        if (DROP) { praw[at] = pj; pj = drop_keep(dr, at) ? pj * dr.scale : 0.f; }
        pw[j] = pj;
        probs[at] = pj;
      }
    }
    __builtin_amdgcn_wave_barrier();
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; ++j) o[j & 3] += pw[j] * v[j * 65 + lane];
    out[((long)b * L + i) * D + hd * 64 + lane] = (o[0] + o[1]) + (o[2] + o[3]);
    __builtin_amdgcn_wave_barrier();
  }
}

// Pass A: a wave per query row (dQ, and delta[i] into LDS); pass B: a wave per key row (dK, dV), re-forming dPd[i][j] by a wave
// reduction.  Every output element has one owner.
template <bool DROP>
__global__ __launch_bounds__(256) void mattn_long_bwd_kernel(const float* __restrict__ qkv, const long* __restrict__ mask,
                                                             const float* __restrict__ probs, const float* __restrict__ praw,
                                                             const float* __restrict__ dout, float* __restrict__ dqkv, int L,
                                                             int H, Drop dr) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int D = H * 64;
  float* k = sm; float* v = k + L * 65; float* drow = v + L * 65;            // drow: [4][MA_MAXL] dP of a row; delta: [MA_MAXL]
  float* delta = drow + 4 * MA_MAXL;
  int* valid = (int*)(delta + MA_MAXL);
  for (int j = threadIdx.x; j < L; j += 256) valid[j] = mask[(long)b * L + j] != 0;
  __syncthreads();
  for (int idx = threadIdx.x; idx < L * 64; idx += 256) {
    const int f = idx >> 6, d = idx & 63;
    const float* base = qkv + ((long)b * L + f) * 3 * D + hd * 64 + d;
    const bool ok = valid[f];
    k[f * 65 + d] = ok ? base[D] : 0.f;
    v[f * 65 + d] = ok ? base[2 * D] : 0.f;
  }
  __syncthreads();
  const unsigned long pbase = (unsigned long)blockIdx.x * L * L;
  const float* pd = probs + pbase;
  const float* pr = DROP ? praw + pbase : pd;
  float* dw = drow + w * MA_MAXL;
  for (int i = w; i < L; i += 4) {
    const float dO = dout[((long)b * L + i) * D + hd * 64 + lane];
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; ++j) {
      const float dp = wave_sum(dO * v[j * 65 + lane]);
      if (lane == 0) dw[j] = dp;
      t[j & 3] += pd[(long)i * L + j] * dp;
    }
    const float dot = (t[0] + t[1]) + (t[2] + t[3]);
    if (lane == 0) delta[i] = dot;
    __builtin_amdgcn_wave_barrier();
    float dq[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; ++j) {
      float dp = dw[j];
      if (DROP) dp = drop_keep(dr, pbase + (unsigned long)i * L + j) ? dp * dr.scale : 0.f;
      dq[j & 3] += pr[(long)i * L + j] * (dp - dot) * k[j * 65 + lane];
    }
    dqkv[((long)b * L + i) * 3 * D + hd * 64 + lane] = ((dq[0] + dq[1]) + (dq[2] + dq[3])) * 0.125f;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  for (int j = w; j < L; j += 4) {
    const float vj = v[j * 65 + lane];
    float dk[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < L; ++i) {
      const float dO = dout[((long)b * L + i) * D + hd * 64 + lane];
      const float q = qkv[((long)b * L + i) * 3 * D + hd * 64 + lane];
      float dp = wave_sum(dO * vj);
      if (DROP) dp = drop_keep(dr, pbase + (unsigned long)i * L + j) ? dp * dr.scale : 0.f;
      dv[i & 3] += pd[(long)i * L + j] * dO;
      dk[i & 3] += pr[(long)i * L + j] * (dp - delta[i]) * q;
    }
    float* o = dqkv + ((long)b * L + j) * 3 * D + hd * 64 + lane;
    o[D] = ((dk[0] + dk[1]) + (dk[2] + dk[3])) * 0.125f;
    o[2 * D] = (dv[0] + dv[1]) + (dv[2] + dv[3]);
  }
}

// ---------------------------------------------------------------- pooler: y = tanh(y) in place; dz = dy (1 - y^2)
__global__ __launch_bounds__(256) void tanh_kernel(float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = tanhf(y[i]);
}
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                       float* __restrict__ dz, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dz[i] = dy[i] * (1.0f - y[i] * y[i]);
}

// what the two attention entry points check alike
int mattn_args_ok(const float* qkv, const long* mask, const float* probs, const float* probs_raw, int b, int L, int H, float p) {
  if (!qkv || !mask || !probs || b <= 0 || L <= 0 || H <= 0 || !drop_p_ok(p) || (p > 0.f && !probs_raw)) return HMMC_ERR_ARG;
  return L > MA_MAXL ? HMMC_ERR_UNSUPPORTED : HMMC_OK;
}

}  // namespace

extern "C" int hmmc_dropout_fwd(const float* x, const float* resid, float* y, long n, float p, long seed, int site,
                                hipStream_t stream) {
  if (!x || !y || n <= 0 || !drop_p_ok(p)) return HMMC_ERR_ARG;
  if ((n & 3) || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)resid) & 15)) return HMMC_ERR_UNSUPPORTED;
  if (p == 0.f) {
    if (!resid && x == y) return HMMC_OK;
    hipLaunchKernelGGL(copy_add_kernel, dim3(nblk(n / 4)), dim3(256), 0, stream, x, resid, y, n / 4);
  } else {
    hipLaunchKernelGGL(dropout_kernel, dim3(nblk(n / 4)), dim3(256), 0, stream, x, resid, y, n / 4, make_drop(p, seed, site));
  }
  return hmmc_launch_status();
}

extern "C" int hmmc_dropout_bwd(const float* dy, float* dx, long n, float p, long seed, int site, hipStream_t stream) {
  return hmmc_dropout_fwd(dy, nullptr, dx, n, p, seed, site, stream);
}

extern "C" int hmmc_bert_embed_fwd(const long* ids, const float* word, const float* pos, const float* type0, const float* gamma,
                                   const float* beta, float* e, float* y, float* mean, float* rstd, long rows, int L, int D,
                                   long vocab, float eps, int* err_flag, hipStream_t stream) {
  if (!ids || !word || !pos || !type0 || !gamma || !beta || !y || !mean || !rstd || rows <= 0 || L <= 0 || vocab <= 0) return HMMC_ERR_ARG;
  if ((D & 3) || D <= 0 || D > 1024) return HMMC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(bert_embed_ln_kernel, dim3(nblk(rows * 64, hmmc_num_cus() * 8)), dim3(256), 0, stream, ids, word, pos, type0, gamma,
                     beta, e, y, mean, rstd, rows, L, D, vocab, eps, err_flag);
  return hmmc_launch_status();
}

extern "C" size_t hmmc_bert_embed_bwd_workspace(long rows, int L, int D) {
  const int nseq = (int)(rows / (L > 0 ? L : 1));
  return std::max(hmmc_layernorm_bwd_workspace((int)rows, D), hmmc_colsum_workspace(nseq > 0 ? nseq : 1, L * D));
}

extern "C" int hmmc_bert_embed_bwd(const long* ids, const float* dy, const float* e, const float* gamma, const float* mean,
                                   const float* rstd, float* de, float* dword, float* dpos, float* dtype, float* dgamma, float* dbeta,
                                   long rows, int L, int D, long vocab, int max_pos, int type_vocab, void* workspace, size_t ws_bytes,
                                   hipStream_t stream) {
  if (!ids || !dy || !e || !gamma || !mean || !rstd || !de || !dword || !dpos || !dtype || !dgamma || !dbeta || rows <= 0 || L <= 0 ||
      vocab <= 0 || type_vocab <= 0 || max_pos < L || rows % L)
    return HMMC_ERR_ARG;
  if ((D & 7) || D > 1024 || rows > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  if (ws_bytes < hmmc_bert_embed_bwd_workspace(rows, L, D)) return HMMC_ERR_WORKSPACE;
  HIPCK(hipMemsetAsync(dtype, 0, (size_t)type_vocab * D * 4, stream));
  // the LayerNorm backward; the column sums of its dx over ALL rows are the gradient of token type 0
  CK(hmmc_layernorm_bwd(dy, e, gamma, mean, rstd, nullptr, de, dgamma, dbeta, dtype, nullptr, (int)rows, D, D, 1, workspace, ws_bytes, stream));
  HIPCK(hipMemsetAsync(dword, 0, (size_t)vocab * D * 4, stream));
  CK(hmmc_text_embed_bwd(ids, de, dword, rows, D, vocab, 1, stream));
  // position l: the sum over sequences of row l, i.e. the column sums of de seen as [nseq, L * D]
  HIPCK(hipMemsetAsync(dpos, 0, (size_t)max_pos * D * 4, stream));
  return hmmc_colsum(de, dpos, (int)(rows / L), L * D, (long)L * D, 1, 1, 0, workspace, ws_bytes, stream);
}

extern "C" int hmmc_masked_attention_fwd(const float* qkv, const long* key_mask, float* out, float* probs, float* probs_raw, int b,
                                         int L, int H, float p, long seed, int site, hipStream_t stream) {
  if (!out) return HMMC_ERR_ARG;
  CK(mattn_args_ok(qkv, key_mask, probs, probs_raw, b, L, H, p));
  const Drop dr = make_drop(p, seed, site);
  const dim3 grid(b * H);
  if (L > 64) {
    const size_t lds = (size_t)(2 * L * 65 + 4 * MA_MAXL + 4 * 64 + MA_MAXL) * sizeof(float);
    if (p > 0.f) hmmc_launch_lds<mattn_long_fwd_kernel<true>>(HMMC_LDS_MOST, grid, dim3(256), lds, stream, qkv, key_mask, out, probs, probs_raw, L, H, dr);
    else hmmc_launch_lds<mattn_long_fwd_kernel<false>>(HMMC_LDS_MOST, grid, dim3(256), lds, stream, qkv, key_mask, out, probs, probs_raw, L, H, dr);
    return hmmc_launch_status();
  }
  const size_t lds = (size_t)(3 * L * 65 + L * L + L) * sizeof(float);
  if (p > 0.f) hmmc_launch_lds<mattn_fwd_kernel<true>>(HMMC_LDS_MOST, grid, dim3(64), lds, stream, qkv, key_mask, out, probs, probs_raw, L, H, dr);
  else hmmc_launch_lds<mattn_fwd_kernel<false>>(HMMC_LDS_MOST, grid, dim3(64), lds, stream, qkv, key_mask, out, probs, probs_raw, L, H, dr);
  return hmmc_launch_status();
}

extern "C" int hmmc_masked_attention_bwd(const float* qkv, const long* key_mask, const float* probs, const float* probs_raw,
                                         const float* dout, float* dqkv, int b, int L, int H, float p, long seed, int site,
                                         hipStream_t stream) {
  if (!dout || !dqkv) return HMMC_ERR_ARG;
  CK(mattn_args_ok(qkv, key_mask, probs, probs_raw, b, L, H, p));
  const Drop dr = make_drop(p, seed, site);
  const dim3 grid(b * H);
  if (L > 64) {
    const size_t lds = (size_t)(2 * L * 65 + 4 * MA_MAXL + MA_MAXL + MA_MAXL) * sizeof(float);
    if (p > 0.f) hmmc_launch_lds<mattn_long_bwd_kernel<true>>(HMMC_LDS_MOST, grid, dim3(256), lds, stream, qkv, key_mask, probs, probs_raw, dout, dqkv, L, H, dr);
    else hmmc_launch_lds<mattn_long_bwd_kernel<false>>(HMMC_LDS_MOST, grid, dim3(256), lds, stream, qkv, key_mask, probs, probs_raw, dout, dqkv, L, H, dr);
    return hmmc_launch_status();
  }
  const size_t lds = (size_t)(4 * L * 65 + (p > 0.f ? 3 : 2) * L * L + L) * sizeof(float);
  if (p > 0.f) hmmc_launch_lds<mattn_bwd_kernel<true>>(HMMC_LDS_MOST, grid, dim3(64), lds, stream, qkv, key_mask, probs, probs_raw, dout, dqkv, L, H, dr);
  else hmmc_launch_lds<mattn_bwd_kernel<false>>(HMMC_LDS_MOST, grid, dim3(64), lds, stream, qkv, key_mask, probs, probs_raw, dout, dqkv, L, H, dr);
  return hmmc_launch_status();
}

int bert_tanh_f32(float* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(tanh_kernel, dim3(nblk(n)), dim3(256), 0, s, y, n);
  return hmmc_launch_status();
}
int bert_tanh_bwd_f32(const float* dy, const float* y, float* dz, long n, hipStream_t s) {
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(nblk(n)), dim3(256), 0, s, dy, y, dz, n);
  return hmmc_launch_status();
}
