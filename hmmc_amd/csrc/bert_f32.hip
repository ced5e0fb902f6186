// The Chinese text branch: an fp32 post-LN BERT encoder (reference modules/module_cross.py:257-265,273-277: HuggingFace
// BertModel behind AutoModel - embeddings + LayerNorm, nlayers x [self-attention with a key-padding mask, dense + residual +
// LayerNorm, dense + erf-GELU, dense + residual + LayerNorm], tanh pooler; dropout after the embedding LayerNorm, on the
// attention probabilities and after both output projections).  Everything is fp32: the GEMMs are hmmc_gemm_f32 (exact f32
// MFMA), nothing is rounded to fp16.  New kernels here: embedding + LayerNorm in one pass, key-masked attention with
// dropout on the probabilities, counter-based dropout, the pooler's tanh; hmmc_bert_fwd / hmmc_bert_bwd only SEQUENCE
// kernels of this library on the caller's stream.  No atomics, fixed summation order: bit-identical from run to run.
#include "common.h"
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
constexpr int MA_MAXL = 256;
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

// y[M,N] = x[M,K] w[N,K]^T (+ bias) (+ resid);  lda / ldc: row strides of x and y (0 = dense)
inline int linear(const float* x, const float* w, float* y, int M, int N, int K, const float* bias, const float* resid, hipStream_t s,
                  long lda = 0, int ldc = 0) {
  return hmmc_gemm_f32(x, w, y, M, N, K, lda ? lda : K, 1, 1, K, ldc ? ldc : N, 1.0f, bias, resid, nullptr, nullptr,
                       (bias ? EPI_BIAS : 0) | (resid ? EPI_RESID : 0), s);
}
// dx[M,K'] = dy[M,N'] w[N',K'] (+ resid);  ldy / ldx: row strides of dy and dx (0 = dense)
inline int dgrad(const float* dy, const float* w, float* dx, int M, int Np, int Kp, const float* resid, hipStream_t s, long ldy = 0,
                 int ldx = 0) {
  return hmmc_gemm_f32(dy, w, dx, M, Kp, Np, ldy ? ldy : Np, 1, Kp, 1, ldx ? ldx : Kp, 1.0f, nullptr, resid, nullptr, nullptr,
                       resid ? EPI_RESID : 0, s);
}
// dW[N',K'] = dy[T,N']^T x[T,K'];  ldy / ldx: row strides of dy and x (0 = dense)
inline int wgrad(const float* dy, const float* x, float* dw, int T, int Np, int Kp, hipStream_t s, long ldy = 0, long ldx = 0) {
  return hmmc_gemm_f32(dy, x, dw, Np, Kp, T, 1, ldy ? ldy : Np, ldx ? ldx : Kp, 1, Kp, 1.0f, nullptr, nullptr, nullptr, nullptr, 0, s);
}

// activation layout of hmmc_bert_fwd / hmmc_bert_bwd: the embedding's pre-LayerNorm rows and statistics, then one slab per
// layer (keep_acts) or one slab that every layer reuses
struct EmbActs { float *e, *mean, *rstd; size_t bytes; };
struct LayerActs { float *x, *qkv, *probs, *praw, *att, *pre1, *x1, *h, *g, *pre2, *m1, *r1, *m2, *r2; size_t bytes; };
EmbActs carve_emb(char* base, long T, int D) {
  EmbActs a;
  char* p = base;
  a.e = (float*)p; p += al((size_t)T * D * 4);
  a.mean = (float*)p; p += al((size_t)T * 4);
  a.rstd = (float*)p; p += al((size_t)T * 4);
  a.bytes = (size_t)(p - base);
  return a;
}
LayerActs carve_layer(char* base, long T, int D, int I, int nseq, int L, int H, bool attn_drop) {
  LayerActs a;
  const size_t td = al((size_t)T * D * 4), ti = al((size_t)T * I * 4), pp = al((size_t)nseq * H * L * L * 4), tr = al((size_t)T * 4);
  char* p = base;
  a.x = (float*)p; p += td;
  a.qkv = (float*)p; p += al((size_t)T * 3 * D * 4);
  a.probs = (float*)p; p += pp;
  a.praw = attn_drop ? (float*)p : nullptr; p += attn_drop ? pp : 0;
  a.att = (float*)p; p += td;
  a.pre1 = (float*)p; p += td;
  a.x1 = (float*)p; p += td;
  a.h = (float*)p; p += ti;
  a.g = (float*)p; p += ti;
  a.pre2 = (float*)p; p += td;
  a.m1 = (float*)p; p += tr;
  a.r1 = (float*)p; p += tr;
  a.m2 = (float*)p; p += tr;
  a.r2 = (float*)p; p += tr;
  a.bytes = (size_t)(p - base);
  return a;
}

constexpr int BERT_EMB_PARAMS = 5, BERT_LAYER_PARAMS = 16;
inline bool bert_dims_ok(int nseq, int L, int heads, int D, int inter, int nlayers) {
  return nseq > 0 && L > 0 && heads > 0 && nlayers > 0 && inter > 0 && D == heads * 64;
}

}  // namespace

extern "C" int hmmc_dropout_fwd(const float* x, const float* resid, float* y, long n, float p, long seed, int site,
                                hipStream_t stream) {
  if (!x || !y || n <= 0 || !(p >= 0.f) || !(p < 1.f)) return HMMC_ERR_ARG;
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
  if (!qkv || !key_mask || !out || !probs || b <= 0 || L <= 0 || H <= 0 || !(p >= 0.f) || !(p < 1.f)) return HMMC_ERR_ARG;
  if (p > 0.f && !probs_raw) return HMMC_ERR_ARG;
  if (L > MA_MAXL) return HMMC_ERR_UNSUPPORTED;
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
  if (!qkv || !key_mask || !probs || !dout || !dqkv || b <= 0 || L <= 0 || H <= 0 || !(p >= 0.f) || !(p < 1.f)) return HMMC_ERR_ARG;
  if (p > 0.f && !probs_raw) return HMMC_ERR_ARG;
  if (L > MA_MAXL) return HMMC_ERR_UNSUPPORTED;
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

extern "C" int hmmc_bert_pooler_fwd(const float* x, const float* W, const float* bias, float* y, int b, long stride, int D,
                                    hipStream_t stream) {
  if (!x || !W || !bias || !y || b <= 0 || D <= 0 || stride < D) return HMMC_ERR_ARG;
  CK(linear(x, W, y, b, D, D, bias, nullptr, stream, stride, 0));
  hipLaunchKernelGGL(tanh_kernel, dim3(nblk((long)b * D)), dim3(256), 0, stream, y, (long)b * D);
  return hmmc_launch_status();
}

extern "C" int hmmc_bert_pooler_bwd(const float* dy, const float* y, const float* x, const float* W, float* dz, float* dx, float* dW,
                                    float* db, int b, long stride, int D, void* workspace, size_t ws_bytes, hipStream_t stream) {
  if (!dy || !y || !x || !W || !dz || !dx || !dW || !db || b <= 0 || D <= 0 || stride < D) return HMMC_ERR_ARG;
  if (stride > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(nblk((long)b * D)), dim3(256), 0, stream, dy, y, dz, (long)b * D);
  CK(hmmc_launch_status());
  CK(hmmc_colsum(dz, db, b, D, D, 1, 1, 0, workspace, ws_bytes, stream));
  CK(wgrad(dz, x, dW, b, D, D, stream, 0, stride));
  return dgrad(dz, W, dx, b, D, D, nullptr, stream, 0, (int)stride);
}

extern "C" size_t hmmc_bert_act_bytes(int nseq, int L, int heads, int D, int inter, int nlayers, int keep_acts, int attn_dropout) {
  const long T = (long)nseq * L;
  return carve_emb(nullptr, T, D).bytes +
         carve_layer(nullptr, T, D, inter, nseq, L, heads, attn_dropout != 0).bytes * (size_t)(keep_acts ? nlayers : 1);
}
// transient gradients of the backward: six [T, D], two [T, inter], one [T, 3D]
extern "C" size_t hmmc_bert_bwd_scratch_bytes(int nseq, int L, int D, int inter) {
  const long T = (long)nseq * L;
  return 6 * al((size_t)T * D * 4) + 2 * al((size_t)T * inter * 4) + al((size_t)T * 3 * D * 4);
}
extern "C" size_t hmmc_bert_workspace_bytes(int nseq, int L, int D, int inter) {
  const int T = nseq * L;
  size_t w = std::max(hmmc_layernorm_bwd_workspace(T, D), hmmc_colsum_workspace(T, inter));
  w = std::max(w, hmmc_colsum_workspace(T, D));
  return al(std::max(w, hmmc_bert_embed_bwd_workspace(T, L, D)));
}

extern "C" int hmmc_bert_fwd(const long* ids, const long* key_mask, float* y, const void* const* params, void* acts, int keep_acts,
                             int nseq, int L, int heads, int D, int inter, int nlayers, long vocab, float eps, float p_hidden,
                             float p_attn, long seed, int* err_flag, hipStream_t s) {
  if (!ids || !key_mask || !y || !params || !acts || vocab <= 0 || !bert_dims_ok(nseq, L, heads, D, inter, nlayers)) return HMMC_ERR_ARG;
  if (!(p_hidden >= 0.f) || !(p_hidden < 1.f) || !(p_attn >= 0.f) || !(p_attn < 1.f)) return HMMC_ERR_ARG;
  if (L > MA_MAXL || D > 1024 || (inter & 3)) return HMMC_ERR_UNSUPPORTED;
  const long T = (long)nseq * L;
  if (T * std::max(3 * D, inter) > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  const bool adrop = p_attn > 0.f;
  const float* const* P = (const float* const*)params;
  const EmbActs ea = carve_emb((char*)acts, T, D);
  char* const slabs = (char*)acts + ea.bytes;
  const size_t slab = carve_layer(nullptr, T, D, inter, nseq, L, heads, adrop).bytes;
  LayerActs a = carve_layer(slabs, T, D, inter, nseq, L, heads, adrop);
  // x0 = dropout(LN(word + pos + type 0)) into the first slab's input
  CK(hmmc_bert_embed_fwd(ids, P[0], P[1], P[2], P[3], P[4], keep_acts ? ea.e : nullptr, a.x, ea.mean, ea.rstd, T, L, D, vocab, eps,
                         err_flag, s));
  CK(hmmc_dropout_fwd(a.x, nullptr, a.x, T * D, p_hidden, seed, 0, s));
  for (int i = 0; i < nlayers; ++i) {
    const float* const* W = P + BERT_EMB_PARAMS + (size_t)i * BERT_LAYER_PARAMS;
    if (keep_acts) a = carve_layer(slabs + (size_t)i * slab, T, D, inter, nseq, L, heads, adrop);
    // the layer's output: the next slab's input, y for the last layer; without kept activations the one slab's input slot,
    // which is dead once attention.output.dense has read it as its residual
    float* out = i + 1 == nlayers ? y : keep_acts ? carve_layer(slabs + (size_t)(i + 1) * slab, T, D, inter, nseq, L, heads, adrop).x : a.x;
    for (int j = 0; j < 3; ++j)                                    // query | key | value into one [T, 3D] buffer
      CK(linear(a.x, W[2 * j], a.qkv + (size_t)j * D, (int)T, D, D, W[2 * j + 1], nullptr, s, 0, 3 * D));
    CK(hmmc_masked_attention_fwd(a.qkv, key_mask, a.att, a.probs, a.praw, nseq, L, heads, p_attn, seed, 1 + 3 * i, s));
    if (p_hidden > 0.f) {
      CK(linear(a.att, W[6], a.pre1, (int)T, D, D, W[7], nullptr, s));
      CK(hmmc_dropout_fwd(a.pre1, a.x, a.pre1, T * D, p_hidden, seed, 2 + 3 * i, s));
    } else {
      CK(linear(a.att, W[6], a.pre1, (int)T, D, D, W[7], a.x, s));
    }
    CK(hmmc_layernorm_fwd(a.pre1, W[8], W[9], a.x1, a.m1, a.r1, nullptr, (int)T, D, D, eps, 1, s));
    CK(linear(a.x1, W[10], a.h, (int)T, inter, D, W[11], nullptr, s));
    CK(hmmc_gelu_erf_fwd(a.h, a.g, T * inter, s));
    if (p_hidden > 0.f) {
      CK(linear(a.g, W[12], a.pre2, (int)T, D, inter, W[13], nullptr, s));
      CK(hmmc_dropout_fwd(a.pre2, a.x1, a.pre2, T * D, p_hidden, seed, 3 + 3 * i, s));
    } else {
      CK(linear(a.g, W[12], a.pre2, (int)T, D, inter, W[13], a.x1, s));
    }
    CK(hmmc_layernorm_fwd(a.pre2, W[14], W[15], out, a.m2, a.r2, nullptr, (int)T, D, D, eps, 1, s));
  }
  return HMMC_OK;
}

extern "C" int hmmc_bert_bwd(const float* dy, const long* ids, const long* key_mask, const void* const* params, void* const* grads,
                             const void* acts, void* scratch, int nseq, int L, int heads, int D, int inter, int nlayers, long vocab,
                             int max_pos, int type_vocab, float p_hidden, float p_attn, long seed, void* workspace, size_t ws_bytes,
                             hipStream_t s) {
  if (!dy || !ids || !key_mask || !params || !grads || !acts || !scratch || vocab <= 0 || !bert_dims_ok(nseq, L, heads, D, inter, nlayers))
    return HMMC_ERR_ARG;
  if (!(p_hidden >= 0.f) || !(p_hidden < 1.f) || !(p_attn >= 0.f) || !(p_attn < 1.f) || max_pos < L || type_vocab <= 0) return HMMC_ERR_ARG;
  if (L > MA_MAXL || D > 1024 || (inter & 3)) return HMMC_ERR_UNSUPPORTED;
  const long T = (long)nseq * L;
  if (T * std::max(3 * D, inter) > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  if (!workspace || ws_bytes < hmmc_bert_workspace_bytes(nseq, L, D, inter)) return HMMC_ERR_WORKSPACE;
  const bool adrop = p_attn > 0.f, hdrop = p_hidden > 0.f;
  const float* const* P = (const float* const*)params;
  float* const* G = (float* const*)grads;
  const EmbActs ea = carve_emb((char*)acts, T, D);
  char* const slabs = (char*)acts + ea.bytes;
  const size_t slab = carve_layer(nullptr, T, D, inter, nseq, L, heads, adrop).bytes;
  char* sp = (char*)scratch;
  float* td[6];
  for (auto& t : td) { t = (float*)sp; sp += al((size_t)T * D * 4); }
  float* const dA = td[0]; float* const dB = td[1]; float* const dC = td[2]; float* const dD = td[3];
  float* const dg = (float*)sp; sp += al((size_t)T * inter * 4);
  float* const dh = (float*)sp; sp += al((size_t)T * inter * 4);
  float* const dqkv = (float*)sp;
  const float* g_in = dy;
  for (int i = nlayers - 1; i >= 0; --i) {
    const float* const* W = P + BERT_EMB_PARAMS + (size_t)i * BERT_LAYER_PARAMS;
    float* const* GW = G + BERT_EMB_PARAMS + (size_t)i * BERT_LAYER_PARAMS;
    const LayerActs a = carve_layer(slabs + (size_t)i * slab, T, D, inter, nseq, L, heads, adrop);
    float* const g_out = td[4 + (i & 1)];
    // ---- out = LN(pre2), pre2 = dropout(g W_o^T + b_o) + x1: dA = d(pre2); without dropout its column sums are d(b_o)
    CK(hmmc_layernorm_bwd(g_in, a.pre2, W[14], a.m2, a.r2, nullptr, dA, GW[14], GW[15], hdrop ? nullptr : GW[13], nullptr, (int)T, D, D, 1,
                          workspace, ws_bytes, s));
    const float* da2 = dA;
    if (hdrop) {
      CK(hmmc_dropout_bwd(dA, dB, T * D, p_hidden, seed, 3 + 3 * i, s));
      CK(hmmc_colsum(dB, GW[13], (int)T, D, D, 1, 1, 0, workspace, ws_bytes, s));
      da2 = dB;
    }
    CK(wgrad(da2, a.g, GW[12], (int)T, D, inter, s));
    CK(dgrad(da2, W[12], dg, (int)T, D, inter, nullptr, s));
    CK(hmmc_gelu_erf_bwd(a.h, dg, dh, T * inter, s));
    CK(hmmc_colsum(dh, GW[11], (int)T, inter, inter, 1, 1, 0, workspace, ws_bytes, s));
    CK(wgrad(dh, a.x1, GW[10], (int)T, inter, D, s));
    CK(dgrad(dh, W[10], dC, (int)T, inter, D, dA, s));                  // d(x1): through intermediate.dense and the residual
    // ---- x1 = LN(pre1), pre1 = dropout(att W_ao^T + b_ao) + x: dD = d(pre1)
    CK(hmmc_layernorm_bwd(dC, a.pre1, W[8], a.m1, a.r1, nullptr, dD, GW[8], GW[9], hdrop ? nullptr : GW[7], nullptr, (int)T, D, D, 1,
                          workspace, ws_bytes, s));
    const float* da1 = dD;
    if (hdrop) {
      CK(hmmc_dropout_bwd(dD, dB, T * D, p_hidden, seed, 2 + 3 * i, s));
      CK(hmmc_colsum(dB, GW[7], (int)T, D, D, 1, 1, 0, workspace, ws_bytes, s));
      da1 = dB;
    }
    CK(wgrad(da1, a.att, GW[6], (int)T, D, D, s));
    CK(dgrad(da1, W[6], dA, (int)T, D, D, nullptr, s));                 // d(att)
    CK(hmmc_masked_attention_bwd(a.qkv, key_mask, a.probs, a.praw, dA, dqkv, nseq, L, heads, p_attn, seed, 1 + 3 * i, s));
    for (int j = 0; j < 3; ++j) {
      CK(hmmc_colsum(dqkv + (size_t)j * D, GW[2 * j + 1], (int)T, D, 3 * D, 1, 1, 0, workspace, ws_bytes, s));
      CK(wgrad(dqkv + (size_t)j * D, a.x, GW[2 * j], (int)T, D, D, s, 3 * D, 0));
    }
    // d(x) = dq W_q + dk W_k + dv W_v + d(pre1), added in this order
    CK(dgrad(dqkv, W[0], dC, (int)T, D, D, dD, s, 3 * D));
    CK(dgrad(dqkv + D, W[2], dA, (int)T, D, D, dC, s, 3 * D));
    CK(dgrad(dqkv + 2 * (size_t)D, W[4], g_out, (int)T, D, D, dA, s, 3 * D));
    g_in = g_out;
  }
  // ---- x0 = dropout(LN(e)): the embedding tables and the embedding LayerNorm
  const float* dx0 = g_in;
  if (hdrop) {
    CK(hmmc_dropout_bwd(g_in, dA, T * D, p_hidden, seed, 0, s));
    dx0 = dA;
  }
  return hmmc_bert_embed_bwd(ids, dx0, ea.e, P[3], ea.mean, ea.rstd, dB, G[0], G[1], G[2], G[3], G[4], T, L, D, vocab, max_pos, type_vocab,
                             workspace, ws_bytes, s);
}
