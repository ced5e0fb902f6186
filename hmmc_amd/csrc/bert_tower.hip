// The runtime of the Chinese text branch (reference modules/module_cross.py:257-265,273-277: HuggingFace BertModel): one C call
// runs the embedding and every post-LN BertLayer, forward or backward, and one the tanh pooler, in tower.hip's idiom - `f32`
// selects the regime, activations are addressed through char* and an element size.  It only SEQUENCES kernels of this library on
// the caller's stream (20 launches per layer forward, 30 backward); the kernels themselves and what each regime rounds are in
// bert_f32.hip (everything fp32) and bert_f16.hip (its header lists the rounding points).  All memory is caller-owned:
//   params  : 5 embedding pointers (word, position, token type, LayerNorm w, b), then per layer 16 (query w, b, key w, b, value w, b,
//             attention.output.dense w, b, its LayerNorm w, b, intermediate.dense w, b, output.dense w, b, its LayerNorm w, b)
//   acts    : hmmc_bert_act_bytes() / hmmc_bert_f16_act_bytes(); layout below
//   scratch : hmmc_bert_bwd_scratch_bytes() / hmmc_bert_f16_bwd_scratch_bytes() for the backward's transient gradients
//   grads   : as params, written (not accumulated)
#include "bert_regime.h"
#include "gemm_seq.h"
#include "philox.h"
#include <algorithm>

namespace {

constexpr int BERT_EMB_PARAMS = 5, BERT_LAYER_PARAMS = 16;

// activation layout: the embedding's fp32 rows (pre-LayerNorm e, statistics; fp16 regime: x0, the LayerNorm's output before the
// one cast), then one slab per layer (keep_acts) or one slab that every layer reuses.  es = element size: 4 fp32, 2 fp16.
struct EmbActs { float *e, *mean, *rstd, *x0; size_t bytes; };
struct LayerActs {
  char *x, *qkv, *att, *pre1, *x1, *h, *g, *pre2;
  float *probs, *praw, *lse;             // attention statistics: probs (+ praw with attention dropout) fp32 regime, lse fp16 regime
  float *m1, *r1, *m2, *r2;
  size_t bytes;
};
EmbActs carve_emb(bool f32, char* base, long T, int D) {
  EmbActs a{};
  char* p = base;
  a.e = (float*)p; p += al((size_t)T * D * 4);
  a.mean = (float*)p; p += al((size_t)T * 4);
  a.rstd = (float*)p; p += al((size_t)T * 4);
  if (!f32) { a.x0 = (float*)p; p += al((size_t)T * D * 4); }
  a.bytes = (size_t)(p - base);
  return a;
}
LayerActs carve_layer(bool f32, char* base, long T, int D, int I, int nseq, int L, int H, bool attn_drop) {
  LayerActs a{};
  const size_t es = f32 ? 4 : 2;
  const size_t td = al((size_t)T * D * es), ti = al((size_t)T * I * es), pp = al((size_t)nseq * H * L * L * 4), tr = al((size_t)T * 4);
  char* p = base;
  a.x = p; p += td;
  a.qkv = p; p += al((size_t)T * 3 * D * es);
  if (f32) {
    a.probs = (float*)p; p += pp;
    if (attn_drop) { a.praw = (float*)p; p += pp; }
  }
  a.att = p; p += td;
  a.pre1 = p; p += td;
  a.x1 = p; p += td;
  a.h = p; p += ti;
  a.g = p; p += ti;
  a.pre2 = p; p += td;
  if (!f32) { a.lse = (float*)p; p += al((size_t)T * H * 4); }
  a.m1 = (float*)p; p += tr;
  a.r1 = (float*)p; p += tr;
  a.m2 = (float*)p; p += tr;
  a.r2 = (float*)p; p += tr;
  a.bytes = (size_t)(p - base);
  return a;
}

// HMMC_OK, or why the regime does not take the shape (checked before any launch)
int bert_shape(bool f32, int nseq, int L, int heads, int D, int inter, int nlayers) {
  if (nseq <= 0 || L <= 0 || heads <= 0 || nlayers <= 0 || inter <= 0 || D != heads * 64) return HMMC_ERR_ARG;
  // fp16: a k-major GEMM operand takes whole 64-wide K tiles
  if (L > (f32 ? MATTN_F32_MAXL : MATTN_F16_MAXL) || D > 1024 || (inter & (f32 ? 3 : 63))) return HMMC_ERR_UNSUPPORTED;
  if ((long)nseq * L * std::max(3 * D, inter) > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  return HMMC_OK;
}

size_t act_bytes(bool f32, int nseq, int L, int heads, int D, int inter, int nlayers, int keep_acts, bool attn_drop) {
  const long T = (long)nseq * L;
  return carve_emb(f32, nullptr, T, D).bytes +
         carve_layer(f32, nullptr, T, D, inter, nseq, L, heads, attn_drop).bytes * (size_t)(keep_acts ? nlayers : 1);
}
// transient gradients of the backward: six [T, D], two [T, inter], one [T, 3D]; fp16 regime: and two fp32 [T, D] for the embedding
size_t bwd_scratch_bytes(bool f32, int nseq, int L, int D, int inter) {
  const long T = (long)nseq * L;
  const size_t es = f32 ? 4 : 2;
  return 6 * al((size_t)T * D * es) + 2 * al((size_t)T * inter * es) + al((size_t)T * 3 * D * es) + (f32 ? 0 : 2 * al((size_t)T * D * 4));
}
size_t workspace_bytes(bool f32, int nseq, int L, int D, int inter) {
  const int T = nseq * L;
  size_t w = std::max(hmmc_layernorm_bwd_workspace(T, D), hmmc_colsum_workspace(T, inter));
  w = std::max(w, hmmc_colsum_workspace(T, D));
  w = std::max(w, hmmc_bert_embed_bwd_workspace(T, L, D));
  const int NK[3][2] = {{D, D}, {D, inter}, {inter, D}};           // the split-K slabs of the fp16 weight gradients
  if (!f32)
    for (const auto& nk : NK) w = std::max(w, hmmc_gemm_f16_workspace(nk[0], nk[1], T));
  return al(w);
}

inline int dropout(bool f32, const void* x, const void* resid, void* y, long n, float p, long seed, int site, hipStream_t s) {
  return f32 ? hmmc_dropout_fwd((const float*)x, (const float*)resid, (float*)y, n, p, seed, site, s)
             : hmmc_dropout_f16_fwd(x, resid, y, n, p, seed, site, s);
}

int bert_fwd(bool f32, const long* ids, const long* key_mask, void* y, const void* const* params, void* acts, int keep_acts, int nseq,
             int L, int heads, int D, int inter, int nlayers, long vocab, float eps, float p_hidden, float p_attn, long seed,
             int* err_flag, hipStream_t s) {
  if (!ids || !key_mask || !y || !params || !acts || vocab <= 0 || !drop_p_ok(p_hidden) || !drop_p_ok(p_attn)) return HMMC_ERR_ARG;
  CK(bert_shape(f32, nseq, L, heads, D, inter, nlayers));
  const long T = (long)nseq * L;
  const size_t es = f32 ? 4 : 2;
  const int dt = f32 ? 1 : 0;
  const bool adrop = p_attn > 0.f;
  const EmbActs ea = carve_emb(f32, (char*)acts, T, D);
  char* const slabs = (char*)acts + ea.bytes;
  const size_t slab = carve_layer(f32, nullptr, T, D, inter, nseq, L, heads, adrop).bytes;
  auto layer_acts = [&](int i) { return carve_layer(f32, slabs + (size_t)i * slab, T, D, inter, nseq, L, heads, adrop); };
  LayerActs a = layer_acts(0);
  // x0 = dropout(LN(word + pos + type 0)), fp32 kernels: straight into the first slab's input, or (fp16 regime) followed by one cast
  const float* const* E = (const float* const*)params;
  float* const x0 = f32 ? (float*)a.x : ea.x0;
  CK(hmmc_bert_embed_fwd(ids, E[0], E[1], E[2], E[3], E[4], keep_acts ? ea.e : nullptr, x0, ea.mean, ea.rstd, T, L, D, vocab, eps,
                         err_flag, s));
  CK(hmmc_dropout_fwd(x0, nullptr, x0, T * D, p_hidden, seed, 0, s));
  if (!f32) CK(hmmc_cast(x0, a.x, T * D, 1, s));
  for (int i = 0; i < nlayers; ++i) {
    const void* const* W = params + BERT_EMB_PARAMS + (size_t)i * BERT_LAYER_PARAMS;
    if (keep_acts) a = layer_acts(i);
    // the layer's output: the next slab's input, y for the last layer; without kept activations the one slab's input slot,
    // which is dead once attention.output.dense (or its dropout) has read it as the residual
    void* out = i + 1 == nlayers ? y : keep_acts ? layer_acts(i + 1).x : a.x;
    for (int j = 0; j < 3; ++j)                                    // query | key | value into one [T, 3D] buffer
      CK(linear(f32, a.x, W[2 * j], a.qkv + (size_t)j * D * es, (int)T, D, D, W[2 * j + 1], nullptr, nullptr, 0, s, 0, 3 * D));
    if (f32) CK(hmmc_masked_attention_fwd((const float*)a.qkv, key_mask, (float*)a.att, a.probs, a.praw, nseq, L, heads, p_attn, seed, 1 + 3 * i, s));
    else CK(hmmc_masked_attention_f16_fwd(a.qkv, key_mask, a.att, a.lse, nseq, L, heads, p_attn, seed, 1 + 3 * i, s));
    if (p_hidden > 0.f) {
      CK(linear(f32, a.att, W[6], a.pre1, (int)T, D, D, W[7], nullptr, nullptr, 0, s));
      CK(dropout(f32, a.pre1, a.x, a.pre1, T * D, p_hidden, seed, 2 + 3 * i, s));
    } else {
      CK(linear(f32, a.att, W[6], a.pre1, (int)T, D, D, W[7], a.x, nullptr, 0, s));
    }
    CK(hmmc_layernorm_fwd(a.pre1, (const float*)W[8], (const float*)W[9], a.x1, a.m1, a.r1, nullptr, (int)T, D, D, eps, dt, s));
    CK(linear(f32, a.x1, W[10], a.h, (int)T, inter, D, W[11], nullptr, nullptr, 0, s));
    if (f32) CK(hmmc_gelu_erf_fwd((const float*)a.h, (float*)a.g, T * inter, s));
    else CK(hmmc_gelu_erf_f16_fwd(a.h, a.g, T * inter, s));
    if (p_hidden > 0.f) {
      CK(linear(f32, a.g, W[12], a.pre2, (int)T, D, inter, W[13], nullptr, nullptr, 0, s));
      CK(dropout(f32, a.pre2, a.x1, a.pre2, T * D, p_hidden, seed, 3 + 3 * i, s));
    } else {
      CK(linear(f32, a.g, W[12], a.pre2, (int)T, D, inter, W[13], a.x1, nullptr, 0, s));
    }
    CK(hmmc_layernorm_fwd(a.pre2, (const float*)W[14], (const float*)W[15], out, a.m2, a.r2, nullptr, (int)T, D, D, eps, dt, s));
  }
  return HMMC_OK;
}

int bert_bwd(bool f32, const void* dy, const long* ids, const long* key_mask, const void* const* params, void* const* grads,
             const void* acts, void* scratch, int nseq, int L, int heads, int D, int inter, int nlayers, long vocab, int max_pos,
             int type_vocab, float p_hidden, float p_attn, long seed, void* workspace, size_t ws_bytes, hipStream_t s) {
  if (!dy || !ids || !key_mask || !params || !grads || !acts || !scratch || vocab <= 0 || !drop_p_ok(p_hidden) || !drop_p_ok(p_attn) ||
      max_pos < L || type_vocab <= 0)
    return HMMC_ERR_ARG;
  CK(bert_shape(f32, nseq, L, heads, D, inter, nlayers));
  if (!workspace || ws_bytes < workspace_bytes(f32, nseq, L, D, inter)) return HMMC_ERR_WORKSPACE;
  const long T = (long)nseq * L;
  const size_t es = f32 ? 4 : 2;
  const int dt = f32 ? 1 : 0;
  const bool adrop = p_attn > 0.f, hdrop = p_hidden > 0.f;
  const EmbActs ea = carve_emb(f32, (char*)acts, T, D);
  char* const slabs = (char*)acts + ea.bytes;
  const size_t slab = carve_layer(f32, nullptr, T, D, inter, nseq, L, heads, adrop).bytes;
  char* sp = (char*)scratch;
  char* td[6];
  for (auto& t : td) { t = sp; sp += al((size_t)T * D * es); }
  char* const dA = td[0]; char* const dB = td[1]; char* const dC = td[2]; char* const dD = td[3];
  char* const dg = sp; sp += al((size_t)T * inter * es);
  char* const dh = sp; sp += al((size_t)T * inter * es);
  char* const dqkv = sp; sp += al((size_t)T * 3 * D * es);
  const void* g_in = dy;
  for (int i = nlayers - 1; i >= 0; --i) {
    const void* const* W = params + BERT_EMB_PARAMS + (size_t)i * BERT_LAYER_PARAMS;
    void* const* GW = grads + BERT_EMB_PARAMS + (size_t)i * BERT_LAYER_PARAMS;
    const LayerActs a = carve_layer(f32, slabs + (size_t)i * slab, T, D, inter, nseq, L, heads, adrop);
    char* const g_out = td[4 + (i & 1)];
    // ---- out = LN(pre2), pre2 = dropout(g W_o^T + b_o) + x1: dA = d(pre2); without dropout its column sums are d(b_o)
    CK(hmmc_layernorm_bwd(g_in, a.pre2, (const float*)W[14], a.m2, a.r2, nullptr, dA, (float*)GW[14], (float*)GW[15],
                          hdrop ? nullptr : GW[13], nullptr, (int)T, D, D, dt, workspace, ws_bytes, s));
    const char* da2 = dA;
    if (hdrop) {
      CK(dropout(f32, dA, nullptr, dB, T * D, p_hidden, seed, 3 + 3 * i, s));
      CK(hmmc_colsum(dB, GW[13], (int)T, D, D, dt, dt, 0, workspace, ws_bytes, s));
      da2 = dB;
    }
    CK(wgrad(f32, da2, a.g, GW[12], (int)T, D, inter, workspace, ws_bytes, s));
    CK(dgrad(f32, da2, W[12], dg, (int)T, D, inter, nullptr, nullptr, 0, s));
    if (f32) CK(hmmc_gelu_erf_bwd((const float*)a.h, (const float*)dg, (float*)dh, T * inter, s));
    else CK(hmmc_gelu_erf_f16_bwd(a.h, dg, dh, T * inter, s));
    CK(hmmc_colsum(dh, GW[11], (int)T, inter, inter, dt, dt, 0, workspace, ws_bytes, s));
    CK(wgrad(f32, dh, a.x1, GW[10], (int)T, inter, D, workspace, ws_bytes, s));
    CK(dgrad(f32, dh, W[10], dC, (int)T, inter, D, dA, nullptr, 0, s));       // d(x1): through intermediate.dense and the residual
    // ---- x1 = LN(pre1), pre1 = dropout(att W_ao^T + b_ao) + x: dD = d(pre1)
    CK(hmmc_layernorm_bwd(dC, a.pre1, (const float*)W[8], a.m1, a.r1, nullptr, dD, (float*)GW[8], (float*)GW[9],
                          hdrop ? nullptr : GW[7], nullptr, (int)T, D, D, dt, workspace, ws_bytes, s));
    const char* da1 = dD;
    if (hdrop) {
      CK(dropout(f32, dD, nullptr, dB, T * D, p_hidden, seed, 2 + 3 * i, s));
      CK(hmmc_colsum(dB, GW[7], (int)T, D, D, dt, dt, 0, workspace, ws_bytes, s));
      da1 = dB;
    }
    CK(wgrad(f32, da1, a.att, GW[6], (int)T, D, D, workspace, ws_bytes, s));
    CK(dgrad(f32, da1, W[6], dA, (int)T, D, D, nullptr, nullptr, 0, s));      // d(att)
    if (f32)
      CK(hmmc_masked_attention_bwd((const float*)a.qkv, key_mask, a.probs, a.praw, (const float*)dA, (float*)dqkv, nseq, L, heads, p_attn,
                                   seed, 1 + 3 * i, s));
    else
      CK(hmmc_masked_attention_f16_bwd(a.qkv, key_mask, a.lse, dA, dqkv, nullptr, nseq, L, heads, p_attn, seed, 1 + 3 * i, s));
    for (int j = 0; j < 3; ++j) {
      CK(hmmc_colsum(dqkv + (size_t)j * D * es, GW[2 * j + 1], (int)T, D, 3 * D, dt, dt, 0, workspace, ws_bytes, s));
      CK(wgrad(f32, dqkv + (size_t)j * D * es, a.x, GW[2 * j], (int)T, D, D, workspace, ws_bytes, s, 3 * D, 0));
    }
    // d(x) = dq W_q + dk W_k + dv W_v + d(pre1), added in this order
    CK(dgrad(f32, dqkv, W[0], dC, (int)T, D, D, dD, nullptr, 0, s, 3 * D));
    CK(dgrad(f32, dqkv + (size_t)D * es, W[2], dA, (int)T, D, D, dC, nullptr, 0, s, 3 * D));
    CK(dgrad(f32, dqkv + 2 * (size_t)D * es, W[4], g_out, (int)T, D, D, dA, nullptr, 0, s, 3 * D));
    g_in = g_out;
  }
  // ---- x0 = dropout(LN(e)): the embedding tables and the embedding LayerNorm, fp32 in both regimes.  The site-0 dropout: fp32
  // regime into dA (none without dropout), de in dB; fp16 regime back to fp32 first, in place there, de in the second fp32 buffer
  const float* dx0 = (const float*)g_in;
  float* de = (float*)dB;
  if (!f32) {
    float* const g32 = (float*)sp;
    de = (float*)(sp + al((size_t)T * D * 4));
    CK(hmmc_cast(g_in, g32, T * D, 0, s));
    CK(hmmc_dropout_bwd(g32, g32, T * D, p_hidden, seed, 0, s));
    dx0 = g32;
  } else if (hdrop) {
    CK(hmmc_dropout_bwd(dx0, (float*)dA, T * D, p_hidden, seed, 0, s));
    dx0 = (const float*)dA;
  }
  const float* const* E = (const float* const*)params;
  float* const* G = (float* const*)grads;
  return hmmc_bert_embed_bwd(ids, dx0, ea.e, E[3], ea.mean, ea.rstd, de, G[0], G[1], G[2], G[3], G[4], T, L, D, vocab, max_pos, type_vocab,
                             workspace, ws_bytes, s);
}

// BertPooler on the class rows, addressed in place at `stride`: y = tanh(x W^T + bias)
int pooler_fwd(bool f32, const void* x, const void* W, const void* bias, void* y, int b, long stride, int D, hipStream_t s) {
  if (!x || !W || !bias || !y || b <= 0 || D <= 0 || stride < D) return HMMC_ERR_ARG;
  if (!f32 && stride > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  CK(linear(f32, x, W, y, b, D, D, bias, nullptr, nullptr, 0, s, stride, 0));
  return f32 ? bert_tanh_f32((float*)y, (long)b * D, s) : bert_tanh_f16(y, (long)b * D, s);
}
// only the fp16 pooler checks (and has a query for) its workspace
int pooler_bwd(bool f32, const void* dy, const void* y, const void* x, const void* W, void* dz, void* dx, void* dW, void* db, int b,
               long stride, int D, void* workspace, size_t ws_bytes, hipStream_t s) {
  if (!dy || !y || !x || !W || !dz || !dx || !dW || !db || b <= 0 || D <= 0 || stride < D) return HMMC_ERR_ARG;
  if (stride > 0x7fffffffL) return HMMC_ERR_UNSUPPORTED;
  if (!f32 && (!workspace || ws_bytes < hmmc_bert_pooler_f16_bwd_workspace(b, D))) return HMMC_ERR_WORKSPACE;
  const int dt = f32 ? 1 : 0;
  CK(f32 ? bert_tanh_bwd_f32((const float*)dy, (const float*)y, (float*)dz, (long)b * D, s) : bert_tanh_bwd_f16(dy, y, dz, (long)b * D, s));
  CK(hmmc_colsum(dz, db, b, D, D, dt, dt, 0, workspace, ws_bytes, s));
  CK(wgrad(f32, dz, x, dW, b, D, D, workspace, ws_bytes, s, 0, stride));
  return dgrad(f32, dz, W, dx, b, D, D, nullptr, nullptr, 0, s, 0, (int)stride);
}

}  // namespace

// ---------------------------------------------------------------- the entry points of both regimes (include/hmmc_hip.h)
extern "C" size_t hmmc_bert_act_bytes(int nseq, int L, int heads, int D, int inter, int nlayers, int keep_acts, int attn_dropout) {
  return act_bytes(true, nseq, L, heads, D, inter, nlayers, keep_acts, attn_dropout != 0);
}
extern "C" size_t hmmc_bert_f16_act_bytes(int nseq, int L, int heads, int D, int inter, int nlayers, int keep_acts) {
  return act_bytes(false, nseq, L, heads, D, inter, nlayers, keep_acts, false);
}
extern "C" size_t hmmc_bert_bwd_scratch_bytes(int nseq, int L, int D, int inter) { return bwd_scratch_bytes(true, nseq, L, D, inter); }
extern "C" size_t hmmc_bert_f16_bwd_scratch_bytes(int nseq, int L, int D, int inter) { return bwd_scratch_bytes(false, nseq, L, D, inter); }
extern "C" size_t hmmc_bert_workspace_bytes(int nseq, int L, int D, int inter) { return workspace_bytes(true, nseq, L, D, inter); }
extern "C" size_t hmmc_bert_f16_workspace_bytes(int nseq, int L, int D, int inter) {
  if (nseq <= 0 || L <= 0 || D <= 0 || inter <= 0 || (long)nseq * L * std::max(3 * D, inter) > 0x7fffffffL) return 0;   // shapes the tower refuses
  return workspace_bytes(false, nseq, L, D, inter);
}

extern "C" int hmmc_bert_fwd(const long* ids, const long* key_mask, float* y, const void* const* params, void* acts, int keep_acts,
                             int nseq, int L, int heads, int D, int inter, int nlayers, long vocab, float eps, float p_hidden,
                             float p_attn, long seed, int* err_flag, hipStream_t s) {
  return bert_fwd(true, ids, key_mask, y, params, acts, keep_acts, nseq, L, heads, D, inter, nlayers, vocab, eps, p_hidden, p_attn, seed,
                  err_flag, s);
}
extern "C" int hmmc_bert_f16_fwd(const long* ids, const long* key_mask, void* y, const void* const* params, void* acts, int keep_acts,
                                 int nseq, int L, int heads, int D, int inter, int nlayers, long vocab, float eps, float p_hidden,
                                 float p_attn, long seed, int* err_flag, hipStream_t s) {
  return bert_fwd(false, ids, key_mask, y, params, acts, keep_acts, nseq, L, heads, D, inter, nlayers, vocab, eps, p_hidden, p_attn, seed,
                  err_flag, s);
}
extern "C" int hmmc_bert_bwd(const float* dy, const long* ids, const long* key_mask, const void* const* params, void* const* grads,
                             const void* acts, void* scratch, int nseq, int L, int heads, int D, int inter, int nlayers, long vocab,
                             int max_pos, int type_vocab, float p_hidden, float p_attn, long seed, void* workspace, size_t ws_bytes,
                             hipStream_t s) {
  return bert_bwd(true, dy, ids, key_mask, params, grads, acts, scratch, nseq, L, heads, D, inter, nlayers, vocab, max_pos, type_vocab,
                  p_hidden, p_attn, seed, workspace, ws_bytes, s);
}
extern "C" int hmmc_bert_f16_bwd(const void* dy, const long* ids, const long* key_mask, const void* const* params, void* const* grads,
                                 const void* acts, void* scratch, int nseq, int L, int heads, int D, int inter, int nlayers,
                                 long vocab, int max_pos, int type_vocab, float p_hidden, float p_attn, long seed, void* workspace,
                                 size_t ws_bytes, hipStream_t s) {
  return bert_bwd(false, dy, ids, key_mask, params, grads, acts, scratch, nseq, L, heads, D, inter, nlayers, vocab, max_pos, type_vocab,
                  p_hidden, p_attn, seed, workspace, ws_bytes, s);
}

extern "C" int hmmc_bert_pooler_fwd(const float* x, const float* W, const float* bias, float* y, int b, long stride, int D,
                                    hipStream_t stream) {
  return pooler_fwd(true, x, W, bias, y, b, stride, D, stream);
}
extern "C" int hmmc_bert_pooler_f16_fwd(const void* x, const void* W, const void* bias, void* y, int b, long stride, int D,
                                        hipStream_t stream) {
  return pooler_fwd(false, x, W, bias, y, b, stride, D, stream);
}
extern "C" size_t hmmc_bert_pooler_f16_bwd_workspace(int b, int D) {
  return al(std::max(hmmc_colsum_workspace(b, D), hmmc_gemm_f16_workspace(D, D, b)));
}
extern "C" int hmmc_bert_pooler_bwd(const float* dy, const float* y, const float* x, const float* W, float* dz, float* dx, float* dW,
                                    float* db, int b, long stride, int D, void* workspace, size_t ws_bytes, hipStream_t stream) {
  return pooler_bwd(true, dy, y, x, W, dz, dx, dW, db, b, stride, D, workspace, ws_bytes, stream);
}
extern "C" int hmmc_bert_pooler_f16_bwd(const void* dy, const void* y, const void* x, const void* W, void* dz, void* dx, void* dW,
                                        void* db, int b, long stride, int D, void* workspace, size_t ws_bytes, hipStream_t stream) {
  return pooler_bwd(false, dy, y, x, W, dz, dx, dW, db, b, stride, D, workspace, ws_bytes, stream);
}
