// The three GEMM calls of a linear layer, for the files that sequence kernels (tower.hip, bert_tower.hip): one spelling for the
// fp16 regime (hmmc_gemm_f16) and the fp32 one (hmmc_gemm_f32).  Row strides are in elements, 0 = dense; an fp16 stride fits an int
// (the callers check).  bias / resid switch their epilogue flags on; `epi` adds the others (the towers' QuickGELU forms).
#pragma once
#include "common.h"

// y[M,N] = x[M,K] w[N,K]^T (+ bias) (+ resid);  lda / ldc: row strides of x and of y
inline int linear(bool f32, const void* x, const void* w, void* y, int M, int N, int K, const void* bias, const void* resid,
                  void* aux_out, int epi, hipStream_t s, long lda = 0, int ldc = 0) {
  lda = lda ? lda : K;
  ldc = ldc ? ldc : N;
  epi |= (bias ? EPI_BIAS : 0) | (resid ? EPI_RESID : 0);
  if (f32)
    return hmmc_gemm_f32((const float*)x, (const float*)w, (float*)y, M, N, K, lda, 1, 1, K, ldc, 1.0f, (const float*)bias,
                         (const float*)resid, (float*)aux_out, nullptr, epi, s);
  return hmmc_gemm_f16(x, w, y, M, N, K, (int)lda, K, ldc, 1, 1, bias, resid, aux_out, nullptr, epi, nullptr, 0, s);
}
// dx[M,K'] = dy[M,N'] w[N',K'] (+ resid);  ldy / ldx: row strides of dy and dx
// csum (fp16 only): fp32 partial column sums of dx, hmmc_gemm_f16_colsum_rows(M, K', N') rows of K' floats
inline int dgrad(bool f32, const void* dy, const void* w, void* dx, int M, int Np, int Kp, const void* resid, const void* aux_in,
                 int epi, hipStream_t s, long ldy = 0, int ldx = 0, float* csum = nullptr, size_t csum_bytes = 0) {
  ldy = ldy ? ldy : Np;
  ldx = ldx ? ldx : Kp;
  epi |= resid ? EPI_RESID : 0;
  if (f32)
    return hmmc_gemm_f32((const float*)dy, (const float*)w, (float*)dx, M, Kp, Np, ldy, 1, Kp, 1, ldx, 1.0f, nullptr,
                         (const float*)resid, nullptr, (const float*)aux_in, epi, s);
  return hmmc_gemm_f16(dy, w, dx, M, Kp, Np, (int)ldy, Kp, ldx, 1, 0, nullptr, resid, nullptr, aux_in, epi | (csum ? EPI_COLSUM : 0),
                       csum, csum_bytes, s);
}
// dW[N',K'] = dy[T,N']^T x[T,K'];  ldy / ldx: row strides of dy and x.  fp16: split over T where the workspace allows; fp32 takes
// none.  Both regimes honour the strides: the fp32 CLIP tower never passes one that differs from the dense default (only the last
// block of a lead_only call does, and hmmc_tower_fwd / hmmc_tower_bwd refuse lead_only for an fp32 tower).
inline int wgrad(bool f32, const void* dy, const void* x, void* dw, int T, int Np, int Kp, void* ws, size_t wsb, hipStream_t s,
                 long ldy = 0, long ldx = 0) {
  ldy = ldy ? ldy : Np;
  ldx = ldx ? ldx : Kp;
  if (f32)
    return hmmc_gemm_f32((const float*)dy, (const float*)x, (float*)dw, Np, Kp, T, 1, ldy, ldx, 1, Kp, 1.0f, nullptr, nullptr,
                         nullptr, nullptr, 0, s);
  const size_t need = hmmc_gemm_f16_workspace(Np, Kp, T);
  return hmmc_gemm_f16(dy, x, dw, Np, Kp, T, (int)ldy, (int)ldx, Kp, 0, 0, nullptr, nullptr, nullptr, nullptr, 0,
                       need <= wsb ? ws : nullptr, need <= wsb ? wsb : 0, s);
}
