// What bert_tower.hip, the one runtime of the Chinese text branch, takes from the files that hold its two regimes' kernels
// (bert_f32.hip, bert_f16.hip) beyond the entry points of include/hmmc_hip.h.  Internal to the library: C++ linkage, no ABI.
#pragma once
#include "common.h"

constexpr int MATTN_F32_MAXL = 256, MATTN_F16_MAXL = 64;   // longest sequence of hmmc_masked_attention_fwd / _f16_fwd

// the pooler's tanh on n elements: y = tanh(y) in place; dz = dy (1 - y^2)
int bert_tanh_f32(float* y, long n, hipStream_t s);
int bert_tanh_bwd_f32(const float* dy, const float* y, float* dz, long n, hipStream_t s);
int bert_tanh_f16(void* y, long n, hipStream_t s);
int bert_tanh_bwd_f16(const void* dy, const void* y, void* dz, long n, hipStream_t s);
