// The frames behind a gallery search hit (hmmc_amd/search.py, frames=True): for given (query, video) pairs, the k largest frame
// logits scale * q . u_f and their frame numbers - the terms of the mean-of-top-k that hmmc_eval_score adds to the video logit
// (reference main_task_retrieval.py:334-336 on the frame logits of modules/modeling.py:225-227) and then drops.
//
// A gather, not a GEMM: topn hits out of len(gallery) videos per query, (F + 1) * E * 4 bytes per pair (26 KiB at F = 12,
// E = 512) and two flops per four bytes, so the kernel is a matter of loads in flight.  One wave per pair.  A lane reads 16
// bytes per load, a wave 1 KiB of a row per instruction; the loads of HIT_ROWS rows are issued before the first sum; up to
// E = 512 the query row stays in two registers per lane quad.  Lane f ends up holding logit_f (F <= 31), its place in the
// output is the number of frames that precede it in (logit descending, f ascending), counted over F cross-lane reads.
#include "common.h"

namespace {

constexpr int HIT_ROWS = 4;        // rows of a video in flight per wave: 8 loads of 16 bytes per lane at E = 512
constexpr int HIT_QREG_VECS = 128; // E / 4 up to which the query row is held in registers (two 16-byte pieces per lane)

__device__ __forceinline__ float hit_dot4(f4 q, f4 x, float acc) {
  acc = __builtin_fmaf(q[0], x[0], acc);
  acc = __builtin_fmaf(q[1], x[1], acc);
  acc = __builtin_fmaf(q[2], x[2], acc);
  return __builtin_fmaf(q[3], x[3], acc);
}

__device__ __forceinline__ f4 pick(f4 a, f4 b, bool first) {
  return f4{first ? a[0] : b[0], first ? a[1] : b[1], first ? a[2] : b[2], first ? a[3] : b[3]};
}

// The order of every sum is the one include/hmmc_hip.h documents: per lane e = 256 j + 4 lane + c ascending by fma from 0 (a
// piece the row does not have is a piece of zeros, which leaves the sum as it is), then the xor butterfly of wave_sum.
template <bool QREG>
__global__ __launch_bounds__(256) void hit_frames_kernel(const float* __restrict__ queries, const float* __restrict__ packed,
                                                         const int* __restrict__ pair_query, const int* __restrict__ pair_video,
                                                         float* __restrict__ frame_score, int* __restrict__ frame_index,
                                                         float* __restrict__ video_logit, long pairs, int nq, int nv,
                                                         int video_base, int F, int P, int E, int k, float scale) {
  const int lane = threadIdx.x & 63;
  const int nvec = E >> 2;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  // Every load is unconditional, so that none waits behind a branch: a lane past the row's end reads the row's last piece and
  // a slot past F reads slot F again; the first is replaced by zeros after the load, the second is never looked at.
  const bool has[2] = {lane < nvec, lane + 64 < nvec};
  const int piece[2] = {has[0] ? lane : nvec - 1, has[1] ? lane + 64 : nvec - 1};
  for (long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6); m < pairs; m += (long)gridDim.x * 4) {
    const int q = pair_query[m];
    const long v = (long)pair_video[m] - video_base;
    if (q < 0 || q >= nq || v < 0 || v >= nv) continue;       // the same for the whole wave: not a pair of this chunk
    const f4* qr = reinterpret_cast<const f4*>(queries + (long)q * E);
    const f4* rows = reinterpret_cast<const f4*>(packed + v * P * E);   // slot s starts at rows + s * nvec
    f4 qreg[2];
    if (QREG) {
#pragma unroll
      for (int j = 0; j < 2; ++j) qreg[j] = pick(qr[piece[j]], zero, has[j]);
    }
    float mine = -INFINITY, video = 0.f;                       // lane f: logit of frame f
    for (int s0 = video_logit ? 0 : 1; s0 <= F; s0 += HIT_ROWS) {
      float acc[HIT_ROWS];
      if (QREG) {
        f4 x[HIT_ROWS][2];
#pragma unroll
        for (int r = 0; r < HIT_ROWS; ++r)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            x[r][j] = pick(rows[(long)min(s0 + r, F) * nvec + piece[j]], zero, has[j]);
#pragma unroll
        for (int r = 0; r < HIT_ROWS; ++r) acc[r] = hit_dot4(qreg[1], x[r][1], hit_dot4(qreg[0], x[r][0], 0.f));
      } else {
#pragma unroll
        for (int r = 0; r < HIT_ROWS; ++r) acc[r] = 0.f;
        for (int g = lane; g < nvec; g += 64) {
          const f4 qv = qr[g];
          f4 x[HIT_ROWS];
#pragma unroll
          for (int r = 0; r < HIT_ROWS; ++r) x[r] = rows[(long)min(s0 + r, F) * nvec + g];
#pragma unroll
          for (int r = 0; r < HIT_ROWS; ++r) acc[r] = hit_dot4(qv, x[r], acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < HIT_ROWS; ++r) {
        const float t = scale * wave_sum(acc[r]);
        const int s = s0 + r;
        if (s == 0) video = t;
        else if (s <= F && lane == s - 1) mine = t;
      }
    }
    if (!(mine == mine)) mine = -INFINITY;                     // NaN counts as -inf
    if (mine == 0.f) mine = 0.f;                               // -0 and +0 are one logit
    int rank = 0;
    for (int g = 0; g < F; ++g) {
      const float other = __shfl(mine, g, 64);
      rank += (other > mine || (other == mine && g < lane)) ? 1 : 0;
    }
    if (lane < F && rank < k) {
      frame_score[m * k + rank] = mine;
      frame_index[m * k + rank] = lane;
    }
    if (video_logit && lane == 0) video_logit[m] = video;
  }
}

}  // namespace

extern "C" int hmmc_hit_frames(const float* queries_unit, const float* packed, const int* pair_query, const int* pair_video,
                               float* frame_score, int* frame_index, float* video_logit, long pairs, int nq, int nv,
                               int video_base, int F, int E, int k, float scale, hipStream_t stream) {
  const int P = hmmc_eval_slots(F);
  if (!queries_unit || !packed || !pair_query || !pair_video || !frame_score || !frame_index || pairs < 0 || nq < 0 || nv < 0 ||
      F <= 0 || E <= 0 || k < 1 || k > F)
    return HMMC_ERR_ARG;
  if (!P || (E & 3) || (((uintptr_t)queries_unit | (uintptr_t)packed) & 15)) return HMMC_ERR_UNSUPPORTED;
  if (pairs == 0) return HMMC_OK;
  // a wave per pair, four to a workgroup; past 64 workgroups per compute unit the waves stride over the pairs
  const long want = (pairs + 3) / 4, cap = (long)hmmc_num_cus() * 64;
  const dim3 grid((unsigned)(want < cap ? want : cap));
  auto kernel = (E >> 2) <= HIT_QREG_VECS ? hit_frames_kernel<true> : hit_frames_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, queries_unit, packed, pair_query, pair_video, frame_score, frame_index,
                     video_logit, pairs, nq, nv, video_base, F, P, E, k, scale);
  return hmmc_launch_status();
}
