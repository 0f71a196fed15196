// score.hip — scores of GIVEN target tokens under one model or a checkpoint ensemble (fairseq-generate --score-reference):
// the decoder's logits [B*T, V] of every member go in, one fp32 score per target position comes out; the float32 [B, T, V]
// log-probability tensor the reference builds per member (sequence_scorer.py:77-81 -> fairseq_decoder.py:58-79 -> utils.py:469-473)
// and gathers one column from (:54-59) is never materialised.  Replaces those call sites and the ensemble average (:96-111) and the
// per-sentence sums (:118-127).
//
// Per live row and member m:  lse_m = mx_m + log(sum_v exp(x_v - mx_m)) (the vocabulary maximum is taken out first),
// l_m = x_target - lse_m;  N = 1: pos = l_1;  N > 1: pos = M + log(sum_m exp(l_m - M)) - log N, M = max_m l_m.  All in fp32.
// One workgroup per target position; a pad position writes 0 and returns before it has formed a logits address.
// A row is read as: the (at most VEC - 1) elements in front of its first 16-byte boundary, 16-byte vectors, the elements behind the
// last whole vector — so any V, any row stride and any element-aligned base take the vector loads, and all sums have a fixed order.
#include "cst_common.h"

namespace {

struct ScoreMembers { const void* p[8]; };

__device__ __forceinline__ float score_block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float score_block_max(float v, float* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// hands f the elements of one row that this thread of 256 owns — a head element, whole vectors, a tail element, in that order
template <typename T, typename F>
__device__ __forceinline__ void score_row_visit(const T* x, int64_t V, F&& f) {
  constexpr int VEC = DT<T>::VEC;
  int64_t head = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(T));
  if (head > V) head = V;
  const int64_t nvec = (V - head) / VEC, tail0 = head + nvec * VEC;
  const int tid = threadIdx.x;
  if (tid < head) { float v[1] = {DT<T>::ld(x + tid)}; f(v); }
  const T* xv = x + head;
  for (int64_t i = tid; i < nvec; i += 256) {
    float v[VEC];
    ld_vec(xv + i * VEC, v);
    f(v);
  }
  if (tail0 + tid < V) { float v[1] = {DT<T>::ld(x + tail0 + tid)}; f(v); }
}

template <typename T>
__global__ __launch_bounds__(256) void score_tokens_kernel(ScoreMembers mem, int N, int64_t ld, const int64_t* target, int64_t pad,
                                                           float* pos, int64_t V, float logN) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const int64_t t = target[row];
  if (t == pad || t < 0 || t >= V) {  // (an id outside the vocabulary never gets here: kernels.score_tokens refuses it on the host)
    if (threadIdx.x == 0) pos[row] = t == pad ? 0.0f : NAN;
    return;
  }
  float l[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (m >= N) break;
    const T* x = (const T*)mem.p[m] + row * ld;
    float mx = -INFINITY;
    score_row_visit(x, V, [&](auto& v) {
#pragma unroll
      for (int e = 0; e < (int)(sizeof(v) / sizeof(float)); ++e) mx = fmaxf(mx, v[e]);
    });
    mx = score_block_max(mx, red);
    float se = 0.0f;
    score_row_visit(x, V, [&](auto& v) {  // second pass over a row this workgroup has just read
#pragma unroll
      for (int e = 0; e < (int)(sizeof(v) / sizeof(float)); ++e) se += __expf(v[e] - mx);
    });
    se = score_block_sum(se, red);
    l[m] = DT<T>::ld(x + t) - (mx + __logf(se));
  }
  if (threadIdx.x != 0) return;
  float p = l[0];
  if (N > 1) {
    float M = l[0];
#pragma unroll
    for (int m = 1; m < 8; ++m) if (m < N) M = fmaxf(M, l[m]);
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < 8; ++m) if (m < N) s += __expf(l[m] - M);
    p = M == -INFINITY ? -INFINITY : (M + __logf(s)) - logN;
  }
  pos[row] = p;
}

// score[b] = (sum of the non-pad pos[b, :]) / len[b]: per-thread partial sums in double over t = tid, tid + 256, ..., then a fixed LDS
// tree — the order of sum_pairs_kernel (loss_optim.hip), no atomics: bit-reproducible.  No target: 0 / 0 = NaN, as the reference.
__global__ __launch_bounds__(256) void score_sentences_kernel(const float* pos, const int64_t* target, int64_t pad, float* score,
                                                              int32_t* len, int64_t T) {
  __shared__ double red[256];
  __shared__ int cnt[256];
  const int64_t b = blockIdx.x;
  double a = 0.0;
  int n = 0;
  for (int64_t t = threadIdx.x; t < T; t += 256)
    if (target[b * T + t] != pad) { a += (double)pos[b * T + t]; ++n; }
  red[threadIdx.x] = a;
  cnt[threadIdx.x] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; cnt[threadIdx.x] += cnt[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    len[b] = cnt[0];
    score[b] = (float)red[0] / (float)cnt[0];
  }
}

}  // namespace

extern "C" int cst_score_tokens(const void* logits, const void* const* logits_n, int64_t members, int64_t ld, const int64_t* target,
                                int64_t pad, float* pos, float* score, int32_t* len, int64_t B, int64_t T, int64_t V, int dtype,
                                cst_stream stream) {
  CST_REQUIRE(logits && target && pos && score && len, "cst_score_tokens: null operand");
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_score_tokens: bad dtype %d", dtype);
  CST_REQUIRE(B > 0 && T > 0 && V > 0 && B * T <= INT32_MAX, "cst_score_tokens: bad shape B %lld T %lld V %lld", (long long)B, (long long)T, (long long)V);
  CST_REQUIRE(ld >= V, "cst_score_tokens: row stride %lld below the vocabulary %lld", (long long)ld, (long long)V);
  CST_REQUIRE(members >= 1 && members <= 8, "cst_score_tokens: %lld ensemble members (1 .. 8)", (long long)members);
  CST_REQUIRE(members == 1 || logits_n, "cst_score_tokens: members %lld without logits_n", (long long)members);
  ScoreMembers mem = {};
  mem.p[0] = logits;
  for (int m = 1; m < members; ++m) {
    CST_REQUIRE(logits_n[m - 1], "cst_score_tokens: the logits of member %d are missing", m);
    mem.p[m] = logits_n[m - 1];
  }
  for (int m = 0; m < members; ++m)
    CST_REQUIRE((uintptr_t)mem.p[m] % cst_dtype_size(dtype) == 0, "cst_score_tokens: the logits of member %d are not element-aligned", m);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = B * T;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)members * rows * V * cst_dtype_size(dtype));
  const float logN = (float)log((double)members);
  if (dtype == CST_BF16) hipLaunchKernelGGL(score_tokens_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, s, mem, (int)members, ld, target, pad, pos, V, logN);
  else hipLaunchKernelGGL(score_tokens_kernel<float>, dim3((unsigned)rows), dim3(256), 0, s, mem, (int)members, ld, target, pad, pos, V, logN);
  hipLaunchKernelGGL(score_sentences_kernel, dim3((unsigned)B), dim3(256), 0, s, (const float*)pos, target, pad, score, len, T);
  return cst_check_launch("cst_score_tokens");
}
