// ctc.hip — connectionist temporal classification on raw logits (criterion `ctc`, fine-tuning wav2vec2 on transcripts):
//   cst_ctc_fwd    : loss and per-utterance nll — replaces log_softmax(logits.float()) + F.ctc_loss (criterions/ctc.py:97-113)
//   cst_ctc_bwd    : d loss / d logits, fused with the log-softmax backward (the autograd of those two calls)
//   cst_ctc_greedy : best-path decode on the device (the host loop of criterions/ctc.py:116-160)
// No fp32 [T, B, V] log-probability tensor exists on either pass: a row-parallel phase reduces each live frame to its log-sum-exp and
// to the S = 2 L + 1 log-probabilities of the extended label sequence (blank, l1, blank, ..., blank), a serial phase runs the
// recursions over that strip.  Everything is fp32 with libm-accuracy expf / logf (tests/ctc_ref.py counts their roundings).
//
// Phases of cst_ctc_fwd:
//   rows   one workgroup per live frame (t, b): mx = max_v x, lse = mx + log(sum_v exp(x_v - mx)), emit[b][t][s] = x[l'_s] - lse.
//          Elements are owned by their LOGICAL index: group g = v / VEC belongs to thread g % NT, and its elements are added in index
//          order — a 16-byte load where the row base is 16-byte aligned, VEC scalar loads of the same elements where it is not.  The
//          order of every sum is therefore independent of the row's alignment: a time-major view of batch-major memory and its
//          contiguous copy give equal bits (the head / vectors / tail split of score.hip would not).
//   alpha, beta   one workgroup per utterance and direction (blockIdx.y), both in ONE launch: they read only the strip.
//          State s lives in thread s % NT; the previous time step's variables live in a double-buffered LDS strip with two -inf pad
//          cells on each side, so one barrier per time step orders everything.  The next step's emissions are loaded before the
//          barrier (they do not depend on the recursion).  alpha_t(s) and beta_t(s) both INCLUDE the emission at t (torch's convention).
//   sum    one workgroup adds nll[0 .. B) in a fixed tree, in double.
// No float atomics anywhere: loss, nll and gradients are bit-reproducible, and an utterance's numbers do not depend on its batch.
#include "cst_common.h"

#define CTC_L_MAX 2047                   // longest padded target: S = 4095 states
#define CTC_S_MAX (2 * CTC_L_MAX + 1)

namespace {

template <int NT>
__device__ __forceinline__ float ctc_block_sum(float v, float* red) {
  v = wave_sum(v);
  if constexpr (NT == 64) return v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float a = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) a += red[w];
  return a;
}
template <int NT>
__device__ __forceinline__ float ctc_block_max(float v, float* red) {
  v = wave_max(v);
  if constexpr (NT == 64) return v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float a = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) a = fmaxf(a, red[w]);
  return a;
}

// hands f(v, n, v0) the groups of VEC consecutive elements this thread owns: n live values v[0 .. n) at element index v0
template <typename T, int NT, typename F>
__device__ __forceinline__ void ctc_row_visit(const T* x, int64_t V, F&& f) {
  constexpr int VEC = DT<T>::VEC;
  const bool aligned = ((uintptr_t)x & 15) == 0;
  for (int64_t v0 = (int64_t)threadIdx.x * VEC; v0 < V; v0 += (int64_t)NT * VEC) {
    float v[VEC];
    const int n = V - v0 >= VEC ? VEC : (int)(V - v0);
    if (aligned && n == VEC) {
      ld_vec(x + v0, v);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = e < n ? DT<T>::ld(x + v0 + e) : -INFINITY;
    }
    f(v, n, v0);
  }
}

__device__ __forceinline__ int64_t ctc_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename T, int NT>
__global__ __launch_bounds__(NT) void ctc_rows_kernel(const T* logits, int64_t st, int64_t sb, const int64_t* targets, int64_t Lmax,
                                                      const int64_t* target_len, const int64_t* input_len, int64_t blank, float* lse,
                                                      float* emit, int64_t T_, int64_t V) {
  __shared__ float red[NT / 64];
  const int64_t t = blockIdx.x, b = blockIdx.y;
  if (t >= ctc_clamp(input_len[b], T_)) {  // a frame at or past the input length is not read
    if (threadIdx.x == 0) lse[b * T_ + t] = 0.0f;
    return;
  }
  const T* x = logits + t * st + b * sb;
  float mx = -INFINITY;
  ctc_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t) {
#pragma unroll
    for (int e = 0; e < DT<T>::VEC; ++e) mx = fmaxf(mx, v[e]);  // (the cells past n hold -inf)
  });
  mx = ctc_block_max<NT>(mx, red);
  float se = 0.0f;
  ctc_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t) {
#pragma unroll
    for (int e = 0; e < DT<T>::VEC; ++e) if (e < n) se += expf(v[e] - mx);
  });
  se = ctc_block_sum<NT>(se, red);
  const float l = mx + logf(se);
  if (threadIdx.x == 0) lse[b * T_ + t] = l;
  const int64_t L = ctc_clamp(target_len[b], Lmax), S = 2 * L + 1, Sp = 2 * Lmax + 1;
  float* e_out = emit + (b * T_ + t) * Sp;
  for (int64_t s = threadIdx.x; s < S; s += NT) {
    const int64_t c = (s & 1) ? targets[b * Lmax + (s >> 1)] : blank;
    e_out[s] = (c >= 0 && c < V) ? DT<T>::ld(x + c) - l : NAN;  // a label outside the vocabulary reads nothing (the caller checks)
  }
}

__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf((expf(a - m) + expf(b - m)) + expf(c - m));
}

// blockIdx.y = 0: alpha (forward in time, neighbours s - 1, s - 2) and nll;  1: beta (backward in time, neighbours s + 1, s + 2).
// prev[2 + s] holds the other time step's variable of state s; prev[0], prev[1], prev[S + 2], prev[S + 3] stay -inf.
template <int NT>
__global__ __launch_bounds__(NT) void ctc_alpha_beta_kernel(const float* emit, const int64_t* targets, int64_t Lmax, const int64_t* target_len,
                                                            const int64_t* input_len, int64_t blank, float* alpha, float* beta, float* nll,
                                                            int64_t T_) {
  constexpr int KMAX = NT == 1024 ? (CTC_S_MAX + NT - 1) / NT : 1;  // states per thread (the narrower blocks are launched for S <= NT)
  __shared__ float buf[2][CTC_S_MAX + 4];
  __shared__ unsigned char skip[CTC_S_MAX];
  const int64_t b = blockIdx.x;
  const bool back = blockIdx.y == 1;
  const int64_t Tb = ctc_clamp(input_len[b], T_), L = ctc_clamp(target_len[b], Lmax), Sp = 2 * Lmax + 1;
  const int S = (int)(2 * L + 1);
  const int64_t* tg = targets + b * Lmax;
  for (int s = threadIdx.x; s < S + 4; s += NT) buf[0][s] = buf[1][s] = -INFINITY;
  // the skip transition between s and its second neighbour exists when the LATER state (in label order) is a label that differs from
  // the earlier one: forward the later state is s itself, backward it is s + 2
  for (int s = threadIdx.x; s < S; s += NT) {
    const int hi = back ? s + 2 : s, lo = hi - 2;
    skip[s] = (hi & 1) && lo >= 0 && hi < S && tg[hi >> 1] != blank && tg[hi >> 1] != tg[lo >> 1];
  }
  float* out = (back ? beta : alpha) + b * T_ * Sp;
  const float* em = emit + b * T_ * Sp;
  if (Tb == 0) {
    if (!back && threadIdx.x == 0) nll[b] = L == 0 ? 0.0f : INFINITY;
    return;
  }
  const int64_t t0 = back ? Tb - 1 : 0, dt = back ? -1 : 1;
  const int nb = back ? 1 : -1;  // direction of the neighbours
  float e[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int s = threadIdx.x + k * NT;
    e[k] = s < S ? em[t0 * Sp + s] : 0.0f;
  }
  __syncthreads();
  int p = 0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int s = threadIdx.x + k * NT;
    if (s < S) {
      const bool start = back ? s >= S - 2 : s < 2;
      const float a = start ? e[k] : -INFINITY;
      buf[p][2 + s] = a;
      out[t0 * Sp + s] = a;
    }
  }
  for (int64_t i = 1; i < Tb; ++i) {
    const int64_t t = t0 + i * dt;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int s = threadIdx.x + k * NT;
      e[k] = s < S ? em[t * Sp + s] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int s = threadIdx.x + k * NT;
      if (s < S) {
        const float a0 = buf[p][2 + s], a1 = buf[p][2 + s + nb], a2 = skip[s] ? buf[p][2 + s + 2 * nb] : -INFINITY;
        const float a = ctc_lse3(a0, a1, a2) + e[k];
        buf[p ^ 1][2 + s] = a;
        out[t * Sp + s] = a;
      }
    }
    p ^= 1;
  }
  if (back) return;
  __syncthreads();
  if (threadIdx.x == 0) nll[b] = -ctc_lse3(buf[p][2 + S - 1], S > 1 ? buf[p][2 + S - 2] : -INFINITY, -INFINITY);
}

__global__ __launch_bounds__(256) void ctc_loss_sum_kernel(const float* nll, float* loss, int64_t B, int zero_infinity) {
  __shared__ double red[256];
  double a = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float v = nll[b];
    a += (zero_infinity && v == INFINITY) ? 0.0 : (double)v;
  }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)red[0];
}

// One workgroup per frame.  Phase 1 writes g * softmax(x) over the whole row; after a barrier phase 2 subtracts the occupancy at the
// at most L + 1 classes the utterance uses.  The occupancy of a class is the log-sum-exp of alpha + beta over its states, in a fixed
// order: the blank's by the block reduction over the even states, a label's by the thread that owns its FIRST occurrence, which walks
// the later occurrences in increasing s.  One writer per class, no atomics.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void ctc_bwd_kernel(const T* logits, int64_t st, int64_t sb, const int64_t* targets, int64_t Lmax,
                                                     const int64_t* target_len, const int64_t* input_len, int64_t blank, int zero_infinity,
                                                     const float* nll, const float* lse, const float* alpha, const float* beta,
                                                     const float* gscale, T* dlogits, int64_t dst, int64_t dsb, int64_t T_, int64_t V) {
  constexpr int VEC = DT<T>::VEC;
  __shared__ float ab[CTC_S_MAX];
  __shared__ int lbl[CTC_L_MAX];
  __shared__ float red[NT / 64];
  const int64_t t = blockIdx.x, b = blockIdx.y;
  T* d = dlogits + t * dst + b * dsb;
  const bool d_al = ((uintptr_t)d & 15) == 0;
  const float nl = nll[b];
  if (t >= ctc_clamp(input_len[b], T_) || (zero_infinity && nl == INFINITY)) {  // exact zeros, nothing read
    for (int64_t v0 = (int64_t)threadIdx.x * VEC; v0 < V; v0 += (int64_t)NT * VEC) {
      if (d_al && V - v0 >= VEC) {
        if constexpr (VEC == 8) { const u32x4 z = {0u, 0u, 0u, 0u}; *reinterpret_cast<u32x4*>(d + v0) = z; }
        else { const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f}; *reinterpret_cast<f32x4*>(d + v0) = z; }
      } else {
        for (int e = 0; e < VEC && v0 + e < V; ++e) DT<T>::st(d + v0 + e, 0.0f);
      }
    }
    return;
  }
  const T* x = logits + t * st + b * sb;
  const float g = gscale[0], l = lse[b * T_ + t];
  const int64_t L = ctc_clamp(target_len[b], Lmax), Sp = 2 * Lmax + 1;
  const int S = (int)(2 * L + 1);
  const float* al = alpha + (b * T_ + t) * Sp;
  const float* be = beta + (b * T_ + t) * Sp;
  for (int s = threadIdx.x; s < S; s += NT) ab[s] = al[s] + be[s];
  for (int j = threadIdx.x; j < (int)L; j += NT) {
    const int64_t c = targets[b * Lmax + j];
    lbl[j] = (c >= 0 && c < V) ? (int)c : -1;
  }
  ctc_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t v0) {
    if (d_al && n == VEC) {
      if constexpr (VEC == 8) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = g * expf(v[e] - l);
        store8(d + v0, o);
      } else {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = g * expf(v[e] - l);
        *reinterpret_cast<f32x4*>(d + v0) = o;
      }
    } else {
      for (int e = 0; e < n; ++e) DT<T>::st(d + v0 + e, g * expf(v[e] - l));
    }
  });
  __threadfence_block();
  __syncthreads();  // ab / lbl are staged, and phase 1's stores are ordered before phase 2's to the same addresses
  // blank: the even states
  float m = -INFINITY;
  for (int s = 2 * threadIdx.x; s < S; s += 2 * NT) m = fmaxf(m, ab[s]);
  m = ctc_block_max<NT>(m, red);
  float sum = 0.0f;
  for (int s = 2 * threadIdx.x; s < S; s += 2 * NT) sum += m == -INFINITY ? 0.0f : expf(ab[s] - m);
  sum = ctc_block_sum<NT>(sum, red);
  if (threadIdx.x == 0 && blank >= 0 && blank < V) {
    const float lp = DT<T>::ld(x + blank) - l;
    const float occ = expf(((m == -INFINITY ? -INFINITY : m + logf(sum)) + nl) - lp);
    DT<T>::st(d + blank, g * (expf(lp) - occ));
  }
  for (int i = threadIdx.x; i < (int)L; i += NT) {
    const int c = lbl[i];
    if (c < 0 || c == blank) continue;  // (a label equal to the blank is the caller's error; its column stays the softmax term)
    bool first = true;
    for (int j = 0; j < i; ++j) if (lbl[j] == c) { first = false; break; }
    if (!first) continue;
    float mc = ab[2 * i + 1];
    for (int j = i + 1; j < (int)L; ++j) if (lbl[j] == c) mc = fmaxf(mc, ab[2 * j + 1]);
    float sc = 0.0f;
    if (mc != -INFINITY)
      for (int j = i; j < (int)L; ++j) if (lbl[j] == c) sc += expf(ab[2 * j + 1] - mc);
    const float lp = DT<T>::ld(x + c) - l;
    const float occ = expf(((mc == -INFINITY ? -INFINITY : mc + logf(sc)) + nl) - lp);
    DT<T>::st(d + c, g * (expf(lp) - occ));
  }
}

// argmax of one frame, lowest index among equal maxima
template <typename T, int NT>
__global__ __launch_bounds__(NT) void ctc_argmax_kernel(const T* logits, int64_t st, int64_t sb, const int64_t* input_len, int32_t* am,
                                                        int64_t T_, int64_t V) {
  __shared__ float rv[NT / 64];
  __shared__ int ri[NT / 64];
  const int64_t t = blockIdx.x, b = blockIdx.y;
  if (t >= ctc_clamp(input_len[b], T_)) {
    if (threadIdx.x == 0) am[b * T_ + t] = -1;
    return;
  }
  const T* x = logits + t * st + b * sb;
  float bv = -INFINITY;
  int bi = INT32_MAX;
  ctc_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t v0) {
#pragma unroll
    for (int e = 0; e < DT<T>::VEC; ++e)
      if (e < n && (v[e] > bv || (v[e] == bv && (int)(v0 + e) < bi))) { bv = v[e]; bi = (int)(v0 + e); }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if constexpr (NT > 64) {
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = bv; ri[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < NT / 64; ++w)
        if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
  }
  if (threadIdx.x == 0) am[b * T_ + t] = bi == INT32_MAX ? 0 : bi;  // (a row of NaNs: class 0)
}

// collapse runs, drop blanks, compact in frame order: chunks of 256 frames, an inclusive scan of the keep flags per chunk
__global__ __launch_bounds__(256) void ctc_collapse_kernel(const int32_t* am, const int64_t* input_len, int64_t blank, int32_t* ids,
                                                           int32_t* counts, int64_t T_) {
  __shared__ int scan[256];
  const int64_t b = blockIdx.x, Tb = ctc_clamp(input_len[b], T_);
  const int32_t* a = am + b * T_;
  int32_t* o = ids + b * T_;
  int base = 0;
  for (int64_t c0 = 0; c0 < Tb; c0 += 256) {
    const int64_t t = c0 + threadIdx.x;
    int id = -1, keep = 0;
    if (t < Tb) {
      id = a[t];
      keep = id != blank && (t == 0 || id != a[t - 1]);
    }
    scan[threadIdx.x] = keep;
    __syncthreads();
    for (int o2 = 1; o2 < 256; o2 <<= 1) {
      const int v = (int)threadIdx.x >= o2 ? scan[threadIdx.x - o2] : 0;
      __syncthreads();
      scan[threadIdx.x] += v;
      __syncthreads();
    }
    if (keep) o[base + scan[threadIdx.x] - 1] = id;
    base += scan[255];
    __syncthreads();
  }
  for (int64_t t = base + threadIdx.x; t < T_; t += 256) o[t] = -1;
  if (threadIdx.x == 0) counts[b] = base;
}

int ctc_check_common(const char* who, const void* logits, int64_t st, int64_t sb, const int64_t* input_len, int64_t blank, int64_t T,
                     int64_t B, int64_t V, int dtype) {
  CST_REQUIRE(logits && input_len, "%s: null operand", who);
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "%s: bad dtype %d", who, dtype);
  CST_REQUIRE(T > 0 && B > 0 && V > 0 && T <= INT32_MAX && B <= 65535 && V <= INT32_MAX, "%s: bad shape T %lld B %lld V %lld", who,
              (long long)T, (long long)B, (long long)V);
  CST_REQUIRE(blank >= 0 && blank < V, "%s: blank %lld outside the %lld classes", who, (long long)blank, (long long)V);
  CST_REQUIRE(st >= V && sb >= V, "%s: strides %lld / %lld below the class count %lld", who, (long long)st, (long long)sb, (long long)V);
  CST_REQUIRE((uintptr_t)logits % cst_dtype_size(dtype) == 0, "%s: logits are not element-aligned", who);
  return CST_OK;
}

int ctc_check_targets(const char* who, const int64_t* targets, int64_t Lmax, const int64_t* target_len) {
  CST_REQUIRE(target_len && Lmax >= 0 && (targets || Lmax == 0), "%s: null operand", who);
  if (Lmax > CTC_L_MAX) {
    cst_set_error("%s: targets of %lld labels exceed the supported %d (the recursion keeps 2 L + 1 states in LDS)", who, (long long)Lmax,
                  CTC_L_MAX);
    return CST_ERR_UNSUPPORTED;
  }
  return CST_OK;
}

}  // namespace

#define CTC_BY_WIDTH(V, LAUNCH)          \
  do {                                   \
    if ((V) <= 512) { LAUNCH(64); }      \
    else { LAUNCH(256); }                \
  } while (0)

extern "C" int cst_ctc_fwd(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* targets, int64_t Lmax,
                           const int64_t* target_len, const int64_t* input_len, int64_t blank, int zero_infinity, float* nll, float* loss,
                           float* lse, float* emit, float* alpha, float* beta, int64_t T, int64_t B, int64_t V, int dtype,
                           cst_stream stream) {
  int rc = ctc_check_common("cst_ctc_fwd", logits, stride_t, stride_b, input_len, blank, T, B, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(nll && loss && lse && emit && alpha, "cst_ctc_fwd: null operand");
  rc = ctc_check_targets("cst_ctc_fwd", targets, Lmax, target_len);
  if (rc != CST_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Sp = 2 * Lmax + 1;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)T * B * (V * cst_dtype_size(dtype) + 3.0 * Sp * 4));
  const dim3 grid((unsigned)T, (unsigned)B);
#define CTC_ROWS(NT)                                                                                                                      \
  if (dtype == CST_BF16)                                                                                                                  \
    hipLaunchKernelGGL((ctc_rows_kernel<bf16_t, NT>), grid, dim3(NT), 0, s, (const bf16_t*)logits, stride_t, stride_b, targets, Lmax,    \
                       target_len, input_len, blank, lse, emit, T, V);                                                                    \
  else                                                                                                                                    \
    hipLaunchKernelGGL((ctc_rows_kernel<float, NT>), grid, dim3(NT), 0, s, (const float*)logits, stride_t, stride_b, targets, Lmax,      \
                       target_len, input_len, blank, lse, emit, T, V)
  CTC_BY_WIDTH(V, CTC_ROWS);
#undef CTC_ROWS
  const dim3 g2((unsigned)B, beta ? 2u : 1u);
  if (Sp <= 64) hipLaunchKernelGGL(ctc_alpha_beta_kernel<64>, g2, dim3(64), 0, s, (const float*)emit, targets, Lmax, target_len, input_len, blank, alpha, beta, nll, T);
  else if (Sp <= 256) hipLaunchKernelGGL(ctc_alpha_beta_kernel<256>, g2, dim3(256), 0, s, (const float*)emit, targets, Lmax, target_len, input_len, blank, alpha, beta, nll, T);
  else hipLaunchKernelGGL(ctc_alpha_beta_kernel<1024>, g2, dim3(1024), 0, s, (const float*)emit, targets, Lmax, target_len, input_len, blank, alpha, beta, nll, T);
  hipLaunchKernelGGL(ctc_loss_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)nll, loss, B, zero_infinity);
  return cst_check_launch("cst_ctc_fwd");
}

extern "C" int cst_ctc_bwd(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* targets, int64_t Lmax,
                           const int64_t* target_len, const int64_t* input_len, int64_t blank, int zero_infinity, const float* nll,
                           const float* lse, const float* alpha, const float* beta, const float* gscale, void* dlogits, int64_t dstride_t,
                           int64_t dstride_b, int64_t T, int64_t B, int64_t V, int dtype, cst_stream stream) {
  int rc = ctc_check_common("cst_ctc_bwd", logits, stride_t, stride_b, input_len, blank, T, B, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(nll && lse && alpha && beta && gscale && dlogits, "cst_ctc_bwd: null operand");
  CST_REQUIRE(dstride_t >= V && dstride_b >= V && (uintptr_t)dlogits % cst_dtype_size(dtype) == 0, "cst_ctc_bwd: bad gradient layout");
  rc = ctc_check_targets("cst_ctc_bwd", targets, Lmax, target_len);
  if (rc != CST_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Sp = 2 * Lmax + 1;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)T * B * (2.0 * V * cst_dtype_size(dtype) + 2.0 * Sp * 4));
  const dim3 grid((unsigned)T, (unsigned)B);
#define CTC_BWD(NT)                                                                                                                       \
  if (dtype == CST_BF16)                                                                                                                  \
    hipLaunchKernelGGL((ctc_bwd_kernel<bf16_t, NT>), grid, dim3(NT), 0, s, (const bf16_t*)logits, stride_t, stride_b, targets, Lmax,     \
                       target_len, input_len, blank, zero_infinity, nll, lse, alpha, beta, gscale, (bf16_t*)dlogits, dstride_t, dstride_b, \
                       T, V);                                                                                                             \
  else                                                                                                                                    \
    hipLaunchKernelGGL((ctc_bwd_kernel<float, NT>), grid, dim3(NT), 0, s, (const float*)logits, stride_t, stride_b, targets, Lmax,       \
                       target_len, input_len, blank, zero_infinity, nll, lse, alpha, beta, gscale, (float*)dlogits, dstride_t, dstride_b, \
                       T, V)
  CTC_BY_WIDTH(V, CTC_BWD);  // by the class count alone: the blank's reduction tree must not depend on the batch's longest target
#undef CTC_BWD
  return cst_check_launch("cst_ctc_bwd");
}

extern "C" int cst_ctc_greedy(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* input_len, int64_t blank,
                              int32_t* argmax_ws, int32_t* ids, int32_t* counts, int64_t T, int64_t B, int64_t V, int dtype,
                              cst_stream stream) {
  const int rc = ctc_check_common("cst_ctc_greedy", logits, stride_t, stride_b, input_len, blank, T, B, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(argmax_ws && ids && counts, "cst_ctc_greedy: null operand");
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)T * B * V * cst_dtype_size(dtype));
  const dim3 grid((unsigned)T, (unsigned)B);
#define CTC_AM(NT)                                                                                                                        \
  if (dtype == CST_BF16)                                                                                                                  \
    hipLaunchKernelGGL((ctc_argmax_kernel<bf16_t, NT>), grid, dim3(NT), 0, s, (const bf16_t*)logits, stride_t, stride_b, input_len,      \
                       argmax_ws, T, V);                                                                                                  \
  else                                                                                                                                    \
    hipLaunchKernelGGL((ctc_argmax_kernel<float, NT>), grid, dim3(NT), 0, s, (const float*)logits, stride_t, stride_b, input_len,        \
                       argmax_ws, T, V)
  CTC_BY_WIDTH(V, CTC_AM);
#undef CTC_AM
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3((unsigned)B), dim3(256), 0, s, (const int32_t*)argmax_ws, input_len, blank, ids, counts, T);
  return cst_check_launch("cst_ctc_greedy");
}
