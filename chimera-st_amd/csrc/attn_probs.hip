// attn_probs.hip — cst_attn_avg_probs: the head-averaged cross-attention probabilities of the reference's decoder
// (modules/multihead_attention.py:334-362 -> models/transformer.py:808-812), which the fused attention kernels never materialise.  It
// serves --print-alignment: the decode engine appends one row per hypothesis row and step to its attention history, the module path
// returns [B, Tq, S] as the second value of MultiheadAttention.forward(need_weights=True).
//
// One launch, one workgroup per (sentence, tile of QT query rows), one THREAD per key.  Pass 1: per head, every thread folds its keys'
// scores into an online (maximum, sum) per query row; the waves' states are merged by a butterfly, the workgroup's in wave order, and
// land in LDS as stats[row][head].  Pass 2: every thread recomputes its keys' scores head by head and adds exp(s - max) / sum to its
// QT accumulators in the order h = 0 .. H-1, then writes (or adds to) `out`.  The scores are never stored, so any S runs; no
// floating-point atomics, so a call is bit-reproducible.  The queries are wave-uniform operands (every lane of a wave reads the same
// q row), the key row of a thread lives in registers across the QT rows.
#include "cst_common.h"

namespace {

// merge of two online-softmax states (maximum, sum of exp(s - maximum)); (-inf, 0) is the empty state
__device__ __forceinline__ void ml_merge(float& m, float& l, float m2, float l2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) { l = 0.0f; return; }
  l = l * expf(m - M) + l2 * expf(m2 - M);
  m = M;
}

template <typename T, int D, int QT>
__device__ __forceinline__ void scores_of_key(const T* __restrict__ krow, const T* const (&qrow)[QT], float scale, float (&s)[QT]) {
  constexpr int VEC = DT<T>::VEC;
  float kf[D];
#pragma unroll
  for (int e0 = 0; e0 < D; e0 += VEC) {
    float v[VEC];
    ld_vec<T>(krow + e0, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) kf[e0 + e] = v[e];
  }
#pragma unroll
  for (int r = 0; r < QT; ++r) {
    float d = 0.0f;
#pragma unroll
    for (int e0 = 0; e0 < D; e0 += VEC) {
      float qv[VEC];
      ld_vec<T>(qrow[r] + e0, qv);  // (a wave-uniform address)
#pragma unroll
      for (int e = 0; e < VEC; ++e) d = fmaf(qv[e], kf[e0 + e], d);
    }
    {
#pragma clang fp contract(off)  // a rounded product of its own: contracted into `s - max` of pass 2 it would differ from pass 1's
      s[r] = scale * d;
    }
  }
}

template <typename T, int D, int QT>
__global__ __launch_bounds__(1024) void attn_avg_probs_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t k_sb, int64_t k_sh,
                                                              int64_t k_st, const uint8_t* __restrict__ kpm, float* __restrict__ out,
                                                              int64_t out_row_stride, const int32_t* __restrict__ stepp, int max_len, int Tq, int H,
                                                              int S, float scale, float out_scale_h, int accumulate) {
  int64_t out_off = 0;
  if (stepp) {
    const int st = *stepp;
    if (st > max_len) return;
    out_off = (int64_t)st * S;
  }
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int NW = blockDim.x >> 6;
  float* sm = lds;                    // [QT][H] maxima
  float* sl = lds + QT * H;           // [QT][H] sums
  float* red = lds + 2 * QT * H;      // [NW][QT][2] the waves' states of the head at hand
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y, t0 = blockIdx.x * QT;
  const T* kb = k + (int64_t)b * k_sb;
  const uint8_t* mb = kpm ? kpm + (int64_t)b * S : nullptr;
  const T* qbase[QT];
#pragma unroll
  for (int r = 0; r < QT; ++r) {
    const int t = t0 + r < Tq ? t0 + r : Tq - 1;  // (rows past the end repeat the last one and are not written)
    qbase[r] = q + ((int64_t)b * Tq + t) * ldq;
  }
  // ---- pass 1: (maximum, sum) of every (row, head) ----
  for (int h = 0; h < H; ++h) {
    const T* qrow[QT];
#pragma unroll
    for (int r = 0; r < QT; ++r) qrow[r] = qbase[r] + h * D;
    float m[QT], l[QT];
#pragma unroll
    for (int r = 0; r < QT; ++r) { m[r] = -INFINITY; l[r] = 0.0f; }
    for (int j = tid; j < S; j += blockDim.x) {
      if (mb && mb[j]) continue;
      float s[QT];
      scores_of_key<T, D, QT>(kb + (int64_t)h * k_sh + (int64_t)j * k_st, qrow, scale, s);
#pragma unroll
      for (int r = 0; r < QT; ++r) {
        if (s[r] > m[r]) { l[r] = l[r] * expf(m[r] - s[r]) + 1.0f; m[r] = s[r]; }
        else l[r] += expf(s[r] - m[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < QT; ++r) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m[r], o, 64), l2 = __shfl_xor(l[r], o, 64);
        ml_merge(m[r], l[r], m2, l2);
      }
      if (lane == 0) { red[(wave * QT + r) * 2] = m[r]; red[(wave * QT + r) * 2 + 1] = l[r]; }
    }
    __syncthreads();
    if (tid < QT) {
      float mm = red[tid * 2], ll = red[tid * 2 + 1];
      for (int w = 1; w < NW; ++w) ml_merge(mm, ll, red[(w * QT + tid) * 2], red[(w * QT + tid) * 2 + 1]);
      sm[tid * H + h] = mm;
      sl[tid * H + h] = ll;
    }
    __syncthreads();
  }
  // ---- pass 2: the probabilities, heads added in the order 0 .. H-1 ----
  for (int j = tid; j < S; j += blockDim.x) {
    float acc[QT];
#pragma unroll
    for (int r = 0; r < QT; ++r) acc[r] = 0.0f;
    if (!(mb && mb[j])) {
      for (int h = 0; h < H; ++h) {
        const T* qrow[QT];
#pragma unroll
        for (int r = 0; r < QT; ++r) qrow[r] = qbase[r] + h * D;
        float s[QT];
        scores_of_key<T, D, QT>(kb + (int64_t)h * k_sh + (int64_t)j * k_st, qrow, scale, s);
#pragma unroll
        for (int r = 0; r < QT; ++r) acc[r] += expf(s[r] - sm[r * H + h]) / sl[r * H + h];
      }
    }
#pragma unroll
    for (int r = 0; r < QT; ++r) {
      if (t0 + r < Tq) {
        float* o = out + ((int64_t)b * Tq + t0 + r) * out_row_stride + out_off + j;
        const float v = acc[r] * out_scale_h;
        *o = accumulate ? *o + v : v;
      }
    }
  }
}

}  // namespace

extern "C" int cst_attn_avg_probs(const void* q, int64_t ldq, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_st, const uint8_t* key_padding_mask,
                                  float* out, int64_t out_row_stride, const int32_t* step, int64_t max_len, int64_t B, int64_t Tq, int64_t H, int64_t D,
                                  int64_t S, float scale, float out_scale, int accumulate, int dtype, cst_stream stream) {
  CST_REQUIRE(q && k && out, "cst_attn_avg_probs: null operand");
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_attn_avg_probs: bad dtype %d", dtype);
  CST_REQUIRE(D == 32 || D == 64, "cst_attn_avg_probs: head dim %lld not in {32,64}", (long long)D);
  CST_REQUIRE(B > 0 && B <= 65535 && Tq > 0 && H > 0 && H * D <= 16384 && S > 0 && S < (1ll << 31) && Tq < (1ll << 31),
              "cst_attn_avg_probs: bad shape (B %lld, Tq %lld, H %lld, S %lld)", (long long)B, (long long)Tq, (long long)H, (long long)S);
  const int64_t vec = dtype == CST_BF16 ? 8 : 4;
  CST_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)out % 16) == 0 && ldq % vec == 0 && k_sb % vec == 0 && k_sh % vec == 0 &&
                  k_st % vec == 0, "cst_attn_avg_probs: q, k and out 16-byte aligned, ldq and the k strides multiples of 16 bytes required");
  CST_REQUIRE(ldq >= H * D && out_row_stride >= S, "cst_attn_avg_probs: ldq %lld < H*D or out_row_stride %lld < S", (long long)ldq, (long long)out_row_stride);
  CST_REQUIRE(step == nullptr || max_len >= 1, "cst_attn_avg_probs: max_len %lld with a step counter", (long long)max_len);
  hipStream_t s = (hipStream_t)stream;
  // query rows per workgroup: the tile that leaves the fewest idle rows (1, 5 = the default beam, 8)
  const int QT = Tq == 1 ? 1 : (cst_ceil_div(Tq, 5) * 5 < cst_ceil_div(Tq, 8) * 8 ? 5 : 8);
  const int threads = S <= 256 ? 256 : S <= 512 ? 512 : 1024;
  const size_t lds = ((size_t)2 * QT * H + (size_t)(threads / 64) * QT * 2) * sizeof(float);
  const dim3 grid((unsigned)cst_ceil_div(Tq, QT), (unsigned)B);
  const float osh = out_scale * (1.0f / (float)H);
  CstProfScope prof(CST_K_ATTN_FWD, s, 4.0 * B * Tq * H * D * S, (double)B * S * H * D * cst_dtype_size(dtype) + 4.0 * B * Tq * S);
  prof.tag("avg_probs B%lld Tq%lld H%lld D%lld S%lld", (long long)B, (long long)Tq, (long long)H, (long long)D, (long long)S);
#define CST_AAP(T, DD, QQ)                                                                                                                        \
  hipLaunchKernelGGL((attn_avg_probs_kernel<T, DD, QQ>), grid, dim3(threads), lds, s, (const T*)q, ldq, (const T*)k, k_sb, k_sh, k_st, key_padding_mask, \
                     out, out_row_stride, step, (int)max_len, (int)Tq, (int)H, (int)S, scale, osh, accumulate)
#define CST_AAP_Q(T, DD) do { if (QT == 1) CST_AAP(T, DD, 1); else if (QT == 5) CST_AAP(T, DD, 5); else CST_AAP(T, DD, 8); } while (0)
  if (dtype == CST_BF16) { if (D == 64) CST_AAP_Q(bf16_t, 64); else CST_AAP_Q(bf16_t, 32); }
  else { if (D == 64) CST_AAP_Q(float, 64); else CST_AAP_Q(float, 32); }
#undef CST_AAP_Q
#undef CST_AAP
  return cst_check_launch("cst_attn_avg_probs");
}
