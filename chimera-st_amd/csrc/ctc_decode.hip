// ctc_decode.hip — CTC prefix beam search on raw logits (fairseq_infer.py --w2l-decoder beam; Graves 2006 §7.5.3, Hannun et al. 2014 Alg. 1):
//   cst_ctc_topn : per live frame the blank's log-probability, the log-sum-exp and the N most probable non-blank classes
//   cst_ctc_beam : per utterance the search itself over those lists, one workgroup looping over the utterance's frames
// It stands where the flashlight decoders of examples/speech_recognition/w2l_decoder.py stand in the reference (those keep the best path
// per state; this one SUMS the alignments of a prefix, so it is a decoder of its own name, not a port).
//
// cst_ctc_topn, one workgroup per live frame (the structure of ctc_argmax_kernel; rows are visited with ctc.hip's ownership rule: group
//   g = v / VEC belongs to thread g % NT and its elements are taken in index order, by a 16-byte load or by VEC scalar loads of the same
//   elements): mx, se, l = mx + logf(se) in the order of ctc_rows_kernel, so lse has the bits cst_ctc_fwd writes, whatever the layout.
//   Then N rounds of "the best class after the previous one" in the order (lp = x - l descending, class id ascending): nothing is
//   mutated or staged, every round re-reads the row (it sits in L1 / L2 after the first pass) and reduces (lp, id) over the block.
// cst_ctc_beam, one workgroup of 256 threads per utterance.  Per frame:
//   stays     thread i < Kc: tot = p_b (+) p_nb;  p_b' = tot + blank_lp;  p_nb' = p_nb + lp(last) — lp(last) = x[last] - lse read from
//             the logits themselves, so a last token outside the frame's list keeps its exact probability
//   extends   cand[i * N + n] = (tok[n] == last_i ? p_b(i) : tot_i) + lp[n]
//   merge     thread j < Kc: its prefix is parent + token; where the parent is beam entry i and the token is list entry n, cand[i N + n]
//             IS prefix j: it is added to p_nb'(j) and leaves the candidates.  A prefix has one parent, so at most one term arrives.
//   select    at most K rounds of "the best candidate after the previous one" in the order (score descending, source rank ascending,
//             stay before extension, token id ascending) among those not below best - beam_threshold; an extension that is selected
//             takes the node of (parent node, token): the one it had if the prefix was in the beam before (looked up among the parent's
//             children), else a new one.  At most K new nodes per frame: the table of 1 + T K nodes cannot overflow.
//   The beam therefore stays sorted, and the n best hypotheses at the end are its first entries.
// fp32 throughout, expf / logf of libm accuracy (tests/ctc_beam_ref.py counts the roundings).  No atomics of any kind, no grid-wide
// synchronisation; every loop is bounded by T, K or N.
#include "cst_common.h"

#define CTCD_K_MAX 128
#define CTCD_N_MAX 128
#define CTCD_KN_MAX 8192  // candidates kept in LDS (include/cst.h has the arithmetic)
#define CTCD_NT 256

namespace {

template <int NT>
__device__ __forceinline__ float ctcd_block_sum(float v, float* red) {
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
__device__ __forceinline__ float ctcd_block_max(float v, float* red) {
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

// ctc.hip's ctc_row_visit: f(v, n, v0) over the groups of VEC consecutive elements this thread owns
template <typename T, int NT, typename F>
__device__ __forceinline__ void ctcd_row_visit(const T* x, int64_t V, F&& f) {
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

__device__ __forceinline__ int64_t ctcd_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (lp, id) a is ranked before b: higher log-probability, then lower id
__device__ __forceinline__ bool ctcd_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

template <typename T, int NT>
__global__ __launch_bounds__(NT) void ctc_topn_kernel(const T* logits, int64_t st, int64_t sb, const int64_t* input_len, int blank, int N,
                                                      float* lse, float* blank_lp, int32_t* tok_id, float* tok_lp, int64_t T_, int64_t V) {
  __shared__ float red[NT / 64];
  __shared__ float rv[NT / 64];
  __shared__ int ri[NT / 64];
  const int64_t t = blockIdx.x, b = blockIdx.y;
  int32_t* oid = tok_id + (b * T_ + t) * N;
  float* olp = tok_lp + (b * T_ + t) * N;
  if (t >= ctcd_clamp(input_len[b], T_)) {  // a frame at or past the input length is not read
    for (int n = threadIdx.x; n < N; n += NT) { oid[n] = -1; olp[n] = -INFINITY; }
    if (threadIdx.x == 0) { lse[b * T_ + t] = 0.0f; blank_lp[b * T_ + t] = -INFINITY; }
    return;
  }
  const T* x = logits + t * st + b * sb;
  float mx = -INFINITY;
  ctcd_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t) {
#pragma unroll
    for (int e = 0; e < DT<T>::VEC; ++e) mx = fmaxf(mx, v[e]);
  });
  mx = ctcd_block_max<NT>(mx, red);
  float se = 0.0f;
  ctcd_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t) {
#pragma unroll
    for (int e = 0; e < DT<T>::VEC; ++e) if (e < n) se += expf(v[e] - mx);
  });
  se = ctcd_block_sum<NT>(se, red);
  const float l = mx + logf(se);
  if (threadIdx.x == 0) {
    lse[b * T_ + t] = l;
    blank_lp[b * T_ + t] = DT<T>::ld(x + blank) - l;
  }
  float pv = INFINITY;  // the previous round's pick; all threads hold the same pair
  int pi = -1;
  for (int r = 0; r < N; ++r) {
    float bv = -INFINITY;
    int bi = INT32_MAX;
    ctcd_row_visit<T, NT>(x, V, [&](auto& v, int n, int64_t v0) {
#pragma unroll
      for (int e = 0; e < DT<T>::VEC; ++e) {
        const float lp = v[e] - l;
        const int id = (int)(v0 + e);
        if (e < n && id != blank && ctcd_before(pv, pi, lp, id) && ctcd_before(lp, id, bv, bi)) { bv = lp; bi = id; }
      }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ctcd_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if constexpr (NT > 64) {
      __syncthreads();  // the previous round's reads of rv / ri are over
      if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = bv; ri[threadIdx.x >> 6] = bi; }
      __syncthreads();
      bv = rv[0]; bi = ri[0];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w)
        if (ctcd_before(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; }
    }
    if (bi == INT32_MAX) {  // no class is left (V - 1 < N, or NaNs): the same verdict in every thread
      for (int n = r + threadIdx.x; n < N; n += NT) { oid[n] = -1; olp[n] = -INFINITY; }
      break;
    }
    if (threadIdx.x == 0) { oid[r] = bi; olp[r] = bv; }
    pv = bv; pi = bi;
  }
}

__device__ __forceinline__ float ctcd_lae(float a, float b) {  // logaddexp; -inf where both are
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(1.0f + expf(n - m));
}

// candidate order: score descending, then key ascending; key = source rank << 32 | (0: stay, 1 + token: extension)
__device__ __forceinline__ bool ctcd_cand_before(float as, uint64_t ak, float bs, uint64_t bk) { return as > bs || (as == bs && ak < bk); }

__global__ __launch_bounds__(CTCD_NT) void ctc_beam_kernel(const void* logits, int bf16, int64_t st, int64_t sb, const int64_t* input_len,
                                                           const float* lse, const float* blank_lp, const int32_t* tok_id,
                                                           const float* tok_lp, int N, int K, float theta, int nbest, int32_t* nodes,
                                                           int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, int32_t* n_hyp,
                                                           int32_t* trace_node, float* trace_pb, float* trace_pnb, int64_t T_, int64_t V) {
  __shared__ float cand[CTCD_KN_MAX];
  __shared__ int bnode[2][CTCD_K_MAX], bpar[2][CTCD_K_MAX], btok[2][CTCD_K_MAX];
  __shared__ float bpb[2][CTCD_K_MAX], bpnb[2][CTCD_K_MAX];
  __shared__ float tot[CTCD_K_MAX], spb[CTCD_K_MAX], spnb[CTCD_K_MAX], ssc[CTCD_K_MAX];
  __shared__ int ftok[CTCD_N_MAX];
  __shared__ float flp[CTCD_N_MAX];
  __shared__ float rs[CTCD_NT / 64];
  __shared__ uint64_t rk[CTCD_NT / 64];
  __shared__ int head[CTCD_K_MAX], bsrc[CTCD_K_MAX];
  __shared__ int s_nn;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, Tb = ctcd_clamp(input_len[b], T_);
  const int64_t cap = 1 + T_ * K;  // nodes of this utterance's trie
  int32_t* npar = nodes + b * 4 * cap;
  int32_t* ntok = npar + cap;
  int32_t* nkid = ntok + cap;  // a node's most recent child, 0: none (the root is nobody's child)
  int32_t* nsib = nkid + cap;  // the next older child of the same parent, 0: none
  int cur = 0, Kc = 1;  // (uniform across the block)
  if (tid == 0) {
    npar[0] = -1; ntok[0] = -1; nkid[0] = 0; nsib[0] = 0; s_nn = 1;
    bnode[0][0] = 0; bpar[0][0] = -1; btok[0][0] = -1; bpb[0][0] = 0.0f; bpnb[0][0] = -INFINITY;
  }
  __syncthreads();
  for (int64_t t = 0; t < Tb; ++t) {
    const int64_t f = b * T_ + t;
    const float lb = blank_lp[f], l = lse[f];
    for (int n = tid; n < N; n += CTCD_NT) { ftok[n] = tok_id[f * N + n]; flp[n] = tok_lp[f * N + n]; }
    if (tid < Kc) {
      const float pb = bpb[cur][tid], pnb = bpnb[cur][tid], tt = ctcd_lae(pb, pnb);
      const int last = btok[cur][tid];
      float rep = -INFINITY;
      if (last >= 0 && last < V) {
        const int64_t off = t * st + b * sb + last;
        const float x = bf16 ? DT<bf16_t>::ld((const bf16_t*)logits + off) : ((const float*)logits)[off];
        rep = pnb + (x - l);
      }
      tot[tid] = tt; spb[tid] = tt + lb; spnb[tid] = rep;
      head[tid] = nkid[bnode[cur][tid]];
    }
    __syncthreads();
    const int M = Kc * N;
    for (int c = tid; c < M; c += CTCD_NT) {
      const int i = c / N, n = c - i * N, tk = ftok[n];
      cand[c] = tk < 0 ? -INFINITY : (tk == btok[cur][i] ? bpb[cur][i] : tot[i]) + flp[n];
    }
    __syncthreads();
    float best = -INFINITY;
    if (tid < Kc) {
      const int par = bpar[cur][tid], tk = btok[cur][tid];
      int src = -1, ln = -1;
      if (par >= 0) {
        for (int i = 0; i < Kc; ++i) if (bnode[cur][i] == par) { src = i; break; }
        if (src >= 0) for (int n = 0; n < N; ++n) if (ftok[n] == tk) { ln = n; break; }
      }
      if (ln >= 0) {
        spnb[tid] = ctcd_lae(spnb[tid], cand[src * N + ln]);
        cand[src * N + ln] = -INFINITY;  // one writer per cell: a prefix has one parent
      }
      best = ssc[tid] = ctcd_lae(spb[tid], spnb[tid]);
    }
    __syncthreads();
    for (int c = tid; c < M; c += CTCD_NT) best = fmaxf(best, cand[c]);
    best = ctcd_block_max<CTCD_NT>(best, rs);
    const float cut = best - theta;
    __syncthreads();  // rs is free again
    const int nxt = cur ^ 1;
    float ps = INFINITY;
    uint64_t pk = 0;
    int Kn = 0;
    for (int r = 0; r < K; ++r) {
      float ms = -INFINITY;
      uint64_t mk = ~0ull;
      if (tid < Kc) {
        const float s = ssc[tid];
        const uint64_t k = (uint64_t)tid << 32;
        if (s >= cut && s > -INFINITY && ctcd_cand_before(ps, pk, s, k)) { ms = s; mk = k; }
      }
      for (int c = tid; c < M; c += CTCD_NT) {
        const float s = cand[c];
        if (s >= cut && s > -INFINITY && s <= ps && s >= ms) {
          const int i = c / N;
          const uint64_t k = ((uint64_t)i << 32) | (uint32_t)(1 + ftok[c - i * N]);
          if (ctcd_cand_before(ps, pk, s, k) && ctcd_cand_before(s, k, ms, mk)) { ms = s; mk = k; }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(ms, o, 64);
        const uint64_t ok = ((uint64_t)(uint32_t)__shfl_xor((int)(mk >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)mk, o, 64);
        if (ctcd_cand_before(os, ok, ms, mk)) { ms = os; mk = ok; }
      }
      __syncthreads();
      if ((tid & 63) == 0) { rs[tid >> 6] = ms; rk[tid >> 6] = mk; }
      __syncthreads();
      ms = rs[0]; mk = rk[0];
#pragma unroll
      for (int w = 1; w < CTCD_NT / 64; ++w)
        if (ctcd_cand_before(rs[w], rk[w], ms, mk)) { ms = rs[w]; mk = rk[w]; }
      if (mk == ~0ull) break;  // nothing is left above the threshold
      const int i = (int)(mk >> 32), sub = (int)(uint32_t)mk;
      if (sub == 0) {
        if (tid == 0) {
          bnode[nxt][Kn] = bnode[cur][i]; bpar[nxt][Kn] = bpar[cur][i]; btok[nxt][Kn] = btok[cur][i];
          bpb[nxt][Kn] = spb[i]; bpnb[nxt][Kn] = spnb[i];
        }
      } else {
        if (tid == 0) {  // its node is resolved below: an older node of the same (parent, token), or a new one
          bnode[nxt][Kn] = -2; bsrc[Kn] = i; bpar[nxt][Kn] = bnode[cur][i]; btok[nxt][Kn] = sub - 1;
          bpb[nxt][Kn] = -INFINITY; bpnb[nxt][Kn] = ms;
        }
      }
      ++Kn;
      ps = ms; pk = mk;
    }
    __syncthreads();
    // A prefix that left the beam may come back: its node is looked up among its parent's children (a list through nkid / nsib), so a
    // prefix has ONE node and parent / token equality stays exact identity.  The walks run in parallel and only read.
    if (tid < Kn && bnode[nxt][tid] == -2) {
      const int tk = btok[nxt][tid];
      int nd = head[bsrc[tid]];
      for (int64_t g = 0; nd > 0 && g < cap; ++g) {
        if (ntok[nd] == tk) { bnode[nxt][tid] = nd; break; }
        nd = nsib[nd];
      }
    }
    __syncthreads();
    if (tid == 0) {
      int nn = s_nn;
      for (int k = 0; k < Kn; ++k) {
        if (bnode[nxt][k] != -2) continue;
        if (nn >= cap) { Kn = k; break; }  // cannot happen (at most K new nodes per frame); never write past the table
        const int pr = bpar[nxt][k], src = bsrc[k];
        npar[nn] = pr; ntok[nn] = btok[nxt][k]; nkid[nn] = 0; nsib[nn] = head[src];
        head[src] = nn; nkid[pr] = nn;
        bnode[nxt][k] = nn++;
      }
      s_nn = nn;
      bsrc[0] = Kn;
    }
    __syncthreads();
    Kn = bsrc[0];
    cur = nxt; Kc = Kn;
    if (trace_node) {
      for (int k = tid; k < K; k += CTCD_NT) {
        const int64_t o = f * K + k;
        trace_node[o] = k < Kc ? bnode[cur][k] : -1;
        trace_pb[o] = k < Kc ? bpb[cur][k] : -INFINITY;
        trace_pnb[o] = k < Kc ? bpnb[cur][k] : -INFINITY;
      }
    }
    if (Kc == 0) break;  // every candidate was NaN or impossible: no hypothesis
  }
  // the beam is sorted: its first entries are the n best
  const int nh = Kc < nbest ? Kc : nbest;
  if (tid == 0) n_hyp[b] = nh;
  for (int h = tid; h < nbest; h += CTCD_NT) {
    int32_t* out = hyp_tokens + (b * nbest + h) * T_;
    int len = 0;
    if (h < nh) {
      for (int nd = bnode[cur][h]; nd > 0 && len < T_; nd = npar[nd]) ++len;
      int p = len;
      for (int nd = bnode[cur][h]; nd > 0 && p > 0; nd = npar[nd]) out[--p] = ntok[nd];
    }
    for (int64_t p = len; p < T_; ++p) out[p] = -1;
    hyp_len[b * nbest + h] = len;
    hyp_score[b * nbest + h] = h < nh ? ctcd_lae(bpb[cur][h], bpnb[cur][h]) : -INFINITY;
  }
}

int ctcd_check_common(const char* who, const void* logits, int64_t st, int64_t sb, const int64_t* input_len, int64_t blank, int64_t T,
                      int64_t B, int64_t V, int dtype) {
  CST_REQUIRE(logits && input_len, "%s: null operand", who);
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "%s: bad dtype %d", who, dtype);
  CST_REQUIRE(T > 0 && B > 0 && V > 0 && T <= INT32_MAX && B <= 65535 && V <= INT32_MAX - 1, "%s: bad shape T %lld B %lld V %lld", who,
              (long long)T, (long long)B, (long long)V);
  CST_REQUIRE(blank >= 0 && blank < V, "%s: blank %lld outside the %lld classes", who, (long long)blank, (long long)V);
  CST_REQUIRE(st >= V && sb >= V, "%s: strides %lld / %lld below the class count %lld", who, (long long)st, (long long)sb, (long long)V);
  CST_REQUIRE((uintptr_t)logits % cst_dtype_size(dtype) == 0, "%s: logits are not element-aligned", who);
  return CST_OK;
}

}  // namespace

extern "C" int cst_ctc_topn(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* input_len, int64_t blank, int64_t N,
                            float* lse, float* blank_lp, int32_t* tok_id, float* tok_lp, int64_t T, int64_t B, int64_t V, int dtype,
                            cst_stream stream) {
  const int rc = ctcd_check_common("cst_ctc_topn", logits, stride_t, stride_b, input_len, blank, T, B, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(lse && blank_lp && tok_id && tok_lp, "cst_ctc_topn: null operand");
  CST_REQUIRE(N >= 1, "cst_ctc_topn: bad list length %lld", (long long)N);
  if (N > CTCD_N_MAX) {
    cst_set_error("cst_ctc_topn: %lld classes per frame exceed the supported %d", (long long)N, CTCD_N_MAX);
    return CST_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)T * B * (V * cst_dtype_size(dtype) + 8.0 * N));
  const dim3 grid((unsigned)T, (unsigned)B);
#define CTC_TOPN(NT)                                                                                                                      \
  if (dtype == CST_BF16)                                                                                                                  \
    hipLaunchKernelGGL((ctc_topn_kernel<bf16_t, NT>), grid, dim3(NT), 0, s, (const bf16_t*)logits, stride_t, stride_b, input_len,        \
                       (int)blank, (int)N, lse, blank_lp, tok_id, tok_lp, T, V);                                                          \
  else                                                                                                                                    \
    hipLaunchKernelGGL((ctc_topn_kernel<float, NT>), grid, dim3(NT), 0, s, (const float*)logits, stride_t, stride_b, input_len,          \
                       (int)blank, (int)N, lse, blank_lp, tok_id, tok_lp, T, V)
  if (V <= 512) { CTC_TOPN(64); }
  else { CTC_TOPN(256); }
#undef CTC_TOPN
  return cst_check_launch("cst_ctc_topn");
}

extern "C" int64_t cst_ctc_beam_workspace_bytes(int64_t T, int64_t B, int64_t K, int64_t N) {
  (void)N;  // the candidates live in LDS; the workspace is the node table alone
  if (T < 1 || B < 1 || K < 1) return 0;
  return B * 4 * (1 + T * K) * (int64_t)sizeof(int32_t);
}

extern "C" int cst_ctc_beam(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* input_len, int64_t blank,
                            const float* lse, const float* blank_lp, const int32_t* tok_id, const float* tok_lp, int64_t N, int64_t K,
                            float beam_threshold, int64_t nbest, void* workspace, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score,
                            int32_t* n_hyp, int32_t* trace_node, float* trace_pb, float* trace_pnb, int64_t T, int64_t B, int64_t V,
                            int dtype, cst_stream stream) {
  const int rc = ctcd_check_common("cst_ctc_beam", logits, stride_t, stride_b, input_len, blank, T, B, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(lse && blank_lp && tok_id && tok_lp && workspace && hyp_tokens && hyp_len && hyp_score && n_hyp, "cst_ctc_beam: null operand");
  CST_REQUIRE((!trace_node && !trace_pb && !trace_pnb) || (trace_node && trace_pb && trace_pnb), "cst_ctc_beam: the trace needs all three buffers");
  CST_REQUIRE(N >= 1 && K >= 1 && nbest >= 1 && nbest <= K, "cst_ctc_beam: bad beam %lld, list %lld or nbest %lld", (long long)K, (long long)N,
              (long long)nbest);
  CST_REQUIRE(beam_threshold >= 0.0f, "cst_ctc_beam: bad beam threshold %g", (double)beam_threshold);  // (a NaN fails this too)
  if (K > CTCD_K_MAX || N > CTCD_N_MAX || K * N > CTCD_KN_MAX) {
    cst_set_error("cst_ctc_beam: beam %lld x %lld classes per frame is beyond the supported K <= %d, N <= %d, K N <= %d (the candidates' "
                  "scores are kept in LDS)", (long long)K, (long long)N, CTCD_K_MAX, CTCD_N_MAX, CTCD_KN_MAX);
    return CST_ERR_UNSUPPORTED;
  }
  CST_REQUIRE(T * K < INT32_MAX, "cst_ctc_beam: %lld x %lld trie nodes do not fit int32", (long long)T, (long long)K);
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)T * B * (8.0 * N + 8.0) + (double)B * nbest * T * 4.0);
  hipLaunchKernelGGL(ctc_beam_kernel, dim3((unsigned)B), dim3(CTCD_NT), 0, s, logits, dtype == CST_BF16 ? 1 : 0, stride_t, stride_b,
                     input_len, lse, blank_lp, tok_id, tok_lp, (int)N, (int)K, beam_threshold, (int)nbest, (int32_t*)workspace, hyp_tokens,
                     hyp_len, hyp_score, n_hyp, trace_node, trace_pb, trace_pnb, T, V);
  return cst_check_launch("cst_ctc_beam");
}
