// decode.hip — the decoder layers of device-resident incremental decoding: the embedding, the single-query self-attention of the
// incremental MHA branch (modules/multihead_attention.py:189-293), the cross attention and the projections of one step of
// fairseq/sequence_generator.py:_generate (:286-541), as kernels that read the step counter from DEVICE memory, so that one decode
// step (embed -> 6 decoder layers -> vocabulary projection -> the beam search step of beam_search.hip) is a fixed launch sequence
// that the host captures once in a hipGraph and replays; the host never synchronises inside the loop (it polls `num_remaining`).
//
// K/V caches are append-only: hypothesis row h writes its new key/value at slot [h][step] and the beam reorder of
// reorder_incremental_state (multihead_attention.py:419-437: index_select on [B*beam, H, t, D] every step) is replaced
// by an ancestry table anc[h][j] = the cache row that holds position j of hypothesis h — reordering moves (t+1) int32
// per hypothesis instead of 2 * layers * t * C cache elements.
#include "cst_common.h"

namespace {

// x[h] = embed_scale * E[tokens[h][step]] + P[pad + 1 + step]   (models/transformer.py:744-760 on the incremental branch;
// sinusoidal_positional_embedding.py:88-95: the position of the newest token is pad + seq_len for every row)
template <typename T>
__global__ void dec_embed_kernel(const int64_t* tokens, const int32_t* stepp, const T* embed, const float* pos, float scale,
                                 int pad, T* out, int rows, int C, int max_len, int pos_rows) {
  const int s = *stepp;
  if (s > max_len) return;
  const int h = blockIdx.x, LT = max_len + 2;
  const int64_t tok = tokens[((int64_t)(s & 1) * rows + h) * LT + s];
  const int pr = pad + 1 + s < pos_rows ? pad + 1 + s : pos_rows - 1;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
#pragma clang fp contract(off)  // the reference multiplies, rounds, then adds (two ATen kernels): no fused multiply-add here
    const float e = DT<T>::ld(embed + tok * C + c);
    const float se = scale * e;
    DT<T>::st(out + (int64_t)h * C + c, se + pos[(int64_t)pr * C + c]);
  }
}

// packed 16-byte vector -> floats (keeps in-flight loads at 4 VGPRs each instead of 8 for bf16)
template <typename T>
__device__ __forceinline__ void cvt_vec(const u32x4& r, float (&v)[DT<T>::VEC]) {
  if constexpr (DT<T>::VEC == 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(r[i] << 16); v[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u); }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(r[i]);
  }
}
template <typename T>
__device__ __forceinline__ void st_vec(T* p, const float (&v)[DT<T>::VEC]) {
  if constexpr (DT<T>::VEC == 8) { float v8[8]; for (int e = 0; e < 8; ++e) v8[e] = v[e]; store8(p, v8); }
  else { f32x4 a = {v[0], v[1], v[2], v[3]}; *reinterpret_cast<f32x4*>(p) = a; }
}

// Single-query self-attention over the append-only caches; one wave per (hypothesis, head), no LDS.
// A key / value row of one head is D*sizeof(T) contiguous bytes: LPK = that / 16 lanes cover it with one 16-byte load each, so a
// 64-lane load instruction fetches KPI = 64 / LPK whole rows (full 128-byte lines, not 64 scattered 16-byte pieces).  One pass
// with an online softmax: the K and V loads of UNR * KPI positions are issued together (the loop is a chain of memory round
// trips, so bytes in flight per wave is what sets its speed); scores = per-lane partial dots reduced over the LPK lanes of a key;
// the output = per-slot partial sums reduced over the KPI slots at the end.
template <typename T, int D>
__global__ __launch_bounds__(256) void dec_self_attn_kernel(const T* qkv, T* kc, T* vc, const int32_t* anc2, const int32_t* stepp,
                                                            T* out, int rows, int H, int max_len, float scale) {
  constexpr int VEC = DT<T>::VEC;          // elements per 16-byte vector
  constexpr int LPK = D / VEC;             // lanes per key row
  constexpr int KPI = 64 / LPK;            // key rows per load instruction
  constexpr int UNR = 8;
  const int s = *stepp;
  if (s > max_len) return;
  const int L1 = max_len + 1, C = H * D;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int item = blockIdx.x * (blockDim.x >> 6) + wave;
  if (item >= rows * H) return;            // waves are independent: no block-level barrier below
  const int h = item / H, head = item % H;
  const int32_t* anc = anc2 + ((int64_t)(s & 1) * rows + h) * L1;
  const int slot = lane / LPK, c0 = (lane % LPK) * VEC;
  const T* qp = qkv + (int64_t)h * 3 * C + head * D + c0;
  const T* kn = qp + C;
  const T* vn = qp + 2 * C;
  const int64_t hoff = (int64_t)head * D + c0;
  float q[VEC];
  ld_vec<T>(qp, q);
#pragma unroll
  for (int e = 0; e < VEC; ++e) q[e] *= scale;
  // caches are head-major [rows][H][L1][D]: the positions of one head are contiguous (128-byte rows back to back), so the KPI
  // rows of a load instruction are one contiguous KPI*128-byte run wherever the ancestry does not switch rows
  if (slot == 0) {  // append this step's key / value (slot 0's lanes hold one full row between them)
    *reinterpret_cast<u32x4*>(kc + (((int64_t)h * H + head) * L1 + s) * D + c0) = *reinterpret_cast<const u32x4*>(kn);
    *reinterpret_cast<u32x4*>(vc + (((int64_t)h * H + head) * L1 + s) * D + c0) = *reinterpret_cast<const u32x4*>(vn);
  }
  float m = -INFINITY, l = 0.0f, acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
  // bf16 (the timed configuration): scores in log2 units (one v_exp_f32 per probability), the 8-lane dot-product sums by DPP instead
  // of ds_bpermute.  fp32 (the parity configuration) keeps expf and the shuffle order its token ids were pinned with.
  constexpr bool FAST = sizeof(T) == 2 && LPK == 8;
  if (FAST) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[e] *= 1.4426950408889634f;
  }
  // The ancestry entries of a batch are a memory round trip IN FRONT of its K / V loads (their addresses): the next batch's are
  // requested while this one is worked on, so only the first batch pays for both.
  int an[UNR];
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int j = u * KPI + slot;
    an[u] = j < s ? anc[j] : 0;
  }
  for (int j0 = 0; j0 <= s; j0 += KPI * UNR) {
    u32x4 tk[UNR], tv[UNR];
    float part[UNR];
    int an_next[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int jn = j0 + KPI * UNR + u * KPI + slot;
      an_next[u] = jn < s ? anc[jn] : 0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * KPI + slot;
      if (j <= s) {  // position s comes from the projection buffer, not from the cache (written above by other lanes)
        const int64_t off = j == s ? 0 : (((int64_t)an[u] * H + head) * L1 + j) * D + c0;
        tk[u] = *reinterpret_cast<const u32x4*>(j == s ? kn : kc + off);
        tv[u] = *reinterpret_cast<const u32x4*>(j == s ? vn : vc + off);
      }
    }
    float bm = -INFINITY;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * KPI + slot;
      float d = 0.0f;
      if (j <= s) {
        float kf[VEC];
        cvt_vec<T>(tk[u], kf);
#pragma unroll
        for (int e = 0; e < VEC; ++e) d = fmaf(q[e], kf[e], d);
      }
      if constexpr (FAST) {
        d += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
        d += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
        d += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d), 0x141, 0xF, 0xF, true));  // row_half_mirror: the other quad of the 8
      } else {
#pragma unroll
        for (int o = LPK >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      }
      part[u] = j <= s ? d : -INFINITY;
      bm = fmaxf(bm, part[u]);
    }
    bm = wave_max(bm);
    const float mn = fmaxf(m, bm);
    const float corr = m == -INFINITY ? 0.0f : (FAST ? __builtin_amdgcn_exp2f(m - mn) : expf(m - mn));
    l *= corr;
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] *= corr;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * KPI + slot;
      if (j <= s) {
        const float pe = FAST ? __builtin_amdgcn_exp2f(part[u] - mn) : expf(part[u] - mn);
        l += pe;
        float vf[VEC];
        cvt_vec<T>(tv[u], vf);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(pe, vf[e], acc[e]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) an[u] = an_next[u];
    m = mn;
  }
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    l += __shfl_xor(l, o, 64);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] /= l;
  if (slot == 0) st_vec<T>(out + (int64_t)h * C + hoff, acc);
}

// Cross attention of the decode step: one workgroup per (sentence, head).  The encoder keys / values of a sentence are shared
// by its `beam` hypotheses (they are never replicated or reordered: the reference's reorder_encoder_out + static_kv caches hold
// beam copies), so every K / V row is read once per step and used for BQ queries.  4 waves split the source positions; rows are
// fetched as whole 128-byte lines (LPK lanes per row, as in the self-attention kernel).  ONE pass: the K and V loads of a batch
// of UNR * KPI positions are issued together and folded into per-query online-softmax state (running max, sum, output); the
// four waves' states are merged through LDS at the end.  (The first version made three passes — scores to LDS, exp, P V — i.e.
// twice the dependent memory round trips per wave: 51 us per layer against 37 for the flash kernel on the same shape.)
template <typename T, int D, int BQ, int NW>
__global__ __launch_bounds__(NW * 64, 8 / NW) void dec_cross_attn_kernel(const T* q, const T* kx, const T* vx, const uint8_t* kpm, T* out,
                                                                const int32_t* stepp, int max_len, int beam, int H, int S, float scale) {
  constexpr int VEC = DT<T>::VEC, LPK = D / VEC, KPI = 64 / LPK, UNR = 4;
  extern __shared__ float smem[];
  if (*stepp > max_len) return;
  float* sm_m = smem;                    // [NW][BQ]
  float* sm_l = smem + NW * BQ;          // [NW][BQ]
  float* sm_o = smem + 2 * NW * BQ;      // [NW][BQ][D]
  float* sm_q = sm_o + NW * BQ * D;      // [BQ][D] scaled queries (read per batch instead of pinning BQ * VEC registers)
  const int b = blockIdx.x / H, head = blockIdx.x % H, C = H * D;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int slot = lane / LPK, c0 = (lane % LPK) * VEC;
  const T* kb = kx + ((int64_t)b * H + head) * S * D + c0;  // head-major [bsz][H][S][D]: a head's rows are one contiguous stream
  const T* vb = vx + ((int64_t)b * H + head) * S * D + c0;
  const uint8_t* mk = kpm ? kpm + (int64_t)b * S : nullptr;
  for (int q0 = 0; q0 < beam; q0 += BQ) {
    const int nq = beam - q0 < BQ ? beam - q0 : BQ;
    __syncthreads();
    for (int i = tid; i < BQ * D; i += NW * 64) {
      const int qi = i / D, dd = i % D;
      sm_q[i] = qi < nq ? DT<T>::ld(q + ((int64_t)(b * beam + q0 + qi)) * C + head * D + dd) * scale : 0.0f;
    }
    __syncthreads();
    float mq[BQ], lq[BQ], acc[BQ][VEC];
#pragma unroll
    for (int qi = 0; qi < BQ; ++qi) {
      mq[qi] = -INFINITY; lq[qi] = 0.0f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[qi][e] = 0.0f;
    }
    for (int j0 = wave * KPI * UNR; j0 < S; j0 += NW * KPI * UNR) {
      u32x4 tk[UNR], tv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int j = j0 + u * KPI + slot;
        if (j < S) {
          tk[u] = *reinterpret_cast<const u32x4*>(kb + (int64_t)j * D);
          tv[u] = *reinterpret_cast<const u32x4*>(vb + (int64_t)j * D);
        }
      }
      float part[UNR][BQ];
      float bm[BQ];
#pragma unroll
      for (int qi = 0; qi < BQ; ++qi) bm[qi] = -INFINITY;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int j = j0 + u * KPI + slot;
        const bool ok = j < S && !(mk && mk[j < S ? j : 0]);
        float kf[VEC];
        cvt_vec<T>(tk[u], kf);
#pragma unroll
        for (int qi = 0; qi < BQ; ++qi) {
          float d = 0.0f;
          if (j < S) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) d = fmaf(sm_q[qi * D + c0 + e], kf[e], d);
          }
#pragma unroll
          for (int o = LPK >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
          part[u][qi] = ok ? d : -INFINITY;
          bm[qi] = fmaxf(bm[qi], part[u][qi]);
        }
      }
#pragma unroll
      for (int qi = 0; qi < BQ; ++qi) {
        const float mn = fmaxf(mq[qi], wave_max(bm[qi]));
        const float corr = (mq[qi] == -INFINITY) ? 0.0f : expf(mq[qi] - mn);
        lq[qi] *= corr;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[qi][e] *= corr;
        mq[qi] = mn;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int j = j0 + u * KPI + slot;
        if (j < S) {
          float vf[VEC];
          cvt_vec<T>(tv[u], vf);
#pragma unroll
          for (int qi = 0; qi < BQ; ++qi) {
            const float pe = part[u][qi] == -INFINITY ? 0.0f : expf(part[u][qi] - mq[qi]);
            lq[qi] += pe;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[qi][e] = fmaf(pe, vf[e], acc[qi][e]);
          }
        }
      }
    }
    // per-wave state: reduce the KPI slots (every lane of a slot counted its keys once per lane -> l is per slot), publish
#pragma unroll
    for (int qi = 0; qi < BQ; ++qi) {
#pragma unroll
      for (int o = LPK; o < 64; o <<= 1) {
        lq[qi] += __shfl_xor(lq[qi], o, 64);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[qi][e] += __shfl_xor(acc[qi][e], o, 64);
      }
      if (lane == 0) { sm_m[wave * BQ + qi] = mq[qi]; sm_l[wave * BQ + qi] = lq[qi]; }
      if (slot == 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) sm_o[(wave * BQ + qi) * D + c0 + e] = acc[qi][e];
      }
    }
    __syncthreads();
    for (int i = tid; i < nq * D; i += NW * 64) {
      const int qi = i / D, dd = i % D;
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < NW; ++w) M = fmaxf(M, sm_m[w * BQ + qi]);
      float l = 0.0f, o = 0.0f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const float f = sm_m[w * BQ + qi] == -INFINITY ? 0.0f : expf(sm_m[w * BQ + qi] - M);
        l += sm_l[w * BQ + qi] * f;
        o += sm_o[(w * BQ + qi) * D + dd] * f;
      }
      // a sentence whose every key is masked has l = 0: its rows come back as +0 (as from the matrix-core kernel), not 0 / 0 — a NaN row
      // would stay in the state of a replayed graph.  Every other row has l >= 1 (its maximal key counts exp(0)) and the same bits as before.
      DT<T>::st(out + ((int64_t)(b * beam + q0 + qi)) * C + head * D + dd, l > 0.0f ? o / l : 0.0f);
    }
  }
}

// ---- decode-step Linear (include/cst.h: cst_dec_linear) ---------------------------------------------------------------------------
// y[M, N] = act(x[M, K] W[N, K]^T + b) (+ resid) for the few hundred hypothesis rows of a beam-search step.  The step is bound by
// streaming each weight matrix (2-8 MB) from HBM ONCE; that takes every byte of it requested within one memory round trip, so the
// matrix is cut into many small workgroups that keep nothing but loads in flight:
//   workgroup = NT x 16 weight rows (output columns) x TT x 16 hypothesis rows, 4 waves; wave w owns K quarter w for the whole tile,
//   operands go global -> registers (no LDS staging: each wave reads its 16-byte k chunks of W rows and x rows straight into
//   MFMA fragments; x comes from L2, it is shared by every workgroup), v_mfma_f32_16x16x32_bf16 with D = W-frag x x-frag, so a lane
//   ends up with 4 consecutive output columns of one hypothesis row; the weights of the next UN k-steps are requested before the
//   MFMAs of the current ones.  The four waves' partial sums are added in wave order through LDS (deterministic), then bias /
//   activation / residual and one 8-byte store per lane and tile.
// LN (fused LayerNorm of the rows of x, models/transformer_layer.py:346-349 / :369-372 / :403-406 in front of the projection):
//   LN(x) W^T + b = rstd_m (x Wg^T - mean_m sg) + sb   with Wg = W * gamma (columns scaled, rounded to bf16 once when the engine packs
//   its weights), sg[n] = sum_k Wg[n,k], sb[n] = sum_k W[n,k] beta[k] + b[n] (fp32).  The kernel multiplies the RAW rows by Wg and
//   gathers sum(x), sum(x^2) of every row from the fragments it loads anyway (each workgroup sees whole rows), so the LayerNorm
//   launch and its activation round trip disappear; W is then Wg, `bias` is unused, ln_sg / ln_sb are the two vectors.
template <int NT, int TT, int UN, bool LN, int NW>
__global__ __launch_bounds__(NW * 64) void dec_linear_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W, const bf16_t* __restrict__ bias,
                                                         const bf16_t* resid, bf16_t* y, int M, int N, int K, int64_t ldx, int64_t ldr,
                                                         int64_t ldy, int act, const int32_t* stepp, int max_len, const float* ln_sg,
                                                         const float* ln_sb, float ln_eps) {
  if (stepp && *stepp > max_len) return;
  using f32x4v = __attribute__((ext_vector_type(4))) float;
  __shared__ float red[NW][NT * TT][64][4];
  __shared__ float stat[LN ? NW : 1][TT][16][2];
  float s1[TT], s2[TT];
#pragma unroll
  for (int i = 0; i < TT; ++i) s1[i] = s2[i] = 0.0f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, c = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT), t0 = blockIdx.y * (16 * TT);
  const int kq = K / NW;  // this wave's K range: [wave * kq, (wave + 1) * kq)
  const bf16_t* wp[NT];
  const bf16_t* xp[TT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    int n = n0 + 16 * j + r;
    n = n < N ? n : N - 1;
    wp[j] = W + (int64_t)n * K + wave * kq + c * 8;
  }
#pragma unroll
  for (int i = 0; i < TT; ++i) {
    int t = t0 + 16 * i + r;
    t = t < M ? t : M - 1;
    xp[i] = x + (int64_t)t * ldx + wave * kq + c * 8;
  }
  f32x4v acc[NT][TT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < TT; ++i) acc[j][i] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
  bf16x8 wv[UN][NT], wn[UN][NT], xv[UN][TT];
#pragma unroll
  for (int u = 0; u < UN; ++u)
#pragma unroll
    for (int j = 0; j < NT; ++j) wn[u][j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp[j] + 32 * u));
  for (int k = 0; k < kq; k += 32 * UN) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
#pragma unroll
      for (int j = 0; j < NT; ++j) wv[u][j] = wn[u][j];
#pragma unroll
      for (int i = 0; i < TT; ++i) xv[u][i] = *reinterpret_cast<const bf16x8*>(xp[i] + k + 32 * u);
    }
    if (k + 32 * UN < kq) {
#pragma unroll
      for (int u = 0; u < UN; ++u)
#pragma unroll
        for (int j = 0; j < NT; ++j) wn[u][j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp[j] + k + 32 * UN + 32 * u));
    }
#pragma unroll
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < TT; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[u][j], xv[u][i], acc[j][i], 0, 0, 0);
    if (LN) {
#pragma unroll
      for (int u = 0; u < UN; ++u)
#pragma unroll
        for (int i = 0; i < TT; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = static_cast<float>(xv[u][i][e]);
            s1[i] += f;
            s2[i] = fmaf(f, f, s2[i]);
          }
    }
  }
  if (LN) {  // row sums: over the four k-chunk lane groups of this wave, then (below) over the four waves' K quarters, in a fixed order
#pragma unroll
    for (int i = 0; i < TT; ++i) {
      s1[i] += __shfl_xor(s1[i], 16, 64); s2[i] += __shfl_xor(s2[i], 16, 64);
      s1[i] += __shfl_xor(s1[i], 32, 64); s2[i] += __shfl_xor(s2[i], 32, 64);
      if (c == 0) { stat[wave][i][r][0] = s1[i]; stat[wave][i][r][1] = s2[i]; }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave][j * TT + i][lane][e] = acc[j][i][e];
  __syncthreads();
  for (int tile = wave; tile < NT * TT; tile += NW) {
    const int j = tile / TT, i = tile % TT;
    const int n = n0 + 16 * j + 4 * c, t = t0 + 16 * i + r;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = red[0][tile][lane][e];
#pragma unroll
      for (int w = 1; w < NW; ++w) a += red[w][tile][lane][e];  // wave order: deterministic
      v[e] = a;
    }
    if (t >= M || n >= N) continue;
    float mean = 0.0f, rstd = 1.0f;
    if (LN) {
      float a = stat[0][i][r][0], b2 = stat[0][i][r][1];
#pragma unroll
      for (int w = 1; w < NW; ++w) { a += stat[w][i][r][0]; b2 += stat[w][i][r][1]; }
      mean = a / (float)K;
      const float var = fmaxf(b2 / (float)K - mean * mean, 0.0f);
      rstd = rsqrtf(var + ln_eps);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (n + e < N) {
        float o = LN ? fmaf(rstd, v[e] - mean * ln_sg[n + e], ln_sb[n + e]) : v[e] + (bias ? DT<bf16_t>::ld(bias + n + e) : 0.0f);
        o = act_t<bf16_t>(o, act);
        if (resid) o += DT<bf16_t>::ld(resid + (int64_t)t * ldr + n + e);
        v[e] = o;
      }
    }
    bf16_t* dst = y + (int64_t)t * ldy + n;
    if (n + 4 <= N && ((ldy | n) & 3) == 0) {
      typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
      bf16x4_t pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = static_cast<__bf16>(v[e]);
      *reinterpret_cast<bf16x4_t*>(dst) = pk;
    } else {
      for (int e = 0; e < 4 && n + e < N; ++e) DT<bf16_t>::st(dst + e, v[e]);
    }
  }
}

}  // namespace

extern "C" {
static int dec_linear_impl(const void* x, const void* W, const void* bias, const void* resid, void* y, int64_t M, int64_t N, int64_t K,
                           int64_t ldx, int64_t ld_resid, int64_t ldy, int act, const int32_t* step, int64_t max_len, int dtype,
                           const float* ln_sg, const float* ln_sb, float ln_eps, cst_stream stream) {
  CST_REQUIRE(x && W && y && M > 0 && N > 0 && K > 0, "cst_dec_linear: bad args");
  CST_REQUIRE(dtype == CST_BF16, "cst_dec_linear: bf16 only (fp32 problems go through cst_gemm)");
  CST_REQUIRE(K % 512 == 0 && ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)W % 16) == 0, "cst_dec_linear: K %% 512 == 0 and 16-byte aligned rows required (K=%lld)", (long long)K);
  CST_REQUIRE(M <= 4096, "cst_dec_linear: a decode-step kernel (M=%lld rows)", (long long)M);
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_GEMM, s, 2.0 * M * N * K, 2.0 * ((double)N * K + (double)M * K + (double)M * N));
  const int ty = (int)cst_ceil_div(M, 80);
  const int64_t wg1 = cst_ceil_div(N, 16) * ty;
  const bool ln = ln_sg != nullptr;
  // Waves per workgroup = how finely K is cut: each wave should have one or two batches of UN k-steps (32 columns each), so that
  // nearly all of its weight bytes are requested at once.  Enough workgroups to have every CU pulling weights, few enough that the
  // shared x rows are not re-read from L2 more than needed.
  static const int env_nw = getenv("CST_DEC_LINEAR_NW") ? atoi(getenv("CST_DEC_LINEAR_NW")) : 0;
  int nw = 8;  // measured (tools/bench_dec_linear.py): 8 waves 10.2 / 8.1 / 10.3 us on the three LayerNorm-fused shapes, 4 waves 10.9 / 8.6 / 11.0; 16 no better
  if (env_nw == 4 || env_nw == 8 || env_nw == 16) nw = env_nw;
  while (nw > 4 && K % (nw * 64) != 0) nw >>= 1;
  const int steps = (int)(K / nw / 32);  // k-steps per wave
#define CST_DL(NTv, UNv, LNv, NWv)                                                                                                  \
  hipLaunchKernelGGL((dec_linear_kernel<NTv, 5, UNv, LNv, NWv>), dim3((unsigned)cst_ceil_div(N, 16 * NTv), (unsigned)ty), dim3(NWv * 64), 0, s, \
                     (const bf16_t*)x, (const bf16_t*)W, (const bf16_t*)bias, (const bf16_t*)resid, (bf16_t*)y, (int)M, (int)N, (int)K, ldx, \
                     ld_resid, ldy, act, step, (int)max_len, ln_sg, ln_sb, ln_eps)
#define CST_DL_LN(NTv, UNv, NWv) do { if (ln) CST_DL(NTv, UNv, true, NWv); else CST_DL(NTv, UNv, false, NWv); } while (0)
  if (wg1 <= 320) {  // one 16-column tile per workgroup
    if (nw == 16) { if (steps % 4 == 0) CST_DL_LN(1, 4, 16); else CST_DL_LN(1, 2, 16); }
    else if (nw == 8) { if (steps % 4 == 0) CST_DL_LN(1, 4, 8); else CST_DL_LN(1, 2, 8); }
    else CST_DL_LN(1, 4, 4);
  } else if (wg1 <= 1024) {  // two column tiles; the wave-partial image of 16 waves would not fit the LDS
    const int nw2 = nw == 16 ? 8 : nw, steps2 = (int)(K / nw2 / 32);
    if (nw2 == 8) { if (steps2 % 4 == 0) CST_DL_LN(2, 4, 8); else CST_DL_LN(2, 2, 8); }
    else CST_DL_LN(2, 4, 4);
  } else {
    CST_DL_LN(4, 2, 4);
  }
#undef CST_DL_LN
#undef CST_DL
  return cst_check_launch("cst_dec_linear");
}

int cst_dec_linear(const void* x, const void* W, const void* bias, const void* resid, void* y, int64_t M, int64_t N, int64_t K,
                   int64_t ldx, int64_t ld_resid, int64_t ldy, int act, const int32_t* step, int64_t max_len, int dtype,
                   cst_stream stream) {
  return dec_linear_impl(x, W, bias, resid, y, M, N, K, ldx, ld_resid, ldy, act, step, max_len, dtype, nullptr, nullptr, 0.0f, stream);
}

int cst_dec_ln_linear(const void* x, const void* Wg, const float* sg, const float* sb, float eps, const void* resid, void* y, int64_t M,
                      int64_t N, int64_t K, int64_t ldx, int64_t ld_resid, int64_t ldy, int act, const int32_t* step, int64_t max_len,
                      int dtype, cst_stream stream) {
  CST_REQUIRE(sg && sb && eps > 0.0f, "cst_dec_ln_linear: the folded LayerNorm vectors are required");
  return dec_linear_impl(x, Wg, nullptr, resid, y, M, N, K, ldx, ld_resid, ldy, act, step, max_len, dtype, sg, sb, eps, stream);
}

int cst_dec_embed(const int64_t* tokens, const int32_t* step, const void* embed, const float* pos_table, float scale,
                  int64_t pad_idx, void* out, int64_t rows, int64_t C, int64_t max_len, int64_t pos_rows, int dtype,
                  cst_stream stream) {
  CST_REQUIRE(tokens && step && embed && pos_table && out, "cst_dec_embed: null operand");
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_dec_embed: bad dtype %d", dtype);
  CST_REQUIRE(rows > 0 && C > 0 && max_len >= 1 && pos_rows > pad_idx + 1, "cst_dec_embed: bad shape");
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_ELEMENTWISE, s, 0.0, (double)rows * C * (2.0 * cst_dtype_size(dtype) + 4.0));
  if (dtype == CST_BF16)
    hipLaunchKernelGGL(dec_embed_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, s, tokens, step, (const bf16_t*)embed, pos_table, scale,
                       (int)pad_idx, (bf16_t*)out, (int)rows, (int)C, (int)max_len, (int)pos_rows);
  else
    hipLaunchKernelGGL(dec_embed_kernel<float>, dim3((unsigned)rows), dim3(256), 0, s, tokens, step, (const float*)embed, pos_table, scale,
                       (int)pad_idx, (float*)out, (int)rows, (int)C, (int)max_len, (int)pos_rows);
  return cst_check_launch("cst_dec_embed");
}

int cst_dec_self_attn(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const int32_t* step, void* out,
                      int64_t rows, int64_t H, int64_t D, int64_t max_len, float scale, int dtype, cst_stream stream) {
  CST_REQUIRE(qkv && kcache && vcache && anc && step && out, "cst_dec_self_attn: null operand");
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_dec_self_attn: bad dtype %d", dtype);
  CST_REQUIRE(D == 32 || D == 64, "cst_dec_self_attn: head dim %lld not in {32,64}", (long long)D);
  CST_REQUIRE(rows > 0 && H > 0 && max_len >= 1 && max_len <= 4000, "cst_dec_self_attn: bad shape (max_len <= 4000)");
  hipStream_t s = (hipStream_t)stream;
  const int WPB = 4;
  const unsigned blocks = (unsigned)cst_ceil_div(rows * H, WPB);
  const size_t lds = 0;
  CstProfScope prof(CST_K_ATTN_FWD, s, 4.0 * rows * H * D * (max_len + 1) * 0.5, 0.0);
#define CST_DSA(T, DD) hipLaunchKernelGGL((dec_self_attn_kernel<T, DD>), dim3(blocks), dim3(64 * WPB), lds, s, (const T*)qkv, (T*)kcache, (T*)vcache, \
                                          anc, step, (T*)out, (int)rows, (int)H, (int)max_len, scale)
  if (dtype == CST_BF16) { if (D == 64) CST_DSA(bf16_t, 64); else CST_DSA(bf16_t, 32); }
  else { if (D == 64) CST_DSA(float, 64); else CST_DSA(float, 32); }
#undef CST_DSA
  return cst_check_launch("cst_dec_self_attn");
}

int cst_dec_cross_attn(const void* q, const void* kx, const void* vx, const uint8_t* key_padding_mask, void* out,
                       const int32_t* step, int64_t max_len, int64_t bsz, int64_t beam, int64_t H, int64_t D, int64_t S, float scale,
                       int dtype, cst_stream stream) {
  CST_REQUIRE(q && kx && vx && out && step, "cst_dec_cross_attn: null operand");
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_dec_cross_attn: bad dtype %d", dtype);
  CST_REQUIRE(D == 32 || D == 64, "cst_dec_cross_attn: head dim %lld not in {32,64}", (long long)D);
  CST_REQUIRE(bsz > 0 && beam > 0 && H > 0 && S > 0, "cst_dec_cross_attn: bad shape");
  hipStream_t s = (hipStream_t)stream;
  // bf16 / head dim 64 / at most 32 hypotheses per sentence: the matrix-core kernel whose four waves split the keys (attention_fast.inc);
  // CST_DEC_CROSS_VALU=1 keeps the VALU kernel below (A/B runs)
  static const bool valu_only = getenv("CST_DEC_CROSS_VALU") != nullptr;
  if (!valu_only && dtype == CST_BF16 && D == 64 && beam <= 32 && S * 128 < (1ll << 31) && ((uintptr_t)q % 16 == 0) && ((uintptr_t)kx % 16 == 0) &&
      ((uintptr_t)vx % 16 == 0) && ((uintptr_t)out % 16 == 0)) {
    CstProfScope prof(CST_K_ATTN_FWD, s, 4.0 * bsz * beam * H * D * S, 2.0 * bsz * S * H * D * cst_dtype_size(dtype));
    const int rc = cst_fa_dec_cross(q, kx, vx, key_padding_mask, out, step, max_len, bsz, beam, H, S, scale, nullptr, nullptr, nullptr, 0.0f, 0, 0, s);
    return rc != CST_OK ? rc : cst_check_launch("cst_dec_cross_attn");
  }
  const int BQ = beam == 1 ? 1 : (beam <= 5 ? 5 : 8);
  // waves per workgroup = slices the key range is cut into (each wave streams its own keys; more waves = more loads in flight)
  static const int env_nw = getenv("CST_DEC_CROSS_NW") ? atoi(getenv("CST_DEC_CROSS_NW")) : 0;
  const int NWv = env_nw == 8 ? 8 : 4;  // 8 measured no faster end to end (and the flash kernel remains the engine's default: 0.198 vs 0.230 s per batch)
  const size_t lds = ((size_t)2 * NWv * BQ + (size_t)NWv * BQ * D + (size_t)BQ * D) * sizeof(float);
  CstProfScope prof(CST_K_ATTN_FWD, s, 4.0 * bsz * beam * H * D * S, 2.0 * bsz * S * H * D * cst_dtype_size(dtype));
#define CST_DCA_W(T, DD, QQ, WW)                                                                                                \
  do {                                                                                                                          \
    static bool attr = false;                                                                                                   \
    if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_cross_attn_kernel<T, DD, QQ, WW>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); attr = true; } \
    hipLaunchKernelGGL((dec_cross_attn_kernel<T, DD, QQ, WW>), dim3((unsigned)(bsz * H)), dim3(WW * 64), lds, s, (const T*)q, (const T*)kx, (const T*)vx, \
                       key_padding_mask, (T*)out, step, (int)max_len, (int)beam, (int)H, (int)S, scale);                       \
  } while (0)
#define CST_DCA(T, DD, QQ) do { if (NWv == 8) CST_DCA_W(T, DD, QQ, 8); else CST_DCA_W(T, DD, QQ, 4); } while (0)
#define CST_DCA_Q(T, DD) do { if (BQ == 1) CST_DCA(T, DD, 1); else if (BQ == 5) CST_DCA(T, DD, 5); else CST_DCA(T, DD, 8); } while (0)
  if (dtype == CST_BF16) { if (D == 64) CST_DCA_Q(bf16_t, 64); else CST_DCA_Q(bf16_t, 32); }
  else { if (D == 64) CST_DCA_Q(float, 64); else CST_DCA_Q(float, 32); }
#undef CST_DCA_Q
#undef CST_DCA
#undef CST_DCA_W
  return cst_check_launch("cst_dec_cross_attn");
}

int cst_dec_ln_q_cross_attn(const void* x, int64_t ldx, const void* Wg, const float* sg, const float* sb, float eps, const void* kx, const void* vx,
                            const uint8_t* key_padding_mask, void* out, const int32_t* step, int64_t max_len, int64_t bsz, int64_t beam, int64_t H,
                            int64_t D, int64_t S, float scale, int dtype, cst_stream stream) {
  CST_REQUIRE(x && Wg && sg && sb && kx && vx && out && step, "cst_dec_ln_q_cross_attn: null operand");
  CST_REQUIRE(dtype == CST_BF16 && D == 64 && beam > 0 && beam <= 32, "cst_dec_ln_q_cross_attn: bf16, head dim 64, beam <= 32 (the unfused pair covers the rest)");
  CST_REQUIRE(bsz > 0 && H > 0 && S > 0 && S * 128 < (1ll << 31), "cst_dec_ln_q_cross_attn: bad shape");
  const int64_t K = H * D;  // the query projection is square: embed_dim -> H * D
  CST_REQUIRE(K % 256 == 0 && ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)Wg % 16) == 0 && ((uintptr_t)sg % 16) == 0 && ((uintptr_t)sb % 16) == 0 &&
                  ((uintptr_t)kx % 16) == 0 && ((uintptr_t)vx % 16) == 0 && ((uintptr_t)out % 16) == 0,
              "cst_dec_ln_q_cross_attn: embed dim %% 256 == 0 and 16-byte aligned operands required");
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_ATTN_FWD, s, 4.0 * bsz * beam * H * D * S + 2.0 * bsz * beam * K * K, 2.0 * bsz * S * H * D * 2 + 2.0 * K * K);
  const int rc = cst_fa_dec_cross(x, kx, vx, key_padding_mask, out, step, max_len, bsz, beam, H, S, scale, Wg, sg, sb, eps, K, ldx, s);
  return rc != CST_OK ? rc : cst_check_launch("cst_dec_ln_q_cross_attn");
}

}  // extern "C"
