// ln_gelu.hip — the wav2vec2 feature extractor in extractor_mode="layer_norm" (the published large models): every conv layer is
// followed by a LayerNorm over the C channels of a frame (Fp32LayerNorm: fp32 statistics) and GELU,
// fairseq/models/wav2vec/wav2vec2.py:714-724.
//
//   cst_conv0_ln_gelu_fwd/bwd : layer 0, Conv1d(1 -> C, k, stride, bias) + LayerNorm(C) + GELU from the raw samples.  The statistics are
//                               per FRAME over the channels, and one wave64 holds all C <= 512 channels of a frame (8 per lane), so
//                               the forward is ONE pass: read the samples once, write B L C elements once; the pre-norm conv output
//                               never reaches HBM and the backward recomputes it from the samples.
//   cst_ln_gelu_fwd/bwd       : layers 1.., y = GELU(LayerNorm_C(u)) over channels-last rows, u = the implicit-GEMM conv output with
//                               bias.  One wave64 per row, 16-byte accesses, as layernorm.hip.
// All reductions over frames (dW, dbias, dgamma, dbeta) go through per-block partials that are added in a fixed order: no atomics,
// bit-reproducible run to run.
#include "cst_common.h"

namespace {

constexpr int LG_WAVES = 4;  // waves per block: one frame / row per wave at a time

// =====================================================================================================================
// layer 0
// =====================================================================================================================
constexpr int C0L_KMAX = 16;
constexpr int C0L_TB = 128;       // frames per block, forward
constexpr int C0L_BWD_TB = 2048;  // frames per block, backward (one partial row set per block)

// lane -> channels 8 lane .. 8 lane + 7 (lanes at or past C / 8 idle: their values are zeros and add nothing to the wave sums)
template <typename T, int KC>
__device__ __forceinline__ void c0l_load_params(const T* w, const T* bias, const T* gamma, const T* beta, int C, int k, int lane,
                                                float (&wr)[KC][8], float (&bi)[8], float (&ga)[8], float (&be)[8]) {
  const bool on = lane * 8 < C;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = lane * 8 + e;
    bi[e] = on ? DT<T>::ld(bias + c) : 0.0f;
    ga[e] = on ? DT<T>::ld(gamma + c) : 0.0f;
    be[e] = on ? DT<T>::ld(beta + c) : 0.0f;
#pragma unroll
    for (int j = 0; j < KC; ++j) wr[j][e] = (on && j < k) ? DT<T>::ld(w + (int64_t)c * k + j) : 0.0f;
  }
}

// frames [t0, t0 + nt) of utterance b: samples [t0 stride, (t0 + nt - 1) stride + k) into LDS, zeros up to `total` (padded taps read them)
__device__ __forceinline__ void c0l_stage(const float* wav, float* sx, int64_t b, int64_t S, int64_t t0, int nt, int k, int stride, int total) {
  const int span = nt > 0 ? (nt - 1) * stride + k : 0;
  for (int i = threadIdx.x; i < total; i += blockDim.x) sx[i] = i < span ? wav[b * S + t0 * stride + i] : 0.0f;
}

template <typename T, int KC>
__global__ __launch_bounds__(LG_WAVES * 64) void conv0_ln_fwd_kernel(const float* wav, const T* w, const T* bias, const T* gamma, const T* beta,
                                                                    T* y, float* mean, float* rstd, int64_t S, int64_t L, int C, int k,
                                                                    int stride, float eps, const int32_t* flim) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int64_t b = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * C0L_TB;
  const int64_t Lb = (flim && flim[b] < L) ? (flim[b] > 0 ? flim[b] : 0) : L;  // frames from flim[b] on: neither computed nor written
  if (t0 >= Lb) return;
  const int nt = (int)((Lb - t0 < C0L_TB) ? (Lb - t0) : C0L_TB);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wr[KC][8], bi[8], ga[8], be[8];
  c0l_load_params<T, KC>(w, bias, gamma, beta, C, k, lane, wr, bi, ga, be);
  c0l_stage(wav, sm, b, S, t0, nt, k, stride, (C0L_TB - 1) * stride + KC);
  __syncthreads();
  const bool on = lane * 8 < C;
  const float inv_c = 1.0f / (float)C;
  for (int tl = wave; tl < nt; tl += LG_WAVES) {
    float u[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] = bi[e];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const float xv = sm[tl * stride + j];
#pragma unroll
      for (int e = 0; e < 8; ++e) u[e] = fmaf(wr[j][e], xv, u[e]);
    }
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += u[e];  // (idle lanes: bias = w = 0 -> u = 0)
    const float mu = wave_sum(s) * inv_c;
    float q = 0.0f;
    if (on) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = u[e] - mu; q = fmaf(d, d, q); }
    }
    const float rs = rsqrtf(wave_sum(q) * inv_c + eps);
    if (on) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = gelu_t<T>(fmaf((u[e] - mu) * rs, ga[e], be[e]));
      store8(y + ((b * L + t0 + tl) * (int64_t)C + lane * 8), o);
    }
    if (lane == 0) { mean[b * L + t0 + tl] = mu; rstd[b * L + t0 + tl] = rs; }
  }
}

// partials: ws [B][nblk][k + 3][C]: row 0 = dgamma, 1 = dbeta, 2 = dbias, 3 + j = dW[:, j]
template <typename T, int KC>
__global__ __launch_bounds__(LG_WAVES * 64) void conv0_ln_bwd_kernel(const T* dy, const float* wav, const T* w, const T* bias, const T* gamma,
                                                                    const T* beta, const float* mean, const float* rstd, float* ws,
                                                                    int64_t S, int64_t L, int C, int k, int stride, const int32_t* blim) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int64_t b = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * C0L_BWD_TB;
  const int64_t Lb = (blim && blim[b] < L) ? blim[b] : L;  // dy is exactly zero from frame blim[b] on: those frames add nothing
  const int64_t left = Lb - t0;
  const int nt = left <= 0 ? 0 : (int)(left < C0L_BWD_TB ? left : C0L_BWD_TB);  // 0: the block only writes its zero partials
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wr[KC][8], bi[8], ga[8], be[8];
  c0l_load_params<T, KC>(w, bias, gamma, beta, C, k, lane, wr, bi, ga, be);
  c0l_stage(wav, sm, b, S, t0, nt, k, stride, (C0L_BWD_TB - 1) * stride + KC);
  __syncthreads();
  const bool on = lane * 8 < C;
  const float inv_c = 1.0f / (float)C;
  float dg[8], db[8], dbi[8], dwa[KC][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    dg[e] = 0.0f; db[e] = 0.0f; dbi[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < KC; ++j) dwa[j][e] = 0.0f;
  }
  for (int tl = wave; tl < nt; tl += LG_WAVES) {
    const int64_t fr = b * L + t0 + tl;
    float d[8], u[8], xv[KC];
#pragma unroll
    for (int e = 0; e < 8; ++e) { d[e] = 0.0f; u[e] = bi[e]; }
    if (on) load8(dy + (fr * (int64_t)C + lane * 8), d);
    const float mu = mean[fr], rs = rstd[fr];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      xv[j] = sm[tl * stride + j];
#pragma unroll
      for (int e = 0; e < 8; ++e) u[e] = fmaf(wr[j][e], xv[j], u[e]);
    }
    float xh[8], g[8], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xh[e] = on ? (u[e] - mu) * rs : 0.0f;
      const float dz = d[e] * dgelu_t<T>(fmaf(xh[e], ga[e], be[e]));  // (idle lanes: d = 0)
      dg[e] = fmaf(dz, xh[e], dg[e]);
      db[e] += dz;
      g[e] = dz * ga[e];
      s1 += g[e];
      s2 = fmaf(g[e], xh[e], s2);
    }
    s1 = wave_sum(s1) * inv_c;
    s2 = wave_sum(s2) * inv_c;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float du = on ? rs * (g[e] - s1 - xh[e] * s2) : 0.0f;
      dbi[e] += du;
#pragma unroll
      for (int j = 0; j < KC; ++j) dwa[j][e] = fmaf(du, xv[j], dwa[j][e]);
    }
  }
  // the block's four waves, added in wave order through LDS (one row of the accumulator set at a time), one store per value
  __syncthreads();  // (everybody is done with the staged samples)
  float* const o = ws + (b * gridDim.x + blockIdx.x) * (int64_t)(k + 3) * C;
#pragma unroll
  for (int row = 0; row < KC + 3; ++row) {
    if (row < k + 3) {  // block-uniform
      float* mine = sm + (size_t)threadIdx.x * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) mine[e] = row == 0 ? dg[e] : (row == 1 ? db[e] : (row == 2 ? dbi[e] : dwa[row >= 3 ? row - 3 : 0][e]));
      __syncthreads();
      if (wave == 0 && on) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = 0.0f;
#pragma unroll
          for (int q = 0; q < LG_WAVES; ++q) v += sm[(size_t)(q * 64 + lane) * 8 + e];
          o[(int64_t)row * C + lane * 8 + e] = v;
        }
      }
      __syncthreads();
    }
  }
}

// fixed-order sum of all block partials: part [n][rows][C] -> out [rows][C]; four interleaved chains p = i, i + 4, ... per thread, added
// 0..3 (the loads of a chain do not wait for each other's adds)
// (o0 / o1 / o2 non-NULL: rows 0 / 1 / 2 go to those vectors instead of out)
__global__ void lg_reduce_kernel(const float* part, float* out, int n, int rows, int C, float* o0, float* o1, float* o2) {
  const int row = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int q0 = 0; q0 < n; q0 += 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (q0 + i < n) a[i] += part[((int64_t)(q0 + i) * rows + row) * C + c];
  }
  const float v = (a[0] + a[1]) + (a[2] + a[3]);
  float* const o = row == 0 ? o0 : (row == 1 ? o1 : (row == 2 ? o2 : nullptr));
  if (o) o[c] = v;
  else if (out) out[(int64_t)row * C + c] = v;
}

// out [k + 3][C] -> dgamma, dbeta, dbias [C], dw [C][k]
__global__ void conv0_ln_scatter_kernel(const float* acc, float* dw, float* dbias, float* dgamma, float* dbeta, int C, int k) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dgamma[c] = acc[c];
  dbeta[c] = acc[C + c];
  dbias[c] = acc[2 * C + c];
  for (int j = 0; j < k; ++j) dw[(int64_t)c * k + j] = acc[(int64_t)(3 + j) * C + c];
}

// =====================================================================================================================
// layers 1..: rows [B][L][C], one wave per row, NV 8-element vectors per lane
// =====================================================================================================================
constexpr int LG_MAXV = 4;  // C <= 2048

template <typename T, int NV>
__global__ __launch_bounds__(LG_WAVES * 64) void ln_gelu_fwd_kernel(const T* u, const T* gamma, const T* beta, T* y, float* mean, float* rstd,
                                                                   const int32_t* lim, int64_t B, int64_t L, int C, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C / 8;
  const int64_t rows = B * L;
  float ga[NV][8], be[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (lane + 64 * i < nvec) { load8(gamma + (lane + 64 * i) * 8, ga[i]); load8(beta + (lane + 64 * i) * 8, be[i]); }
  const float inv_c = 1.0f / (float)C;
  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < rows; row += (int64_t)gridDim.x * LG_WAVES) {
    const int64_t b = (uint32_t)row / (uint32_t)L, t = row - b * L;  // (rows < 2^31: checked by the caller)
    if (lim && t >= lim[b]) {  // (wave-uniform) a row nobody reads: not read, not computed; zeros, so that whoever meets it meets a number
      const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (lane + 64 * i < nvec) store8(y + row * C + (lane + 64 * i) * 8, z);
      if (lane == 0) { mean[row] = 0.0f; rstd[row] = 0.0f; }
      continue;
    }
    float v[NV][8];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) {
        load8(u + row * C + (lane + 64 * i) * 8, v[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[i][e];
      }
    const float mu = wave_sum(s) * inv_c;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mu; q = fmaf(d, d, q); }
      }
    const float rs = rsqrtf(wave_sum(q) * inv_c + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = gelu_t<T>(fmaf((v[i][e] - mu) * rs, ga[i][e], be[i][e]));
        store8(y + row * C + (lane + 64 * i) * 8, o);
      }
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  }
}

// du = rstd (g - mean(g) - xhat mean(g xhat)), g = dy GELU'(xhat gamma + beta) gamma; partials [nblocks][3][C]: dgamma, dbeta, colsum(du)
template <typename T, int NV>
__global__ __launch_bounds__(LG_WAVES * 64) void ln_gelu_bwd_kernel(const T* dy, const T* u, const T* gamma, const T* beta, const float* mean,
                                                                   const float* rstd, T* du, int64_t du_bstride, float* part,
                                                                   const int32_t* lim, int64_t B, int64_t L, int C) {
  __shared__ float red[LG_WAVES][64 * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C / 8;
  const int64_t rows = B * L;
  float ga[NV][8], be[NV][8], dg[NV][8], db[NV][8], dc[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { dg[i][e] = 0.0f; db[i][e] = 0.0f; dc[i][e] = 0.0f; ga[i][e] = 0.0f; be[i][e] = 0.0f; }
    if (lane + 64 * i < nvec) { load8(gamma + (lane + 64 * i) * 8, ga[i]); load8(beta + (lane + 64 * i) * 8, be[i]); }
  }
  const float inv_c = 1.0f / (float)C;
  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < rows; row += (int64_t)gridDim.x * LG_WAVES) {
    const int64_t b = (uint32_t)row / (uint32_t)L, t = row - b * L;
    T* const dur = du + b * du_bstride + t * C;
    if (lim && t >= lim[b]) {  // dy is exactly zero here, and so is du: written, nothing read
      const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (lane + 64 * i < nvec) store8(dur + (lane + 64 * i) * 8, z);
      continue;
    }
    const float mu = mean[row], rs = rstd[row];
    float g[NV][8], xh[NV][8];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) {
        float d[8], x[8];
        load8(dy + row * C + (lane + 64 * i) * 8, d);
        load8(u + row * C + (lane + 64 * i) * 8, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[i][e] = (x[e] - mu) * rs;
          const float dz = d[e] * dgelu_t<T>(fmaf(xh[i][e], ga[i][e], be[i][e]));
          dg[i][e] = fmaf(dz, xh[i][e], dg[i][e]);
          db[i][e] += dz;
          g[i][e] = dz * ga[i][e];
          s1 += g[i][e];
          s2 = fmaf(g[i][e], xh[i][e], s2);
        }
      }
    s1 = wave_sum(s1) * inv_c;
    s2 = wave_sum(s2) * inv_c;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          o[e] = rs * (g[i][e] - s1 - xh[i][e] * s2);
          dc[i][e] += o[e];
        }
        store8(dur + (lane + 64 * i) * 8, o);
      }
  }
  // the block's waves in wave order, one vector slot and one quantity at a time
  float* const p = part + (int64_t)blockIdx.x * 3 * C;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = pass == 0 ? dg[i][e] : (pass == 1 ? db[i][e] : dc[i][e]);
      __syncthreads();
      if (wave == 0 && lane + 64 * i < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float a = 0.0f;
#pragma unroll
          for (int q = 0; q < LG_WAVES; ++q) a += red[q][lane * 8 + e];
          p[(int64_t)pass * C + (lane + 64 * i) * 8 + e] = a;
        }
      }
    }
  }
}

int lg_blocks(int64_t rows, int cap) {
  const int64_t b = cst_ceil_div(rows, LG_WAVES);
  return (int)(b < cap ? b : cap);
}
constexpr int LG_FWD_BLOCKS = 4096, LG_BWD_BLOCKS = 1024;
inline int lg_nv(int64_t C) { return C <= 512 ? 1 : (C <= 1024 ? 2 : 4); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int cst_conv0_ln_gelu_fwd(const float* wav, const void* w, const void* bias, const void* gamma, const void* beta, void* y,
                                     float* mean, float* rstd, const int32_t* frame_limit, int64_t B, int64_t S, int64_t C, int k,
                                     int stride, float eps, int dtype, cst_stream stream) {
  CST_REQUIRE(wav && w && bias && gamma && beta && y && mean && rstd, "cst_conv0_ln_gelu_fwd: null tensor");
  CST_REQUIRE(k >= 1 && k <= C0L_KMAX && stride >= 1 && stride <= 7 && S >= k, "cst_conv0_ln_gelu_fwd: unsupported k=%d stride=%d S=%lld (k <= 16, stride <= 7)", k, stride, (long long)S);
  CST_REQUIRE(C % 8 == 0 && C >= 8 && C <= 512, "cst_conv0_ln_gelu_fwd: C=%lld must be a multiple of 8 and <= 512 (one wave holds a frame)", (long long)C);
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_conv0_ln_gelu_fwd: bad dtype %d", dtype);
  CST_REQUIRE(B > 0 && B <= 65535, "cst_conv0_ln_gelu_fwd: B=%lld", (long long)B);
  const int64_t L = (S - k) / stride + 1;
  hipStream_t s = (hipStream_t)stream;
  const double bytes = (double)B * S * 4.0 + (double)B * L * C * cst_dtype_size(dtype);
  CstProfScope prof(CST_K_CONV0, s, 2.0 * (double)B * L * C * k, bytes);
  const dim3 grid((unsigned)cst_ceil_div(L, C0L_TB), (unsigned)B);
#define CST_C0LF(T, KC) hipLaunchKernelGGL((conv0_ln_fwd_kernel<T, KC>), grid, dim3(LG_WAVES * 64), sizeof(float) * ((size_t)(C0L_TB - 1) * stride + KC), s, wav, (const T*)w, (const T*)bias, (const T*)gamma, (const T*)beta, (T*)y, mean, rstd, S, L, (int)C, k, stride, eps, frame_limit)
  if (dtype == CST_BF16) { if (k == 10) CST_C0LF(bf16_t, 10); else CST_C0LF(bf16_t, C0L_KMAX); }
  else { if (k == 10) CST_C0LF(float, 10); else CST_C0LF(float, C0L_KMAX); }
#undef CST_C0LF
  return cst_check_launch("cst_conv0_ln_gelu_fwd");
}

static int64_t conv0_ln_bwd_blocks(int64_t L) { return cst_ceil_div(L, C0L_BWD_TB); }

/* [B][nblk][k + 3][C] block partials followed by the reduced [k + 3][C] */
extern "C" int64_t cst_conv0_ln_bwd_workspace(int64_t B, int64_t S, int64_t C, int k, int stride) {
  const int64_t L = S >= k ? (S - k) / stride + 1 : 0;
  return (B * conv0_ln_bwd_blocks(L) + 1) * (int64_t)(k + 3) * C * (int64_t)sizeof(float);
}

extern "C" int cst_conv0_ln_gelu_bwd(const void* dy, const float* wav, const void* w, const void* bias, const void* gamma, const void* beta,
                                     const float* mean, const float* rstd, float* dw, float* dbias, float* dgamma, float* dbeta,
                                     float* workspace, const int32_t* frame_limit, int64_t B, int64_t S, int64_t C, int k, int stride,
                                     int dtype, cst_stream stream) {
  CST_REQUIRE(dy && wav && w && bias && gamma && beta && mean && rstd && dw && dbias && dgamma && dbeta && workspace, "cst_conv0_ln_gelu_bwd: null tensor");
  CST_REQUIRE(k >= 1 && k <= C0L_KMAX && stride >= 1 && stride <= 7 && S >= k, "cst_conv0_ln_gelu_bwd: unsupported k=%d stride=%d (k <= 16, stride <= 7)", k, stride);
  CST_REQUIRE(C % 8 == 0 && C >= 8 && C <= 512, "cst_conv0_ln_gelu_bwd: C=%lld must be a multiple of 8 and <= 512", (long long)C);
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "cst_conv0_ln_gelu_bwd: bad dtype %d", dtype);
  CST_REQUIRE(B > 0 && B <= 65535, "cst_conv0_ln_gelu_bwd: B=%lld", (long long)B);
  const int64_t L = (S - k) / stride + 1;
  hipStream_t s = (hipStream_t)stream;
  const double bytes = (double)B * S * 4.0 + (double)B * L * C * cst_dtype_size(dtype);
  CstProfScope prof(CST_K_CONV0, s, 4.0 * (double)B * L * C * k, bytes);
  const int nblk = (int)conv0_ln_bwd_blocks(L);
  float* acc = workspace + (size_t)B * nblk * (k + 3) * C;
  size_t lds = sizeof(float) * ((size_t)(C0L_BWD_TB - 1) * stride + C0L_KMAX);
  if (lds < sizeof(float) * LG_WAVES * 64 * 8) lds = sizeof(float) * LG_WAVES * 64 * 8;
  const dim3 grid((unsigned)nblk, (unsigned)B);
#define CST_C0LB(T, KC) hipLaunchKernelGGL((conv0_ln_bwd_kernel<T, KC>), grid, dim3(LG_WAVES * 64), lds, s, (const T*)dy, wav, (const T*)w, (const T*)bias, (const T*)gamma, (const T*)beta, mean, rstd, workspace, S, L, (int)C, k, stride, frame_limit)
  if (dtype == CST_BF16) { if (k == 10) CST_C0LB(bf16_t, 10); else CST_C0LB(bf16_t, C0L_KMAX); }
  else { if (k == 10) CST_C0LB(float, 10); else CST_C0LB(float, C0L_KMAX); }
#undef CST_C0LB
  hipLaunchKernelGGL(lg_reduce_kernel, dim3((unsigned)cst_ceil_div(C, 64), (unsigned)(k + 3)), dim3(64), 0, s, workspace, acc, (int)(B * nblk), k + 3, (int)C, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  hipLaunchKernelGGL(conv0_ln_scatter_kernel, dim3((unsigned)cst_ceil_div(C, 64)), dim3(64), 0, s, acc, dw, dbias, dgamma, dbeta, (int)C, k);
  return cst_check_launch("cst_conv0_ln_gelu_bwd");
}

extern "C" int cst_ln_gelu_fwd(const void* u, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                               const int32_t* row_limit, int64_t B, int64_t L, int64_t C, float eps, int dtype, cst_stream stream) {
  CST_REQUIRE(u && gamma && beta && y && mean && rstd, "cst_ln_gelu_fwd: null tensor");
  CST_REQUIRE(B * L < ((int64_t)1 << 31), "cst_ln_gelu_fwd: too many rows");
  CST_REQUIRE(B > 0 && L > 0 && C > 0 && C % 8 == 0 && C <= 8 * 64 * LG_MAXV, "cst_ln_gelu_fwd: C=%lld must be a multiple of 8 and <= %d", (long long)C, 8 * 64 * LG_MAXV);
  CST_REQUIRE(dtype == CST_BF16 || dtype == CST_F32, "cst_ln_gelu_fwd: bad dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LAYERNORM, s, 0.0, (double)B * L * C * cst_dtype_size(dtype) * 2.0);
  const dim3 grid(lg_blocks(B * L, LG_FWD_BLOCKS));
#define CST_LGF(T, NVV) hipLaunchKernelGGL((ln_gelu_fwd_kernel<T, NVV>), grid, dim3(LG_WAVES * 64), 0, s, (const T*)u, (const T*)gamma, (const T*)beta, (T*)y, mean, rstd, row_limit, B, L, (int)C, eps)
#define CST_LGF_NV(T) do { const int nv = lg_nv(C); if (nv == 1) CST_LGF(T, 1); else if (nv == 2) CST_LGF(T, 2); else CST_LGF(T, 4); } while (0)
  if (dtype == CST_BF16) CST_LGF_NV(bf16_t);
  else CST_LGF_NV(float);
#undef CST_LGF_NV
#undef CST_LGF
  return cst_check_launch("cst_ln_gelu_fwd");
}

/* [blocks][3][C] block partials */
extern "C" int64_t cst_ln_gelu_bwd_workspace(int64_t rows, int64_t C) {
  return (int64_t)lg_blocks(rows, LG_BWD_BLOCKS) * 3 * C * (int64_t)sizeof(float);
}

extern "C" int cst_ln_gelu_bwd(const void* dy, const void* u, const void* gamma, const void* beta, const float* mean, const float* rstd,
                               void* du, int64_t du_batch_stride, float* dgamma, float* dbeta, float* dcolsum, float* workspace,
                               const int32_t* row_limit, int64_t B, int64_t L, int64_t C, int dtype, cst_stream stream) {
  CST_REQUIRE(dy && u && gamma && beta && mean && rstd && du && dgamma && dbeta && workspace, "cst_ln_gelu_bwd: null tensor");
  CST_REQUIRE(B * L < ((int64_t)1 << 31), "cst_ln_gelu_bwd: too many rows");
  CST_REQUIRE(B > 0 && L > 0 && C > 0 && C % 8 == 0 && C <= 8 * 64 * LG_MAXV, "cst_ln_gelu_bwd: C=%lld must be a multiple of 8 and <= %d", (long long)C, 8 * 64 * LG_MAXV);
  CST_REQUIRE(du_batch_stride >= L * C && du_batch_stride % 8 == 0, "cst_ln_gelu_bwd: du_batch_stride=%lld", (long long)du_batch_stride);
  CST_REQUIRE(dtype == CST_BF16 || dtype == CST_F32, "cst_ln_gelu_bwd: bad dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LAYERNORM, s, 0.0, (double)B * L * C * cst_dtype_size(dtype) * 3.0);
  const int nb = lg_blocks(B * L, LG_BWD_BLOCKS);
#define CST_LGB(T, NVV) hipLaunchKernelGGL((ln_gelu_bwd_kernel<T, NVV>), dim3(nb), dim3(LG_WAVES * 64), 0, s, (const T*)dy, (const T*)u, (const T*)gamma, (const T*)beta, mean, rstd, (T*)du, du_batch_stride, workspace, row_limit, B, L, (int)C)
#define CST_LGB_NV(T) do { const int nv = lg_nv(C); if (nv == 1) CST_LGB(T, 1); else if (nv == 2) CST_LGB(T, 2); else CST_LGB(T, 4); } while (0)
  if (dtype == CST_BF16) CST_LGB_NV(bf16_t);
  else CST_LGB_NV(float);
#undef CST_LGB_NV
#undef CST_LGB
  // rows 0 / 1 / 2 of the partials straight into dgamma / dbeta / dcolsum (a NULL dcolsum: row 2 is dropped)
  hipLaunchKernelGGL(lg_reduce_kernel, dim3((unsigned)cst_ceil_div(C, 64), dcolsum ? 3u : 2u), dim3(64), 0, s, workspace, (float*)nullptr, nb, 3, (int)C, dgamma, dbeta, dcolsum);
  return cst_check_launch("cst_ln_gelu_bwd");
}
