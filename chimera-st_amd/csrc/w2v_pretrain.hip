// w2v_pretrain.hip — the head of wav2vec2 pre-training.  First the contrastive half (models/wav2vec/wav2vec2.py:454-525 +
// criterions/wav2vec_criterion.py); the Gumbel vector quantizer follows further down with its own header:
//   cst_w2v_negatives  : the index draws of sample_negatives from the counter hash (integers only; rng.negatives_numpy is the twin)
//   cst_infonce_fwd    : cos(x, y[target]) / temp over the positive and the K' gathered negatives, cross entropy against class 0
//   cst_infonce_bwd_x  : d loss / d x, and per (position, j) the pair (d loss / d cos, cos) for the second backward
//   cst_infonce_bwd_y  : d loss / d y through an inverted index (per target row the (position, j) pairs that read it)
// The reference gathers a [K' + 1, B, M, D] tensor of targets, runs cosine_similarity over it and keeps the [K' + 1, B M] logits for
// autograd.  Here neither exists: one wave owns one position, keeps its x row in registers and reads the K' + 1 target rows by index.
// Everything is fp32 on bf16 / fp32 storage with correctly rounded division and square root and libm-accuracy expf / logf
// (tests/w2v_pretrain_ref.py counts the roundings).
//
// Row layout in a wave: D = 8 NG elements, lane l owns the 8-element groups l and l + 64 (D <= 1024), read with one 16-byte (bf16) or two
// 16-byte (fp32) loads.  A dot product is the lane's fmaf chain over its elements in index order, then the 6-step xor butterfly — every
// lane ends with the same bits, so the per-target scalars (cos, logit, weights) are wave-uniform without a broadcast.
// cos follows the installed torch.cosine_similarity: each norm is clamped to eps = 1e-8 on its own, cos = x.t / (max(|x|, eps) max(|t|, eps)).
// A negative whose row equals the positive's row element for element gets logit -inf (compute_preds :514-523); when all do, nll = 0.
// No float atomics anywhere, no host synchronisation: loss, counters and gradients are bit-reproducible, and at Kx = 0 an utterance's
// numbers do not depend on the rest of its batch.
#include "cst_common.h"

#define W2V_D_MAX 1024                 // two 8-element groups per lane
#define W2V_KP_MAX 1023                // K' + 1 logits of a position are staged in LDS: 4 waves x 1024 floats
#define W2V_EPS 1e-8f                  // F.cosine_similarity's default, which the reference leaves alone
#define W2V_WAVES 4

namespace {

template <typename T>
__device__ __forceinline__ void w2v_load_row(const T* row, int NG, int lane, float (&v)[2][8]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int g = lane + 64 * i;
    if (g < NG) {
      load8(row + 8 * g, v[i]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.0f;
    }
  }
}
template <typename T>
__device__ __forceinline__ void w2v_store_row(T* row, int NG, int lane, const float (&v)[2][8]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int g = lane + 64 * i;
    if (g < NG) store8(row + 8 * g, v[i]);
  }
}
__device__ __forceinline__ float w2v_dot(const float (&a)[2][8], const float (&b)[2][8]) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(a[i][e], b[i][e], s);
  return wave_sum(s);
}
__device__ __forceinline__ bool w2v_rows_equal(const float (&a)[2][8], const float (&b)[2][8]) {
  bool eq = true;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) eq = eq && (a[i][e] == b[i][e]);
  return __all(eq);
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
// the target row of (position p, slot j): j = 0 is the positive, y[p]; an index outside [0, N) is clamped (device data cannot be refused)
__device__ __forceinline__ int64_t w2v_target_row(const int32_t* idx, int64_t p, int j, int KP, int64_t N) {
  if (j == 0) return p;
  const int64_t r = idx[p * KP + (j - 1)];
  return r < 0 ? 0 : (r >= N ? N - 1 : r);
}
// logit of one target: wave-uniform.  cos is returned too.
__device__ __forceinline__ float w2v_logit(const float (&xv)[2][8], const float (&pv)[2][8], const float (&tv)[2][8], float cx, float nt,
                                           float inv_temp, int j, float& cos_out) {
  // forward and backward must see EQUAL bits, so the product below may not be contracted into a caller's subtraction (l - lse): without
  // this the backward's exp(l_0 - lse) at an all-masked position is exp(of a rounding residue), not exp(0)
#pragma clang fp contract(off)
  const float dot = w2v_dot(xv, tv);
  const float c = dot / (cx * fmaxf(nt, W2V_EPS));
  cos_out = c;
  if (j > 0 && w2v_rows_equal(pv, tv)) return -INFINITY;
  return c * inv_temp;
}

// ny[r] = |y_r|: once per row, not once per (position, j) that reads it
template <typename T>
__global__ __launch_bounds__(64 * W2V_WAVES) void w2v_norm_kernel(const T* y, float* ny, int64_t N, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * W2V_WAVES + (threadIdx.x >> 6);
  if (r >= N) return;
  float v[2][8];
  w2v_load_row(y + r * D, D >> 3, lane, v);
  const float n = sqrtf(w2v_dot(v, v));
  if (lane == 0) ny[r] = n;
}

template <typename T>
__global__ __launch_bounds__(64 * W2V_WAVES) void infonce_fwd_kernel(const T* x, const T* y, const int32_t* idx, const float* ny, float inv_temp,
                                                                     float* nll, float* lse_out, float* nx_out, int32_t* flags,
                                                                     float* logits_dbg, int64_t N, int KP, int D) {
  __shared__ float sl[W2V_WAVES][W2V_KP_MAX + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NG = D >> 3;
  const int64_t p0 = (int64_t)blockIdx.x * W2V_WAVES + wave;
  const bool live = p0 < N;
  const int64_t p = live ? p0 : N - 1;  // (a wave past the end repeats the last position and stores nothing: the barrier below is uniform)
  float xv[2][8], pv[2][8], tv[2][8];
  w2v_load_row(x + p * D, NG, lane, xv);
  w2v_load_row(y + p * D, NG, lane, pv);
  const float nx = sqrtf(w2v_dot(xv, xv)), cx = fmaxf(nx, W2V_EPS);
  for (int j = 0; j <= KP; ++j) {
    const int64_t r = w2v_target_row(idx, p, j, KP, N);
    w2v_load_row(y + r * D, NG, lane, tv);
    float c;
    const float l = w2v_logit(xv, pv, tv, cx, ny[r], inv_temp, j, c);
    if (lane == 0) sl[wave][j] = l;
  }
  __syncthreads();
  float m = -INFINITY, mn = INFINITY;
  for (int j = lane; j <= KP; j += 64) { m = fmaxf(m, sl[wave][j]); mn = fminf(mn, sl[wave][j]); }
  m = wave_max(m);
  mn = wave_min(mn);
  float se = 0.0f;
  for (int j = lane; j <= KP; j += 64) se += expf(sl[wave][j] - m);
  se = wave_sum(se);
  const float lse = m + logf(se), l0 = sl[wave][0];
  if (live && logits_dbg)
    for (int j = lane; j <= KP; j += 64) logits_dbg[p * (KP + 1) + j] = sl[wave][j];
  if (live && lane == 0) {
    nll[p] = lse - l0;
    lse_out[p] = lse;
    nx_out[p] = nx;
    flags[p] = (l0 == m) && !(l0 == mn);  // argmax == 0 and not argmin == 0, ties to the lowest index (wav2vec_criterion.py:97-103)
  }
}

// loss = the sum of nll in a fixed tree, in double; counters = (correct, count)
__global__ __launch_bounds__(256) void infonce_sum_kernel(const float* nll, const int32_t* flags, float* loss, int32_t* counters, int64_t N) {
  __shared__ double red[256];
  __shared__ int redc[256];
  double a = 0.0;
  int c = 0;
  for (int64_t i = threadIdx.x; i < N; i += 256) { a += (double)nll[i]; c += flags[i]; }
  red[threadIdx.x] = a;
  redc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; redc[threadIdx.x] += redc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { loss[0] = (float)red[0]; counters[0] = redc[0]; counters[1] = (int32_t)N; }
}

// d cos / d a of cos = a.b / (max(|a|, eps) max(|b|, eps)) summed with weights: out = acc / ca - [|a| >= eps] S / (ca |a|) a, where
// acc = sum w b / cb-weighted rows and S = sum dcos cos (clamp_min passes the gradient at |a| >= eps)
__device__ __forceinline__ void w2v_finish_grad(float (&acc)[2][8], const float (&av)[2][8], float S, float na) {
  const float ca = fmaxf(na, W2V_EPS);
  const float coef = na >= W2V_EPS ? S / (ca * na) : 0.0f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = acc[i][e] / ca - coef * av[i][e];
}

template <typename T>
__global__ __launch_bounds__(64 * W2V_WAVES) void infonce_bwd_x_kernel(const T* x, const T* y, const int32_t* idx, const float* ny, const float* nx_in,
                                                                       const float* lse_in, const float* gscale, float inv_temp, T* dx,
                                                                       float* pairs, int64_t N, int KP, int D) {
  const int lane = threadIdx.x & 63, NG = D >> 3;
  const int64_t p = (int64_t)blockIdx.x * W2V_WAVES + (threadIdx.x >> 6);
  if (p >= N) return;
  float xv[2][8], pv[2][8], tv[2][8], acc[2][8];
  w2v_load_row(x + p * D, NG, lane, xv);
  w2v_load_row(y + p * D, NG, lane, pv);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.0f;
  const float nx = nx_in[p], cx = fmaxf(nx, W2V_EPS), lse = lse_in[p], g = gscale[0];
  float S = 0.0f;
  float* pr = pairs + p * (KP + 1) * 2;
  for (int j = 0; j <= KP; ++j) {
    const int64_t r = w2v_target_row(idx, p, j, KP, N);
    w2v_load_row(y + r * D, NG, lane, tv);
    const float nt = ny[r];
    float c;
    const float l = w2v_logit(xv, pv, tv, cx, nt, inv_temp, j, c);  // the forward's bits
    const float dl = l == -INFINITY ? 0.0f : g * (expf(l - lse) - (j == 0 ? 1.0f : 0.0f));
    const float dc = dl * inv_temp;
    const float w = dc / fmaxf(nt, W2V_EPS);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[i][e] = fmaf(w, tv[i][e], acc[i][e]);
    S = fmaf(dc, c, S);
    if (lane == 0) { pr[2 * j] = dc; pr[2 * j + 1] = c; }
  }
  w2v_finish_grad(acc, xv, S, nx);
  w2v_store_row(dx + p * D, NG, lane, acc);
}

// One wave per target row sums its list in list order (the row's own positive first, then the negatives that drew it in ascending
// (position, j)): a fixed order, hence reproducible bits.  The draws are UNIFORM over an utterance's positions (cst_w2v_negatives), so
// every list is about K' + 1 long and the waves are evenly loaded — that is why the one-wave-per-destination form is taken here; with
// skewed destinations (codebook usage, token embeddings) a few waves would carry most of the work.
template <typename T>
__global__ __launch_bounds__(64 * W2V_WAVES) void infonce_bwd_y_kernel(const T* x, const T* y, const int64_t* perm, const int32_t* offs,
                                                                       const float* pairs, const float* nx_in, const float* ny, T* dy,
                                                                       int64_t N, int KP, int D) {
  const int lane = threadIdx.x & 63, NG = D >> 3;
  const int64_t r = (int64_t)blockIdx.x * W2V_WAVES + (threadIdx.x >> 6);
  if (r >= N) return;
  float tv[2][8], xv[2][8], acc[2][8];
  w2v_load_row(y + r * D, NG, lane, tv);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.0f;
  float S = 0.0f;
  const int64_t total = N * (int64_t)(KP + 1);
  int64_t i0 = offs[r], i1 = offs[r + 1];
  i0 = i0 < 0 ? 0 : i0;
  i1 = i1 > total ? total : i1;
  for (int64_t i = i0; i < i1; ++i) {
    const int64_t v = perm[i];
    if (v < 0 || v >= total) continue;  // (an index that is none is never followed)
    const int64_t p = v < N ? v : (v - N) / KP;
    const int j = v < N ? 0 : (int)((v - N) % KP) + 1;
    const float dc = pairs[(p * (KP + 1) + j) * 2], c = pairs[(p * (KP + 1) + j) * 2 + 1];
    const float w = dc / fmaxf(nx_in[p], W2V_EPS);
    w2v_load_row(x + p * D, NG, lane, xv);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[a][e] = fmaf(w, xv[a][e], acc[a][e]);
    S = fmaf(dc, c, S);
  }
  w2v_finish_grad(acc, tv, S, ny[r]);
  w2v_store_row(dy + r * D, NG, lane, acc);
}

// element (b, m, j) of out [B, M, K + Kx]: one 32-bit word of the counter hash, scaled by a multiply-high
__global__ __launch_bounds__(256) void w2v_negatives_kernel(uint32_t key, int32_t* out, int64_t B, int64_t M, int64_t K, int64_t Kx) {
  const int64_t KP = K + Kx, total = B * M * KP;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t j = e % KP, pos = e / KP, m = pos % M, b = pos / M;
  const uint32_t bits = cst_drop_bits(key, (uint64_t)e);
  uint32_t r;
  if (j < K) {  // own utterance: uniform over the M - 1 other positions
    r = __umulhi(bits, (uint32_t)(M - 1));
    r += r >= (uint32_t)m;
    r += (uint32_t)(b * M);
  } else {      // any utterance: uniform over B M - 1 values, shifted past the position's TIME index as the reference does (:481-493)
    r = __umulhi(bits, (uint32_t)(B * M - 1));
    r += r >= (uint32_t)m;
  }
  out[e] = (int32_t)r;
}

int infonce_check(const char* who, const void* x, const void* y, const int32_t* idx, int64_t N, int64_t KP, int64_t D, int dtype) {
  CST_REQUIRE(x && y && idx, "%s: null operand", who);
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "%s: bad dtype %d", who, dtype);
  CST_REQUIRE(N > 0 && KP > 0 && D > 0 && N * (KP + 1) < INT32_MAX, "%s: bad shape N %lld K' %lld D %lld", who, (long long)N, (long long)KP,
              (long long)D);
  CST_REQUIRE(D % 8 == 0 && D <= W2V_D_MAX, "%s: D = %lld must be a multiple of 8 and at most %d", who, (long long)D, W2V_D_MAX);
  CST_REQUIRE(KP <= W2V_KP_MAX, "%s: %lld negatives exceed the supported %d", who, (long long)KP, W2V_KP_MAX);
  CST_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)idx % 4 == 0, "%s: operands are not 16-byte aligned", who);
  return CST_OK;
}

}  // namespace

#define W2V_GRID(n) dim3((unsigned)cst_ceil_div((n), W2V_WAVES)), dim3(64 * W2V_WAVES), 0, s

extern "C" int cst_w2v_negatives(uint32_t key, int64_t B, int64_t M, int64_t K, int64_t Kx, int32_t* out, cst_stream stream) {
  CST_REQUIRE(out, "cst_w2v_negatives: null operand");
  CST_REQUIRE(B > 0 && M > 0 && K >= 0 && Kx >= 0 && K + Kx > 0 && B < INT32_MAX && M < INT32_MAX && K + Kx < INT32_MAX &&
                  B * M < INT32_MAX && B * M * (K + Kx) < INT32_MAX,
              "cst_w2v_negatives: bad shape B %lld M %lld K %lld Kx %lld", (long long)B, (long long)M, (long long)K, (long long)Kx);
  CST_REQUIRE(K == 0 || M >= 2, "cst_w2v_negatives: own-utterance negatives need M >= 2 positions, got %lld", (long long)M);
  CST_REQUIRE(Kx == 0 || B * M >= 2, "cst_w2v_negatives: cross-sample negatives need B M >= 2 positions, got %lld", (long long)(B * M));
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = B * M * (K + Kx);
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)total * 4);
  hipLaunchKernelGGL(w2v_negatives_kernel, dim3((unsigned)cst_ceil_div(total, 256)), dim3(256), 0, s, key, out, B, M, K, Kx);
  return cst_check_launch("cst_w2v_negatives");
}

extern "C" int cst_infonce_fwd(const void* x, const void* y, const int32_t* idx, float inv_temp, float* nll, float* loss, int32_t* counters,
                               float* lse, float* nx, float* ny, int32_t* flags, float* logits_dbg, int64_t N, int64_t KP, int64_t D,
                               int dtype, cst_stream stream) {
  const int rc = infonce_check("cst_infonce_fwd", x, y, idx, N, KP, D, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(nll && loss && counters && lse && nx && ny && flags, "cst_infonce_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 2.0 * N * (KP + 2) * D, (double)N * (KP + 3) * D * cst_dtype_size(dtype));
  if (dtype == CST_BF16) {
    hipLaunchKernelGGL(w2v_norm_kernel<bf16_t>, W2V_GRID(N), (const bf16_t*)y, ny, N, (int)D);
    hipLaunchKernelGGL(infonce_fwd_kernel<bf16_t>, W2V_GRID(N), (const bf16_t*)x, (const bf16_t*)y, idx, (const float*)ny, inv_temp, nll, lse,
                       nx, flags, logits_dbg, N, (int)KP, (int)D);
  } else {
    hipLaunchKernelGGL(w2v_norm_kernel<float>, W2V_GRID(N), (const float*)y, ny, N, (int)D);
    hipLaunchKernelGGL(infonce_fwd_kernel<float>, W2V_GRID(N), (const float*)x, (const float*)y, idx, (const float*)ny, inv_temp, nll, lse, nx,
                       flags, logits_dbg, N, (int)KP, (int)D);
  }
  hipLaunchKernelGGL(infonce_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)nll, (const int32_t*)flags, loss, counters, N);
  return cst_check_launch("cst_infonce_fwd");
}

extern "C" int cst_infonce_bwd_x(const void* x, const void* y, const int32_t* idx, float inv_temp, const float* lse, const float* nx,
                                 const float* ny, const float* gscale, void* dx, float* pairs, int64_t N, int64_t KP, int64_t D, int dtype,
                                 cst_stream stream) {
  const int rc = infonce_check("cst_infonce_bwd_x", x, y, idx, N, KP, D, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(lse && nx && ny && gscale && dx && pairs, "cst_infonce_bwd_x: null operand");
  CST_REQUIRE((uintptr_t)dx % 16 == 0, "cst_infonce_bwd_x: operands are not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 4.0 * N * (KP + 1) * D, (double)N * (KP + 4) * D * cst_dtype_size(dtype));
  if (dtype == CST_BF16)
    hipLaunchKernelGGL(infonce_bwd_x_kernel<bf16_t>, W2V_GRID(N), (const bf16_t*)x, (const bf16_t*)y, idx, ny, nx, lse, gscale, inv_temp,
                       (bf16_t*)dx, pairs, N, (int)KP, (int)D);
  else
    hipLaunchKernelGGL(infonce_bwd_x_kernel<float>, W2V_GRID(N), (const float*)x, (const float*)y, idx, ny, nx, lse, gscale, inv_temp,
                       (float*)dx, pairs, N, (int)KP, (int)D);
  return cst_check_launch("cst_infonce_bwd_x");
}

extern "C" int cst_infonce_bwd_y(const void* x, const void* y, const int64_t* perm, const int32_t* offs, const float* pairs, const float* nx,
                                 const float* ny, void* dy, int64_t N, int64_t KP, int64_t D, int dtype, cst_stream stream) {
  CST_REQUIRE(perm && offs, "cst_infonce_bwd_y: null operand");
  const int rc = infonce_check("cst_infonce_bwd_y", x, y, offs, N, KP, D, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(pairs && nx && ny && dy, "cst_infonce_bwd_y: null operand");
  CST_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)perm % 8 == 0, "cst_infonce_bwd_y: operands are not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 2.0 * N * (KP + 1) * D, (double)N * (KP + 3) * D * cst_dtype_size(dtype));
  if (dtype == CST_BF16)
    hipLaunchKernelGGL(infonce_bwd_y_kernel<bf16_t>, W2V_GRID(N), (const bf16_t*)x, (const bf16_t*)y, perm, offs, pairs, nx, ny, (bf16_t*)dy, N,
                       (int)KP, (int)D);
  else
    hipLaunchKernelGGL(infonce_bwd_y_kernel<float>, W2V_GRID(N), (const float*)x, (const float*)y, perm, offs, pairs, nx, ny, (float*)dy, N,
                       (int)KP, (int)D);
  return cst_check_launch("cst_infonce_bwd_y");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Gumbel vector quantizer (modules/gumbel_vector_quantizer.py:138-199).  The reference builds one-hot [N G, V] tensors three times and
// multiplies [N, G V, 1] by the codebook; here one wave owns one (row, group): lane l holds classes l, l + 64, ... (V <= 1024).
//   cst_gumbel_vq_fwd : k = argmax_v (l_v + g_v) in training, argmax_v l_v in eval (ties: the lowest index); q = vars[g V + k], idx, the
//                       one-hot; avg_probs / prob_perplexity (softmax of the raw logits, :161-166) and code_perplexity (the raw logits'
//                       argmax, :150-159) through per-workgroup partial sums and a second, one-workgroup launch — fixed order, no atomics
//   cst_gumbel_vq_bwd : d logits = straight-through term (1 / tau) s~ (gy - sum s~ gy), s~ = softmax((l + g) / tau) RECOMPUTED from
//                       the logits and the regenerated noise (nothing is kept, as with dropout masks), plus the diversity term through
//                       avg_probs, (1 / N) s (h - sum s h), h_v = -dppl exp(H_g) (log(a_v + 1e-7) + a_v / (a_v + 1e-7))
// Noise: g = -log(-log u), u = ((bits >> 9) + 0.5) 2^-23 with bits = cst_drop_bits(key, element (n G + g) V + v): 23 bits, so that
// u is exact in fp32 and lies in [2^-24, 1 - 2^-24] — with 24 bits the largest value rounds to u = 1 and g = +inf.
// rng.gumbel_uniform_numpy restates u exactly.  A `noise` pointer (fp32 [N, G, V]) is read instead when given (tests, fixtures).
// ---------------------------------------------------------------------------------------------------------------------------------
#define VQ_V_MAX 1024
#define VQ_ROWS 32        // rows per workgroup in the statistics' first stage: 8 per wave
#define VQ_TINY 1e-7f     // the reference's + 1e-7 inside the perplexities' logarithm

namespace {

__device__ __forceinline__ float vq_uniform(uint32_t bits) { return ((float)(bits >> 9) + 0.5f) * 1.1920928955078125e-07f; }
__device__ __forceinline__ float vq_gumbel(uint32_t key, const float* noise, int64_t e) {
  if (noise) return noise[e];
  return -logf(-logf(vq_uniform(cst_drop_bits(key, (uint64_t)e))));
}
// argmax over a wave's classes, ties to the lowest index
__device__ __forceinline__ int vq_wave_argmax(float bv, int bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  return bi;
}

template <typename T, int NI>
__global__ __launch_bounds__(256) void gumbel_vq_fwd_kernel(const T* logits, const T* vars, const float* noise, uint32_t key, int training,
                                                            T* q, int32_t* idx, T* onehot, float* part_p, int32_t* part_c, int64_t N, int G,
                                                            int V, int d) {
  __shared__ float sp[4][64 * NI];
  __shared__ int sc[4][64 * NI];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * VQ_ROWS;
  float accp[NI];
  int cnt[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) { accp[i] = 0.0f; cnt[i] = 0; }
  for (int64_t n = r0 + wave; n < r0 + VQ_ROWS && n < N; n += 4) {
    const int64_t e0 = (n * G + g) * V;
    float l[NI];
    float bl = -INFINITY, bs = -INFINITY;
    int il = INT32_MAX, is = INT32_MAX;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int v = lane + 64 * i;
      l[i] = v < V ? DT<T>::ld(logits + e0 + v) : -INFINITY;
      if (v < V) {
        if (l[i] > bl) { bl = l[i]; il = v; }  // (ascending v: the first maximum stays)
        const float s = training ? l[i] + vq_gumbel(key, noise, e0 + v) : l[i];
        if (s > bs) { bs = s; is = v; }
      }
    }
    int kh = vq_wave_argmax(bl, il);                // the raw logits' choice: code_perplexity
    int k = training ? vq_wave_argmax(bs, is) : kh;
    kh = kh == INT32_MAX ? 0 : kh;                  // (a row of NaNs: code 0 — no address is formed from a choice that is none)
    k = k == INT32_MAX ? 0 : k;
    const float m = wave_max(bl);
    float ex[NI], se = 0.0f;
#pragma unroll
    for (int i = 0; i < NI; ++i) { ex[i] = lane + 64 * i < V ? expf(l[i] - m) : 0.0f; se += ex[i]; }
    se = wave_sum(se);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int v = lane + 64 * i;
      accp[i] += ex[i] / se;
      cnt[i] += (v == kh);
      if (v < V) DT<T>::st(onehot + e0 + v, v == k ? 1.0f : 0.0f);
    }
    if (lane == 0) idx[n * G + g] = k;
    const T* src = vars + ((int64_t)g * V + k) * d;
    T* dst = q + (n * G + g) * d;
    for (int c = lane; c < (d >> 3); c += 64) {
      float t[8];
      load8(src + 8 * c, t);
      store8(dst + 8 * c, t);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) { sp[wave][lane + 64 * i] = accp[i]; sc[wave][lane + 64 * i] = cnt[i]; }
  __syncthreads();
  for (int v = threadIdx.x; v < V; v += 256) {
    const float p = ((sp[0][v] + sp[1][v]) + sp[2][v]) + sp[3][v];
    const int c = sc[0][v] + sc[1][v] + sc[2][v] + sc[3][v];
    part_p[((int64_t)blockIdx.x * G + g) * V + v] = p;
    part_c[((int64_t)blockIdx.x * G + g) * V + v] = c;
  }
}

__device__ __forceinline__ float vq_block_sum256(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// one workgroup: the partial sums in block order, then the two perplexities.  stats = (prob_perplexity, code_perplexity), exph [G] =
// exp(H_g) of the soft distribution (the backward's factor)
__global__ __launch_bounds__(256) void gumbel_vq_stats_kernel(const float* part_p, const int32_t* part_c, float* avg_probs, float* stats,
                                                              float* exph, int64_t N, int64_t nblk, int G, int V) {
  __shared__ float red[256];
  float ppl = 0.0f, cpl = 0.0f;
  const float fn = (float)N;
  for (int g = 0; g < G; ++g) {
    float hs = 0.0f, hc = 0.0f;
    for (int v = threadIdx.x; v < V; v += 256) {
      float p = 0.0f;
      int c = 0;
      for (int64_t b = 0; b < nblk; ++b) { p += part_p[(b * G + g) * V + v]; c += part_c[(b * G + g) * V + v]; }
      const float a = p / fn, h = (float)c / fn;
      avg_probs[g * V + v] = a;
      hs += a * logf(a + VQ_TINY);
      hc += h * logf(h + VQ_TINY);
    }
    const float es = expf(-vq_block_sum256(hs, red)), ec = expf(-vq_block_sum256(hc, red));
    if (threadIdx.x == 0) exph[g] = es;
    ppl += es;
    cpl += ec;
  }
  if (threadIdx.x == 0) { stats[0] = ppl; stats[1] = cpl; }
}

template <typename T, int NI>
__global__ __launch_bounds__(256) void gumbel_vq_bwd_kernel(const T* logits, const float* noise, uint32_t key, float inv_tau, const T* gy,
                                                            const float* avg_probs, const float* exph, const float* dppl, T* dl, int64_t N,
                                                            int G, int V) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= N * G) return;
  const int g = (int)(item % G);
  const int64_t e0 = item * V;
  const float c0 = dppl[0] * exph[g], inv_n = 1.0f / (float)N;
  float l[NI], z[NI], gv[NI], h[NI];
  float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int v = lane + 64 * i;
    const bool in = v < V;
    l[i] = in ? DT<T>::ld(logits + e0 + v) : -INFINITY;
    z[i] = in ? (l[i] + vq_gumbel(key, noise, e0 + v)) * inv_tau : -INFINITY;
    gv[i] = in ? DT<T>::ld(gy + e0 + v) : 0.0f;
    const float a = in ? avg_probs[g * V + v] : 0.0f;
    h[i] = in ? -c0 * (logf(a + VQ_TINY) + a / (a + VQ_TINY)) : 0.0f;
    m1 = fmaxf(m1, z[i]);
    m2 = fmaxf(m2, l[i]);
  }
  m1 = wave_max(m1);
  m2 = wave_max(m2);
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const bool in = lane + 64 * i < V;
    z[i] = in ? expf(z[i] - m1) : 0.0f;
    l[i] = in ? expf(l[i] - m2) : 0.0f;
    s1 += z[i];
    s2 += l[i];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  float d1 = 0.0f, d2 = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    z[i] = z[i] / s1;  // s~
    l[i] = l[i] / s2;  // s
    d1 = fmaf(z[i], gv[i], d1);
    d2 = fmaf(l[i], h[i], d2);
  }
  d1 = wave_sum(d1);
  d2 = wave_sum(d2);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int v = lane + 64 * i;
    if (v < V) DT<T>::st(dl + e0 + v, inv_tau * z[i] * (gv[i] - d1) + inv_n * l[i] * (h[i] - d2));
  }
}

int vq_check(const char* who, const void* logits, int64_t N, int64_t G, int64_t V, int dtype) {
  CST_REQUIRE(logits, "%s: null operand", who);
  CST_REQUIRE(dtype == CST_F32 || dtype == CST_BF16, "%s: bad dtype %d", who, dtype);
  CST_REQUIRE(N > 0 && G > 0 && G <= 65535 && V > 0 && N * G * V < ((int64_t)1 << 40), "%s: bad shape N %lld G %lld V %lld", who, (long long)N,
              (long long)G, (long long)V);
  CST_REQUIRE(V <= VQ_V_MAX, "%s: V = %lld codes per group exceed the supported %d", who, (long long)V, VQ_V_MAX);
  return CST_OK;
}

}  // namespace

#define VQ_BY_WIDTH(V, LAUNCH)             \
  do {                                     \
    if ((V) <= 64) { LAUNCH(1); }          \
    else if ((V) <= 320) { LAUNCH(5); }    \
    else { LAUNCH(16); }                   \
  } while (0)

extern "C" int64_t cst_gumbel_vq_workspace(int64_t N, int64_t G, int64_t V) {
  if (N <= 0 || G <= 0 || V <= 0) return 0;
  return cst_ceil_div(N, VQ_ROWS) * G * V * 8;  // fp32 probability sums + int32 counts per first-stage workgroup
}

extern "C" int cst_gumbel_vq_fwd(const void* logits, const void* vars, const float* noise, uint32_t key, int training, void* q, int32_t* idx,
                                 void* onehot, float* avg_probs, float* stats, float* exph, void* workspace, int64_t N, int64_t G, int64_t V,
                                 int64_t d, int dtype, cst_stream stream) {
  const int rc = vq_check("cst_gumbel_vq_fwd", logits, N, G, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(vars && q && idx && onehot && avg_probs && stats && exph && workspace, "cst_gumbel_vq_fwd: null operand");
  CST_REQUIRE(d > 0 && d % 8 == 0, "cst_gumbel_vq_fwd: d = %lld must be a multiple of 8", (long long)d);
  CST_REQUIRE((uintptr_t)vars % 16 == 0 && (uintptr_t)q % 16 == 0 && (uintptr_t)workspace % 4 == 0,
              "cst_gumbel_vq_fwd: operands are not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nblk = cst_ceil_div(N, VQ_ROWS);
  CST_REQUIRE(nblk < INT32_MAX, "cst_gumbel_vq_fwd: bad shape N %lld", (long long)N);
  float* part_p = (float*)workspace;
  int32_t* part_c = (int32_t*)workspace + nblk * G * V;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)N * G * (2.0 * V + d) * cst_dtype_size(dtype));
  const dim3 grid((unsigned)nblk, (unsigned)G);
#define VQ_FWD(NI)                                                                                                                        \
  if (dtype == CST_BF16)                                                                                                                  \
    hipLaunchKernelGGL((gumbel_vq_fwd_kernel<bf16_t, NI>), grid, dim3(256), 0, s, (const bf16_t*)logits, (const bf16_t*)vars, noise, key,  \
                       training, (bf16_t*)q, idx, (bf16_t*)onehot, part_p, part_c, N, (int)G, (int)V, (int)d);                            \
  else                                                                                                                                    \
    hipLaunchKernelGGL((gumbel_vq_fwd_kernel<float, NI>), grid, dim3(256), 0, s, (const float*)logits, (const float*)vars, noise, key,    \
                       training, (float*)q, idx, (float*)onehot, part_p, part_c, N, (int)G, (int)V, (int)d)
  VQ_BY_WIDTH(V, VQ_FWD);
#undef VQ_FWD
  hipLaunchKernelGGL(gumbel_vq_stats_kernel, dim3(1), dim3(256), 0, s, (const float*)part_p, (const int32_t*)part_c, avg_probs, stats, exph, N,
                     nblk, (int)G, (int)V);
  return cst_check_launch("cst_gumbel_vq_fwd");
}

extern "C" int cst_gumbel_vq_bwd(const void* logits, const float* noise, uint32_t key, float inv_tau, const void* gy, const float* avg_probs,
                                 const float* exph, const float* dppl, void* dl, int64_t N, int64_t G, int64_t V, int dtype,
                                 cst_stream stream) {
  const int rc = vq_check("cst_gumbel_vq_bwd", logits, N, G, V, dtype);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(gy && avg_probs && exph && dppl && dl, "cst_gumbel_vq_bwd: null operand");
  CST_REQUIRE(inv_tau > 0.0f, "cst_gumbel_vq_bwd: 1 / tau = %g must be positive", (double)inv_tau);
  hipStream_t s = (hipStream_t)stream;
  CstProfScope prof(CST_K_LOSS, s, 0.0, (double)N * G * V * 3.0 * cst_dtype_size(dtype));
  const dim3 grid((unsigned)cst_ceil_div(N * G, 4));
#define VQ_BWD(NI)                                                                                                                        \
  if (dtype == CST_BF16)                                                                                                                  \
    hipLaunchKernelGGL((gumbel_vq_bwd_kernel<bf16_t, NI>), grid, dim3(256), 0, s, (const bf16_t*)logits, noise, key, inv_tau,             \
                       (const bf16_t*)gy, avg_probs, exph, dppl, (bf16_t*)dl, N, (int)G, (int)V);                                          \
  else                                                                                                                                    \
    hipLaunchKernelGGL((gumbel_vq_bwd_kernel<float, NI>), grid, dim3(256), 0, s, (const float*)logits, noise, key, inv_tau,               \
                       (const float*)gy, avg_probs, exph, dppl, (float*)dl, N, (int)G, (int)V)
  VQ_BY_WIDTH(V, VQ_BWD);
#undef VQ_BWD
  return cst_check_launch("cst_gumbel_vq_bwd");
}
