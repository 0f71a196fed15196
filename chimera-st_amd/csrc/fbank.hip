// fbank.hip — Kaldi filter banks of collated 16 kHz audio, and the data config's feature transforms, on the device.
//   fbank_frames_kernel    : torchaudio.compliance.kaldi.fbank(wave * 32768, num_mel_bins=80, sample_frequency=16000) at the
//                            reference's call (fairseq/data/audio/audio_utils.py:80-93, reached from
//                            speech_to_text_dataset.py:143-147): 400-sample Povey frames every 160 samples (snip_edges), DC
//                            removal, pre-emphasis 0.97, 512-point real FFT, power, 80 triangular mel filters 20..8000 Hz,
//                            log(max(E, FLT_EPSILON)).  Rows t >= T_i are written 0.
//   fbank_transform_kernel : utterance_cmvn / global_cmvn / specaugment (feature_transforms/*.py) applied in place, in
//                            config order, from per-tile partial sums reduced in a fixed order (no float atomics).
#include "cst_common.h"

namespace {

constexpr int FB_WIN = 400, FB_SHIFT = 160, FB_NFFT = 512, FB_HALF = 256, FB_MEL = 80;
constexpr int FB_TILE = 32;                                      // frames per workgroup of the frames kernel
constexpr int FB_SPAN = FB_SHIFT * (FB_TILE - 1) + FB_WIN;       // samples a tile reads: 5360
constexpr int FB_WAVES = 4;
constexpr int FB_PAD = FB_HALF + FB_HALF / 32;                   // one float of padding every 32 (breaks the power-of-2 strides)
constexpr int FB_CHUNK = 256;                                    // frames per workgroup of the transform kernel
constexpr int FB_MAXMASK = 8;

__device__ __forceinline__ int fpad(int i) { return i + (i >> 5); }

struct FbTables {
  float win[FB_WIN];
  float tw_re[FB_HALF], tw_im[FB_HALF];       // exp(-2 pi i m / 256): twiddles of the 256-point complex FFT
  float rs_re[FB_HALF], rs_im[FB_HALF];       // exp(-2 pi i k / 512): the real-split step
  float frac[FB_HALF];                        // u_k - floor(u_k), u_k = (mel(31.25 k) - mel(20)) / delta
  int kb[FB_MEL + 2];                         // kb[m] = #{k : u_k <= m}: filter m is 0 outside bins [kb[m], kb[m + 2])
  int fl[FB_HALF];                            // floor(u_k)
};

struct FbSmem {
  FbTables tab;
  float stage[FB_SPAN];
  float re[FB_WAVES][2][FB_PAD], im[FB_WAVES][2][FB_PAD];
  float tile[FB_TILE][FB_MEL];
};

// tables in fp64, rounded once: an fp32 mel position u (up to 81) carries ~1e-5 of absolute error into the filter weights,
// which is 1e-5 of a frame's largest energy
__device__ void build_tables(FbTables& tb, int tid, int nthr) {
  const double mel_lo = 1127.0 * log1p(20.0 / 700.0), mel_hi = 1127.0 * log1p(8000.0 / 700.0);
  const double delta = (mel_hi - mel_lo) / (FB_MEL + 1);
  for (int n = tid; n < FB_WIN; n += nthr) tb.win[n] = (float)pow(0.5 - 0.5 * cospi(2.0 * n / (FB_WIN - 1)), 0.85);
  for (int m = tid; m < FB_HALF; m += nthr) {
    double s, c;
    sincospi(-2.0 * m / FB_HALF, &s, &c);
    tb.tw_re[m] = (float)c; tb.tw_im[m] = (float)s;
    sincospi(-2.0 * m / FB_NFFT, &s, &c);
    tb.rs_re[m] = (float)c; tb.rs_im[m] = (float)s;
    const double u = (1127.0 * log1p(31.25 * m / 700.0) - mel_lo) / delta;
    const double f = floor(u);
    tb.fl[m] = (int)f;
    tb.frac[m] = (float)(u - f);
  }
  __syncthreads();
  for (int m = tid; m < FB_MEL + 2; m += nthr) {
    int c = 0;
    for (int k = 0; k < FB_HALF; ++k) c += (tb.fl[k] < m || (tb.fl[k] == m && tb.frac[k] == 0.0f)) ? 1 : 0;
    tb.kb[m] = c;
  }
}

__device__ __forceinline__ int64_t frames_of(int64_t n) { return n >= FB_WIN ? 1 + (n - FB_WIN) / FB_SHIFT : 0; }

// grid (ceil(T / 32), B), 256 threads; wave w computes frames w, w + 4, ... of the tile.  LDS ~56 KiB.
__global__ __launch_bounds__(256) void fbank_frames_kernel(const float* __restrict__ wave, int64_t S, const int64_t* __restrict__ n_samples,
                                                           int64_t T, float* __restrict__ out, int64_t* __restrict__ n_frames,
                                                           double* __restrict__ partial) {
  __shared__ FbSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.y, tile = blockIdx.x, t0 = tile * FB_TILE;
  int64_t n = n_samples[b];
  n = n < 0 ? 0 : (n > S ? S : n);
  int64_t Ti = frames_of(n);
  Ti = Ti > T ? T : Ti;
  if (tile == 0 && tid == 0 && n_frames) n_frames[b] = Ti;
  float* orow = out + (b * T + t0) * FB_MEL;
  const int nf = (int)(T - t0 < FB_TILE ? T - t0 : FB_TILE);          // rows of this tile inside the output
  if (t0 >= Ti) {                                                      // padding rows only: zeros
    for (int i = tid; i < nf * FB_MEL / 4; i += 256) reinterpret_cast<f32x4*>(orow)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const int nvalid = (int)(Ti - t0 < FB_TILE ? Ti - t0 : FB_TILE);
  build_tables(sm.tab, tid, 256);

  // stage the tile's sample span once (16-byte loads where the row is aligned), zeros beyond the utterance
  const float* src = wave + b * S + t0 * FB_SHIFT;
  const int64_t avail64 = n - t0 * FB_SHIFT;
  const int avail = (int)(avail64 < FB_SPAN ? avail64 : FB_SPAN);
  if ((S & 3) == 0 && ((uintptr_t)wave & 15) == 0) {
    const int nq = avail >> 2;
    for (int q = tid; q < nq; q += 256) {
      const f32x4 v = reinterpret_cast<const f32x4*>(src)[q];
      sm.stage[4 * q] = v[0]; sm.stage[4 * q + 1] = v[1]; sm.stage[4 * q + 2] = v[2]; sm.stage[4 * q + 3] = v[3];
    }
    for (int i = (nq << 2) + tid; i < FB_SPAN; i += 256) sm.stage[i] = i < avail ? src[i] : 0.0f;
  } else {
    for (int i = tid; i < FB_SPAN; i += 256) sm.stage[i] = i < avail ? src[i] : 0.0f;
  }
  __syncthreads();

  const FbTables& tb = sm.tab;
  for (int it = 0; it < FB_TILE / FB_WAVES; ++it) {
    const int f = it * FB_WAVES + w;                                  // frame within the tile (uniform per wave)
    const float* x = sm.stage + f * FB_SHIFT;
    // DC removal: the frame mean of the scaled samples
    float acc = 0.f;
    for (int j = lane; j < FB_WIN; j += 64) acc += x[j] * 32768.0f;
    const float mean = wave_sum(acc) * (1.0f / FB_WIN);
    // pre-emphasis, Povey window, zero pad; z[n] = y[2n] + i y[2n + 1]
    float* zr = sm.re[w][0];
    float* zi = sm.im[w][0];
    for (int j = lane; j < FB_NFFT; j += 64) {
      float y = 0.f;
      if (j < FB_WIN) {
        const float xj = x[j] * 32768.0f - mean, xp = x[j > 0 ? j - 1 : 0] * 32768.0f - mean;
        y = (xj - 0.97f * xp) * tb.win[j];
      }
      if (j & 1) zi[fpad(j >> 1)] = y; else zr[fpad(j >> 1)] = y;
    }
    __syncthreads();
    // 256-point complex FFT: four radix-4 Stockham stages, lane j = one butterfly, ping-pong between the two buffers
    int cur = 0;
    for (int Ns = 1; Ns < FB_HALF; Ns *= 4) {
      const float* ar = sm.re[w][cur];
      const float* ai = sm.im[w][cur];
      float* br = sm.re[w][cur ^ 1];
      float* bi = sm.im[w][cur ^ 1];
      const int j = lane, k = j % Ns, step = 64 / Ns;
      float vr[4], vi[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = ar[fpad(j + r * 64)], pi = ai[fpad(j + r * 64)];
        const int m = r * k * step;
        const float cr = tb.tw_re[m], ci = tb.tw_im[m];
        vr[r] = pr * cr - pi * ci;
        vi[r] = pr * ci + pi * cr;
      }
      const float t0r = vr[0] + vr[2], t0i = vi[0] + vi[2], t1r = vr[0] - vr[2], t1i = vi[0] - vi[2];
      const float t2r = vr[1] + vr[3], t2i = vi[1] + vi[3], t3r = vi[1] - vi[3], t3i = vr[3] - vr[1];  // t3 = -i (v1 - v3)
      const int d = (j / Ns) * Ns * 4 + k;
      br[fpad(d)] = t0r + t2r;          bi[fpad(d)] = t0i + t2i;
      br[fpad(d + Ns)] = t1r + t3r;     bi[fpad(d + Ns)] = t1i + t3i;
      br[fpad(d + 2 * Ns)] = t0r - t2r; bi[fpad(d + 2 * Ns)] = t0i - t2i;
      br[fpad(d + 3 * Ns)] = t1r - t3r; bi[fpad(d + 3 * Ns)] = t1i - t3i;
      cur ^= 1;
      __syncthreads();
    }
    // real split: X[k] = (Z[k] + conj Z[256-k]) / 2 - i W^k (Z[k] - conj Z[256-k]) / 2, W = exp(-2 pi i / 512); power |X[k]|^2
    {
      const float* Zr = sm.re[w][cur];
      const float* Zi = sm.im[w][cur];
      float* P = sm.re[w][cur ^ 1];
      for (int k = lane; k < FB_HALF; k += 64) {
        const int kc = (FB_HALF - k) & (FB_HALF - 1);
        const float ar = Zr[fpad(k)], ai = Zi[fpad(k)], cr = Zr[fpad(kc)], ci = -Zi[fpad(kc)];
        const float er = 0.5f * (ar + cr), ei = 0.5f * (ai + ci);
        const float dr = 0.5f * (ar - cr), di = 0.5f * (ai - ci);
        const float orr = di, oi = -dr;                               // -i (Z[k] - conj Z[256-k]) / 2
        const float wr = tb.rs_re[k], wi = tb.rs_im[k];
        const float xr = er + wr * orr - wi * oi, xi = ei + wr * oi + wi * orr;
        P[fpad(k)] = xr * xr + xi * xi;
      }
    }
    __syncthreads();
    // mel filters: lane m sums its contiguous bin range; each bin feeds filters floor(u) (rising) and floor(u) - 1 (falling)
    {
      const float* P = sm.re[w][cur ^ 1];
      const int64_t t = t0 + f;
      for (int m = lane; m < FB_MEL; m += 64) {
        float e = 0.f;
        for (int k = tb.kb[m]; k < tb.kb[m + 2]; ++k) e += (tb.fl[k] == m ? tb.frac[k] : (tb.fl[k] == m + 1 ? 1.0f - tb.frac[k] : 0.0f)) * P[fpad(k)];
        const float v = e > 1.1920928955078125e-07f ? logf(e) : -15.942385152878742f;  // log(FLT_EPSILON), rounded once
        if (f < nvalid) {
          sm.tile[f][m] = v;
          orow[f * FB_MEL + m] = v;
        } else if (t < T) {
          orow[f * FB_MEL + m] = 0.0f;
        }
      }
    }
  }
  if (partial) {                                                     // per-tile partial sums, frames in order, fp64
    __syncthreads();
    if (tid < FB_MEL) {
      double s1 = 0.0, s2 = 0.0;
      for (int f = 0; f < nvalid; ++f) {
        const double v = sm.tile[f][tid];
        s1 += v;
        s2 += v * v;
      }
      double* p = partial + ((b * gridDim.x + tile) * 2) * FB_MEL;
      p[tid] = s1;
      p[FB_MEL + tid] = s2;
    }
  }
}

struct FbXform {
  int utt, norm_means, norm_vars, global_first, specaug, mask_mean, n_fmask, n_tmask;
  float mask_value;
  const float* gmean;
  const float* gstd;
  const int32_t* fmask;
  const int32_t* tmask;
};

// grid (ceil(T / 256), B), 256 threads: reduce the utterance's tile partials (tile order), fold the CMVN steps into one map
// (x - c) a + d per bin, then apply it and the SpecAugment masks to the block's frames, in place.
__global__ __launch_bounds__(256) void fbank_transform_kernel(float* __restrict__ out, const int64_t* __restrict__ n_samples, int64_t S,
                                                              int64_t T, const double* __restrict__ partial, int ntiles, FbXform x) {
  __shared__ float cc[FB_MEL], alpha[FB_MEL], beta[FB_MEL];
  __shared__ double s1sh[FB_MEL];
  __shared__ float mval;
  __shared__ int fm[FB_MAXMASK][2], tm[FB_MAXMASK][2];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y, c0 = (int64_t)blockIdx.x * FB_CHUNK;
  int64_t n = n_samples[b];
  n = n < 0 ? 0 : (n > S ? S : n);
  int64_t Ti = frames_of(n);
  Ti = Ti > T ? T : Ti;
  if (c0 >= Ti) return;
  if (tid < FB_MEL) {
    const int nt = (int)((Ti + FB_TILE - 1) / FB_TILE);
    const double* p = partial + (b * ntiles * 2) * FB_MEL;
    double a1 = 0.0, a2 = 0.0;
#pragma unroll 8
    for (int i = 0; i < nt; ++i) {
      a1 += p[(i * 2) * FB_MEL + tid];
      a2 += p[(i * 2 + 1) * FB_MEL + tid];
    }
    const double inv = 1.0 / (double)Ti;
    // the CMVN steps as y = (x - c) a + d per bin (the subtraction first, as the reference does it: no large a * x terms)
    double c = 0.0, a = 1.0, d = 0.0;
    double gm = 0.0, gs = 1.0;
    if (x.gmean) { gm = x.gmean[tid]; gs = x.gstd[tid]; }
    if (x.gmean && x.global_first) { c = gm; a = 1.0 / gs; }
    if (x.utt) {
      // statistics of what utterance_cmvn sees, y = (x - c) a: mean (mean_x - c) a, variance var_x a^2
      const double mean_x = a1 * inv, var_x = a2 * inv - mean_x * mean_x;
      const double var = var_x * a * a;
      if (x.norm_means) c = mean_x;
      if (x.norm_vars) a /= sqrt(var > 1e-10 ? var : 1e-10);
    }
    if (x.gmean && !x.global_first) { a /= gs; d = (d - gm) / gs; }
    cc[tid] = (float)c;
    alpha[tid] = (float)a;
    beta[tid] = (float)d;
    s1sh[tid] = a * (a1 - (double)Ti * c) + (double)Ti * d;            // column sum of the transformed spectrogram
  }
  if (tid < FB_MAXMASK) {
    const bool fo = tid < x.n_fmask, to = tid < x.n_tmask;
    fm[tid][0] = fo ? x.fmask[(b * x.n_fmask + tid) * 2] : 0;
    fm[tid][1] = fo ? x.fmask[(b * x.n_fmask + tid) * 2 + 1] : 0;
    tm[tid][0] = to ? x.tmask[(b * x.n_tmask + tid) * 2] : 0;
    tm[tid][1] = to ? x.tmask[(b * x.n_tmask + tid) * 2 + 1] : 0;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int m = 0; m < FB_MEL; ++m) s += s1sh[m];
    mval = x.mask_mean ? (float)(s / ((double)Ti * FB_MEL)) : x.mask_value;
  }
  __syncthreads();
  const int64_t c1 = c0 + FB_CHUNK < Ti ? c0 + FB_CHUNK : Ti;
  float* base = out + b * T * FB_MEL;
  const int64_t q0 = c0 * (FB_MEL / 4), q1 = c1 * (FB_MEL / 4);
  for (int64_t q = q0 + tid; q < q1; q += 256) {
    const int64_t t = q / (FB_MEL / 4);
    const int m0 = (int)(q % (FB_MEL / 4)) * 4;
    f32x4 v = reinterpret_cast<f32x4*>(base)[q];
    bool tmasked = false;
    if (x.specaug)
      for (int i = 0; i < x.n_tmask; ++i) tmasked |= (t >= tm[i][0] && t < tm[i][0] + tm[i][1]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + e;
      float y = (v[e] - cc[m]) * alpha[m] + beta[m];
      if (x.specaug) {
        bool mk = tmasked;
        for (int i = 0; i < x.n_fmask; ++i) mk |= (m >= fm[i][0] && m < fm[i][0] + fm[i][1]);
        if (mk) y = mval;
      }
      v[e] = y;
    }
    reinterpret_cast<f32x4*>(base)[q] = v;
  }
}

}  // namespace

extern "C" int64_t cst_fbank_workspace_bytes(int64_t B, int64_t T) {
  if (B <= 0 || T <= 0) return 0;
  return B * cst_ceil_div(T, FB_TILE) * 2 * FB_MEL * (int64_t)sizeof(double);
}

extern "C" int cst_fbank(const cst_fbank_desc* d, cst_stream stream) {
  CST_REQUIRE(d, "cst_fbank: null descriptor");
  CST_REQUIRE(d->wave && d->n_samples && d->out, "cst_fbank: null operand (wave / n_samples / out)");
  CST_REQUIRE(d->B > 0 && d->B < 65536 && d->S > 0 && d->T > 0 && d->T < (1LL << 31) / FB_MEL,
              "cst_fbank: bad shape B=%lld S=%lld T=%lld", (long long)d->B, (long long)d->S, (long long)d->T);
  CST_REQUIRE(((uintptr_t)d->out & 15) == 0, "cst_fbank: out must be 16-byte aligned");
  CST_REQUIRE(d->n_fmask >= 0 && d->n_fmask <= FB_MAXMASK && d->n_tmask >= 0 && d->n_tmask <= FB_MAXMASK,
              "cst_fbank: at most %d frequency and %d time masks per utterance", FB_MAXMASK, FB_MAXMASK);
  CST_REQUIRE(!d->specaugment || ((d->n_fmask == 0 || d->fmask) && (d->n_tmask == 0 || d->tmask)),
              "cst_fbank: specaugment needs its mask intervals");
  CST_REQUIRE((d->global_mean == nullptr) == (d->global_std == nullptr), "cst_fbank: global_cmvn needs both mean and std");
  const bool xform = d->utterance_cmvn || d->global_mean || d->specaugment;
  const int64_t ws = cst_fbank_workspace_bytes(d->B, d->T);
  if (xform) {
    CST_REQUIRE(d->workspace && ((uintptr_t)d->workspace & 7) == 0, "cst_fbank: transforms need an 8-byte aligned workspace");
    if (d->workspace_bytes < ws) {
      cst_set_error("cst_fbank: workspace of %lld bytes, %lld needed", (long long)d->workspace_bytes, (long long)ws);
      return CST_ERR_WORKSPACE;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const double bytes = 4.0 * d->B * d->S + 4.0 * d->B * d->T * FB_MEL * (xform ? 3.0 : 1.0);
  CstProfScope prof(CST_K_ELEMENTWISE, s, 0.0, bytes);
  prof.tag("fbank B=%lld S=%lld T=%lld xform=%d", (long long)d->B, (long long)d->S, (long long)d->T, (int)xform);
  const int ntiles = (int)cst_ceil_div(d->T, FB_TILE);
  hipLaunchKernelGGL(fbank_frames_kernel, dim3((unsigned)ntiles, (unsigned)d->B), dim3(256), 0, s, d->wave, d->S, d->n_samples, d->T,
                     d->out, d->n_frames, xform ? (double*)d->workspace : nullptr);
  int rc = cst_check_launch("cst_fbank: fbank_frames_kernel");
  if (rc != CST_OK || !xform) return rc;
  FbXform x{};
  x.utt = d->utterance_cmvn != 0;
  x.norm_means = d->norm_means != 0;
  x.norm_vars = d->norm_vars != 0;
  x.global_first = d->global_first != 0;
  x.specaug = d->specaugment != 0;
  x.mask_mean = d->mask_mean != 0;
  x.n_fmask = d->specaugment ? d->n_fmask : 0;
  x.n_tmask = d->specaugment ? d->n_tmask : 0;
  x.mask_value = d->mask_value;
  x.gmean = d->global_mean;
  x.gstd = d->global_std;
  x.fmask = d->fmask;
  x.tmask = d->tmask;
  hipLaunchKernelGGL(fbank_transform_kernel, dim3((unsigned)cst_ceil_div(d->T, FB_CHUNK), (unsigned)d->B), dim3(256), 0, s, d->out,
                     d->n_samples, d->S, d->T, (const double*)d->workspace, ntiles, x);
  return cst_check_launch("cst_fbank: fbank_transform_kernel");
}
