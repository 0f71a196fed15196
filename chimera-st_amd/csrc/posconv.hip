// posconv.hip — sliding-window kernels of the wav2vec2 positional convolution (bf16, 48 channels per group, k <= 128 taps).
//
// The implicit GEMM of gemm.hip reads, for output frame t, the contiguous k-frame window of one group as a row of its A operand;
// frame t + 1's row is the same window moved by 48 elements, so every K tile re-fetches data the workgroup already had (a 128-row
// tile pulls 1.5 MB through L2 -> LDS for 24 KB of distinct input).  Here the window is staged ONCE per workgroup, straight from the
// channels-last [B, T, C] tensor (no group-major copy), and the taps walk over it in LDS.
//
// Order of summation (unchanged, so y / z / dx / dw / db keep the bits of the GEMM route): v_mfma_f32_32x32x16_bf16, one accumulator
// chain per output element, K index = tap-major / channel-minor (forward, dX) or ascending frame index of the zero-padded
// [B, Tp] frame axis in blocks of 64 (dW), 16 K values per MFMA in ascending order, lanes 0-31 the low 8 and lanes 32-63 the high 8;
// the epilogue is gemm_common.h's epilogue_store8 itself.
#include "gemm_common.h"

namespace {
using namespace cstg;

constexpr int CG = 48;     // channels per group
constexpr int KMAX = 128;  // taps

// ---------------------------------------------------------------------------------------------------------------------
// forward / dX: out[b, m, g, co] = epilogue( sum_j sum_ci in[b, m - left + j, g, ci] * w[g][co][j][ci] )
// One workgroup = (group, utterance, block of 256 frames); 4 waves, wave w owns rows [64 w, 64 w + 64) x 64 columns (48 live).
// LDS: the window, (256 + k - 1) rows of 48 bf16 at a row stride of 56 elements (112 B = 28 dwords: 28 r mod 64 takes 16 distinct
// multiples of 4 for 16 rows that differ mod 16, which is what each 16-lane group of a ds_read_b128 fragment read touches ->
// conflict-free for every tap offset), then a two-stage ring of the weight, 4 taps (192 K values) x 48 rows per stage at a row
// stride of 200 elements (100 dwords = 36 mod 64: the same argument).  81 296 B: two workgroups per CU.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int FBM = 256;
constexpr int WLD = 56;
constexpr int WROWS = FBM + KMAX - 1;
constexpr int TAPS = 4;
constexpr int BLD = TAPS * CG + 8;
constexpr int WIN_BYTES = WROWS * WLD * 2;
constexpr int BST_BYTES = CG * BLD * 2;
constexpr int FWD_LDS = WIN_BYTES + 2 * BST_BYTES;
constexpr int FLDC = 64 + 4;
constexpr int BVEC = CG * TAPS * CG / 8;           // 16-byte vectors per weight stage (1152)
constexpr int NVB = (BVEC + 255) / 256;            // per thread
static_assert(WIN_BYTES % 16 == 0 && BST_BYTES % 16 == 0, "16-byte aligned LDS regions");
static_assert(FBM * FLDC * 4 <= FWD_LDS, "the fp32 epilogue staging reuses the operand space");
static_assert(FWD_LDS <= 160 * 1024, "LDS of one CU");

struct PcFwdParams {
  GemmParams e;  // epilogue operands only (bias, act, aux_out, resid, C and their strides)
  const bf16_t* x;
  const bf16_t* w;
  const int32_t* m_len;
  int B, T, C, G, k, left, nblk;
};

__global__ __launch_bounds__(256, 2) void posconv_win_kernel(PcFwdParams q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* win = reinterpret_cast<bf16_t*>(smem);
  bf16_t* bst = reinterpret_cast<bf16_t*>(smem + WIN_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // XCD-contiguous item order (bijective, as in gemm.hip): the workgroups of one group share its 590 KB of weight in one L2
  const int per = q.B * q.nblk, total = q.G * per;
  int item;
  {
    const int id = blockIdx.x, n8 = total / 8, r8 = total % 8, xcd = id % 8, loc = id / 8;
    item = (xcd < r8 ? xcd * (n8 + 1) : r8 * (n8 + 1) + (xcd - r8) * n8) + loc;
  }
  const int g = item / per, rem = item % per, b = rem / q.nblk, blk = rem % q.nblk;
  const int m0 = blk * FBM, k = q.k, T = q.T;
  bool live = true;
  if (q.m_len) live = m0 < q.m_len[b];  // rows from m_len[b] on have all-zero windows: zero accumulators, epilogue only
  const int nst = live ? (k + TAPS - 1) / TAPS : 0;

  const bf16_t* xb = q.x + (int64_t)b * T * q.C + g * CG;
  const bf16_t* wb = q.w + (int64_t)g * CG * k * CG;
  u32x4 rb[NVB];
  auto load_b = [&](int s) {
    const int j0 = s * TAPS;
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int v = tid + 256 * i, row = v / (TAPS * 6), c = v % (TAPS * 6);
      const bool ok = v < BVEC && j0 + c / 6 < k;
      const u32x4 zero = {0, 0, 0, 0};
      rb[i] = ok ? *reinterpret_cast<const u32x4*>(wb + ((int64_t)row * k + j0) * CG + c * 8) : zero;
    }
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int v = tid + 256 * i, row = v / (TAPS * 6), c = v % (TAPS * 6);
      if (v < BVEC) *reinterpret_cast<u32x4*>(bst + buf * (CG * BLD) + row * BLD + c * 8) = rb[i];
    }
  };

  if (nst) {
    load_b(0);
    const int nrows = FBM + k - 1;
    for (int v = tid; v < nrows * 6; v += 256) {
      const int r = v / 6, c = v % 6, t = m0 - q.left + r;
      u32x4 val = {0, 0, 0, 0};
      if (t >= 0 && t < T) val = *reinterpret_cast<const u32x4*>(xb + (int64_t)t * q.C + c * 8);
      *reinterpret_cast<u32x4*>(win + r * WLD + c * 8) = val;
    }
    store_b(0);
  }
  __syncthreads();

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int lrow = lane & 31, lk = 8 * (lane >> 5);
  const int brow1 = (32 + lrow) < CG ? 32 + lrow : CG - 1;  // columns 48..63 do not exist: clamped (never stored)
  for (int s = 0; s < nst; ++s) {
    const bool more = s + 1 < nst;
    if (more) load_b(s + 1);
    const bf16_t* sb = bst + (s & 1) * (CG * BLD);
    const int nt = (k - s * TAPS) < TAPS ? (k - s * TAPS) : TAPS;
    const bf16_t* wr = win + (wave * 64 + lrow + s * TAPS) * WLD + lk;
    const bf16_t* br0 = sb + lrow * BLD + lk;
    const bf16_t* br1 = sb + brow1 * BLD + lk;
    if (nt == TAPS) {
      // the 12 k16 steps of a full stage, fragments of step c + 1 requested before the MFMAs of step c (a wave's LDS latency would
      // otherwise stand between every two MFMA pairs)
      Frag<bf16_t> fa[2][2], fb[2][2];
      auto rd = [&](int c, int buf) {
        const int jj = c / 3, kk = (c % 3) * 16;
        frag_load_contig(fa[buf][0], wr + jj * WLD + kk);
        frag_load_contig(fa[buf][1], wr + (jj + 32) * WLD + kk);
        frag_load_contig(fb[buf][0], br0 + jj * CG + kk);
        frag_load_contig(fb[buf][1], br1 + jj * CG + kk);
      };
      rd(0, 0);
#pragma unroll
      for (int c = 0; c < TAPS * 3; ++c) {
        if (c + 1 < TAPS * 3) rd(c + 1, (c + 1) & 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) mma16(acc[i][j], fa[c & 1][i], fb[c & 1][j]);
      }
    } else {
      for (int jj = 0; jj < nt; ++jj) {
#pragma unroll
        for (int kk = 0; kk < CG; kk += 16) {
          Frag<bf16_t> fa[2], fb[2];
          frag_load_contig(fa[0], wr + jj * WLD + kk);
          frag_load_contig(fa[1], wr + (jj + 32) * WLD + kk);
          frag_load_contig(fb[0], br0 + jj * CG + kk);
          frag_load_contig(fb[1], br1 + jj * CG + kk);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) mma16(acc[i][j], fa[i], fb[j]);
        }
      }
    }
    if (more) store_b((s + 1) & 1);
    __syncthreads();
  }

  // epilogue: accumulators -> LDS (fp32) -> 8-column vectors -> epilogue_store8 (bias, aux_out, GELU, residual, 16-byte stores)
  float* stage = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[(wave * 64 + i * 32 + acc_row(r, lane)) * FLDC + j * 32 + lrow] = acc[i][j][r];
  __syncthreads();
  const int64_t cofs = (int64_t)b * T * q.C + g * CG, bofs = (int64_t)g * CG;
  for (int v = tid; v < FBM * (CG / 8); v += 256) {
    const int rl = v / (CG / 8), cl = (v % (CG / 8)) * 8;
    const int64_t row = m0 + rl;
    if (row >= T) continue;
    float x8[8];
    const f32x4 a = *reinterpret_cast<const f32x4*>(stage + rl * FLDC + cl);
    const f32x4 c = *reinterpret_cast<const f32x4*>(stage + rl * FLDC + cl + 4);
    x8[0] = a[0]; x8[1] = a[1]; x8[2] = a[2]; x8[3] = a[3]; x8[4] = c[0]; x8[5] = c[1]; x8[6] = c[2]; x8[7] = c[3];
    epilogue_store8<bf16_t>(q.e, cofs, bofs, row, cl, x8);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// dW: dw[g co][ci][j] = sum_kappa dzp[kappa + lp][co] * xp[kappa + j][ci] over the zero-padded frame axis of the whole batch
// (row rho = b Tp + p; xp frame = p - padl, dzp frame = p - lp; zero outside [0, T)), kappa ascending in blocks of 64 — the K
// order of the GEMM route with one split.  One workgroup = (group, block of 8 taps): 64 x 384 accumulators (48 x 384 live), wave w
// owns taps 2 w, 2 w + 1.  Per K block the 64 dz rows and the 64 + 7 window rows of x are fetched once, with global_load_lds, into a
// 6-stage ring (5 blocks = 65 KB in flight per CU); rows outside an utterance read a zero line instead.  The LDS images are
// unpadded 96-byte rows: the window operand is then the flat image itself, B[kappa][j 48 + ci] = image[48 kappa + (j 48 + ci)], and
// both operands are read with ds_read_b64_tr_b16 (rows k .. k + 3 at a stride of 96 B: rows 0 and 3 share 32 of their 64 bytes'
// banks, a 2-way conflict on half the lanes — accepted: 10 such reads per 6 MFMAs stay under the MFMA time).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int DTJ = 8;                       // taps per workgroup
constexpr int DNS = 6;                       // ring stages
constexpr int DZ_BYTES = 64 * CG * 2;        // 6 144: six 1-KiB DMA groups
constexpr int DX_ROWS = 64 + DTJ - 1;        // 71
constexpr int DX_BYTES = 7 * 1024;           // seven groups (74.67 rows: the last 3.67 are fetched and never read)
constexpr int DST_BYTES = DZ_BYTES + DX_BYTES;
constexpr int DGROUPS = DST_BYTES / 1024;    // 13 per K block: wave 0 issues 4, the others 3
constexpr int DW_LDS = DNS * DST_BYTES;
constexpr int DKLIST = 1024;
static_assert(DX_ROWS * CG * 2 <= DX_BYTES, "window rows of one K block");
static_assert(CG * DTJ * CG * 4 <= DW_LDS, "the fp32 epilogue staging reuses the ring");
static_assert(DW_LDS + DKLIST * 4 + 64 <= 160 * 1024, "LDS of one CU");

__device__ u32x4 pc_zero_line[1];  // source of every ring row that lies outside an utterance (zero-initialised)

struct PcDwParams {
  const bf16_t* dz;
  const bf16_t* x;
  bf16_t* dw;   // [G * 48][48][k]
  bf16_t* db;   // [G * 48] or nullptr
  const uint32_t* k_live; uint32_t k_epoch;
  int B, T, C, G, k, Tp, lp, padl, nkb, ntb;
  uint32_t magic;  // floor(2^32 / Tp)
};

template <int N>
__device__ __forceinline__ void pc_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

__global__ __launch_bounds__(256, 1) void posconv_dw_kernel(PcDwParams q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int klist[DKLIST];
  __shared__ int klist_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-contiguous item order (bijective): the tap blocks of one group run on ONE XCD, whose L2 then fetches that group's 96-byte
  // column of every frame once for all of them (dealt round-robin, every XCD's L2 would fetch every group's column)
  int item;
  {
    const int total = q.G * q.ntb, id = blockIdx.x, n8 = total / 8, r8 = total % 8, xcd = id % 8, loc = id / 8;
    item = (xcd < r8 ? xcd * (n8 + 1) : r8 * (n8 + 1) + (xcd - r8) * n8) + loc;
  }
  const int g = item / q.ntb, tb = item % q.ntb, j0 = tb * DTJ;
  const int T = q.T, Tp = q.Tp;

  // live K blocks, compacted in ascending order (dead ones hold only zero dz rows: each would add 0 to every accumulator)
  const bool kskip = q.k_live != nullptr && q.nkb <= DKLIST;
  int nk = q.nkb;
  if (kskip) {
    if (wave == 0) {
      int seen = 0;
      for (int base = 0; base < q.nkb; base += 64) {
        const int kt = base + lane;
        const bool lv = kt < q.nkb && q.k_live[kt] == q.k_epoch;
        const uint64_t m = __builtin_amdgcn_ballot_w64(lv);
        if (lv) klist[seen + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = kt;
        seen += __builtin_popcountll(m);
      }
      if (lane == 0) klist_n = seen;
    }
    __syncthreads();
    nk = klist_n;
  }

  const bf16_t* dzg = q.dz + g * CG;
  const bf16_t* xg = q.x + g * CG;
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(pc_zero_line);
  // DMA group d of a stage = LDS bytes [1024 d, 1024 d + 1024); lane l fills 16-byte chunk c = 64 d + l: groups 0..5 are the dz image
  // (row c / 6, chunk c % 6), groups 6..12 the window image.  This wave owns groups wave + 4 i.  The block's first row is split into
  // (utterance, position) once per group on the scalar unit (multiplication by floor(2^32 / Tp), corrected); a lane only adds its row.
  int rowv[4], chv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = wave + 4 * i, c = (d >= 6 ? d - 6 : d) * 64 + lane;
    rowv[i] = c / 6;
    chv[i] = (c % 6) * 8;
  }
  auto issue = [&](int kb, int stage) {
    char* sbase = smem + stage * DST_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = wave + 4 * i;
      if (d < DGROUPS) {  // (wave-uniform)
        const bool is_x = d >= 6;
        const uint32_t r0 = (uint32_t)(kb * 64 + (is_x ? j0 : q.lp));  // first row of the image on the padded frame axis
        uint32_t bq = __umulhi(r0, q.magic), rem = r0 - bq * (uint32_t)Tp;
        while (rem >= (uint32_t)Tp) { rem -= (uint32_t)Tp; ++bq; }
        int bb = (int)bq, pp = (int)rem + rowv[i];
        while (pp >= Tp) { pp -= Tp; ++bb; }
        const int t = pp - (is_x ? q.padl : q.lp);
        const bool ok = bb < q.B && (unsigned)t < (unsigned)T;
        const bf16_t* src = ok ? (is_x ? xg : dzg) + ((bb * T + t) * q.C + chv[i]) : zero;  // (B T C < 2^31: checked at launch)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(sbase + d * 1024), 16, 0, 0);
      }
    }
  };

  f32x16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  // bias gradient (tap block 0 only): thread t adds rows t / 8 and 32 + t / 8 of every K block for columns 8 (t % 8) .. + 8, then the
  // 32 partial sums per column are added in row order — the chain of gemm.hip's colsum
  const bool do_cs = q.db != nullptr && tb == 0;
  float cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.0f;

  // Every LDS read of the ring inside the loop is inline assembly with its own counted lgkmcnt waits: the compiler orders a plain LDS
  // load behind ALL outstanding global_load_lds writes (s_waitcnt vmcnt(0) in front of the first fragment read of an iteration),
  // which would leave one K block in flight instead of five.
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const uint32_t klist0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int*)klist;
  uint32_t fofs[5];  // per-lane byte offset of fragment f's first transpose read inside a stage (2 of dz, 3 of the window)
  {
    const int sl = lane & 15, lk = 8 * (lane >> 5);
    const int col = 16 * ((lane >> 4) & 1) + 4 * (sl & 3), krow = lk + (sl >> 2);
    fofs[0] = (uint32_t)((krow * CG + col) * 2);
    fofs[1] = fofs[0] + 64;
#pragma unroll
    for (int j = 0; j < 3; ++j) fofs[2 + j] = (uint32_t)(DZ_BYTES + (krow * CG + wave * 96 + j * 32 + col) * 2);
  }
  const uint32_t csofs = (uint32_t)(((tid >> 3) * CG + (tid & 7) * 8) * 2);
  auto next_block = [&](int it) {
    if (!kskip) return it;
    int kt;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(kt) : "v"(klist0 + 4u * (uint32_t)it) : "memory");
    return __builtin_amdgcn_readfirstlane(kt);
  };
#pragma unroll
  for (int s = 0; s < DNS - 1; ++s)
    if (s < nk) issue(next_block(s), s);
  for (int it = 0; it < nk; ++it) {
    const int issued = (it + DNS - 1 < nk) ? it + DNS - 1 : nk;
    if (issued - it - 1 == DNS - 2) {
      if (wave == 0) pc_wait_vmcnt<(DNS - 2) * 4>();
      else pc_wait_vmcnt<(DNS - 2) * 3>();
    } else {
      pc_wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();  // block `it` has landed for every wave, and nobody still reads the stage the next issue overwrites
    if (it + DNS - 1 < nk) issue(next_block(it + DNS - 1), (it + DNS - 1) % DNS);
    const uint32_t sbase = lds0 + (uint32_t)((it % DNS) * DST_BYTES);
    if (do_cs && (tid & 7) < 6) {
      u32x4 v0, v1;
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:3072\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(v0), "=&v"(v1) : "v"(sbase + csofs) : "memory");
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cs[2 * e] += __uint_as_float(v0[e] << 16);
        cs[2 * e + 1] += __uint_as_float(v0[e] & 0xffff0000u);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cs[2 * e] += __uint_as_float(v1[e] << 16);
        cs[2 * e + 1] += __uint_as_float(v1[e] & 0xffff0000u);
      }
    }
    // k16 step kk: rows kk .. kk + 16 of both images (1 536 bytes further per step; the second read of a fragment 4 rows = 384 bytes on);
    // the 10 reads of step kk + 1 are requested before the MFMAs of step kk, which wait for their own 10 only (LDS returns in order)
    v4s_t fr[2][5][2];
    auto rd = [&](int kk, int buf) {
#pragma unroll
      for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fr[buf][f][h]) : "v"(sbase + fofs[f] + (uint32_t)(kk * 1536 + h * 384)));
    };
    rd(0, 0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk & 1;
      if (kk < 3) {
        rd(kk + 1, c ^ 1);
        asm volatile("s_waitcnt lgkmcnt(10)"
                     : "+v"(fr[c][0][0]), "+v"(fr[c][0][1]), "+v"(fr[c][1][0]), "+v"(fr[c][1][1]), "+v"(fr[c][2][0]), "+v"(fr[c][2][1]),
                       "+v"(fr[c][3][0]), "+v"(fr[c][3][1]), "+v"(fr[c][4][0]), "+v"(fr[c][4][1]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(fr[c][0][0]), "+v"(fr[c][0][1]), "+v"(fr[c][1][0]), "+v"(fr[c][1][1]), "+v"(fr[c][2][0]), "+v"(fr[c][2][1]),
                       "+v"(fr[c][3][0]), "+v"(fr[c][3][1]), "+v"(fr[c][4][0]), "+v"(fr[c][4][1]));
      }
      Frag<bf16_t> fg[5];
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        const v4s_t x = fr[c][f][0], y = fr[c][f][1];
        u16x8 t;
        t[0] = (unsigned short)x[0]; t[1] = (unsigned short)x[1]; t[2] = (unsigned short)x[2]; t[3] = (unsigned short)x[3];
        t[4] = (unsigned short)y[0]; t[5] = (unsigned short)y[1]; t[6] = (unsigned short)y[2]; t[7] = (unsigned short)y[3];
        fg[f].v = __builtin_bit_cast(bf16x8, t);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) mma16(acc[i][j], fg[i], fg[2 + j]);
    }
  }
  __syncthreads();

  if (do_cs) {  // (block-uniform)
    float* red = reinterpret_cast<float*>(smem);  // [32][64]
    if ((tid & 7) < 6) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[(tid >> 3) * 64 + (tid & 7) * 8 + e] = cs[e];
    }
    __syncthreads();
    if (tid < CG) {
      float tot = 0.0f;
      for (int r = 0; r < 32; ++r) tot += red[r * 64 + tid];
      DT<bf16_t>::st(q.db + g * CG + tid, tot);
    }
    __syncthreads();
  }

  // epilogue: fp32 accumulators -> LDS [co][n = jj 48 + ci] -> dw[g co][ci][j0 + jj] in bf16 (8 consecutive taps = 16 bytes)
  float* stage = reinterpret_cast<float*>(smem);
  constexpr int SLD = DTJ * CG;  // 384
  const int lrow = lane & 31;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = i * 32 + acc_row(r, lane);
        if (co < CG) stage[co * SLD + wave * 96 + j * 32 + lrow] = acc[i][j][r];
      }
  __syncthreads();
  const int k = q.k;
  const bool vec = (k % 8) == 0 && j0 + DTJ <= k;
  for (int v = tid; v < CG * CG; v += 256) {
    const int co = v / CG, ci = v % CG;
    bf16_t* dst = q.dw + ((int64_t)(g * CG + co) * CG + ci) * k + j0;
    float x8[8];
#pragma unroll
    for (int jj = 0; jj < DTJ; ++jj) x8[jj] = stage[co * SLD + jj * CG + ci];
    if (vec) store8(dst, x8);
    else
      for (int jj = 0; jj < DTJ && j0 + jj < k; ++jj) DT<bf16_t>::st(dst + jj, x8[jj]);
  }
}

int posconv_win_launch(const void* in, const void* w, const void* bias, void* out, void* z, const void* resid, const int32_t* m_len,
                       int64_t B, int64_t T, int64_t C, int64_t G, int64_t k, int64_t left, int act, hipStream_t s, const char* what) {
  CST_REQUIRE(in && w && out, "%s: null operand", what);
  CST_REQUIRE(B > 0 && T > 0 && G > 0 && C == G * CG, "%s: needs C = 48 * groups (B %lld T %lld C %lld groups %lld)", what, (long long)B,
              (long long)T, (long long)C, (long long)G);
  CST_REQUIRE(k >= 1 && k <= KMAX && left >= 0 && left < k, "%s: taps %lld (left %lld) outside 1..%d", what, (long long)k, (long long)left, KMAX);
  CST_REQUIRE(B * T * C < (1ll << 31), "%s: tensor too large", what);
  const int64_t nblk = cst_ceil_div(T, FBM);
  CST_REQUIRE(G * B * nblk < (1ll << 31), "%s: grid too large", what);
  PcFwdParams q = {};
  q.e.N = CG; q.e.alpha = 1.0f; q.e.vec_epi = 1;
  q.e.C = out; q.e.ldc = C;
  q.e.bias = bias; q.e.bias_mode = bias ? CST_BIAS_COL : CST_BIAS_NONE;
  q.e.act = act;
  q.e.aux_out = z; q.e.ld_aux_out = C;
  q.e.resid = resid; q.e.ld_resid = C;
  q.x = (const bf16_t*)in; q.w = (const bf16_t*)w; q.m_len = m_len;
  q.B = (int)B; q.T = (int)T; q.C = (int)C; q.G = (int)G; q.k = (int)k; q.left = (int)left; q.nblk = (int)nblk;
  static_assert(FWD_LDS <= 160 * 1024, "checked against the CU's LDS");
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&posconv_win_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, FWD_LDS);
    attr_set = true;
  }
  const double flops = 2.0 * (double)B * T * C * CG * k;
  const double bytes = 2.0 * ((double)B * T * C * 3 + (double)C * CG * k);
  CstProfScope prof(CST_K_GEMM, s, flops, bytes);
  prof.tag("%s B=%lld T=%lld C=%lld k=%lld", what, (long long)B, (long long)T, (long long)C, (long long)k);
  hipLaunchKernelGGL(posconv_win_kernel, dim3((unsigned)(G * B * nblk)), dim3(256), FWD_LDS, s, q);
  return cst_check_launch(what);
}
}  // namespace

extern "C" int cst_posconv_fwd(const void* x, const void* w, const void* bias, void* y, void* z, const int32_t* m_len, int64_t B, int64_t T,
                               int64_t C, int64_t groups, int64_t k, cst_stream stream) {
  return posconv_win_launch(x, w, bias, y, z, x, m_len, B, T, C, groups, k, k / 2, CST_ACT_GELU, (hipStream_t)stream, "cst_posconv_fwd");
}

extern "C" int cst_posconv_dx(const void* dz, const void* wflip, const void* dy, void* dx, const int32_t* m_len, int64_t B, int64_t T,
                              int64_t C, int64_t groups, int64_t k, cst_stream stream) {
  return posconv_win_launch(dz, wflip, nullptr, dx, nullptr, dy, m_len, B, T, C, groups, k, k - 1 - k / 2, CST_ACT_NONE, (hipStream_t)stream,
                            "cst_posconv_dx");
}

extern "C" int cst_posconv_dw(const void* dz, const void* x, void* dw, void* db, const uint32_t* k_live, uint32_t k_epoch, int64_t B,
                              int64_t T, int64_t C, int64_t groups, int64_t k, cst_stream stream) {
  CST_REQUIRE(dz && x && dw, "cst_posconv_dw: null operand");
  CST_REQUIRE(B > 0 && T > 0 && groups > 0 && C == groups * CG, "cst_posconv_dw: needs C = 48 * groups");
  CST_REQUIRE(k >= 1 && k <= KMAX, "cst_posconv_dw: taps %lld outside 1..%d", (long long)k, KMAX);
  const int64_t Tp = T + k - 1 + (k % 2 == 0 ? 1 : 0);
  CST_REQUIRE((B + 2) * T * C < (1ll << 31) && B * Tp + 128 < (1ll << 31), "cst_posconv_dw: tensor too large");
  PcDwParams q = {};
  q.dz = (const bf16_t*)dz; q.x = (const bf16_t*)x; q.dw = (bf16_t*)dw; q.db = (bf16_t*)db;
  q.k_live = k_live; q.k_epoch = k_epoch;
  q.B = (int)B; q.T = (int)T; q.C = (int)C; q.G = (int)groups; q.k = (int)k; q.Tp = (int)Tp;
  q.padl = (int)(k / 2); q.lp = (int)(k - 1 - k / 2);
  q.nkb = (int)cst_ceil_div(B * Tp - (k - 1), 64);
  q.ntb = (int)cst_ceil_div(k, DTJ);
  q.magic = (uint32_t)((1ull << 32) / (uint64_t)Tp);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&posconv_dw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DW_LDS);
    attr_set = true;
  }
  hipStream_t s = (hipStream_t)stream;
  const double flops = 2.0 * (double)B * T * C * CG * k;
  const double bytes = 2.0 * ((double)B * T * C * 2 * q.ntb + (double)C * CG * k);
  CstProfScope prof(CST_K_GEMM, s, flops, bytes);
  prof.tag("cst_posconv_dw B=%lld T=%lld C=%lld k=%lld", (long long)B, (long long)T, (long long)C, (long long)k);
  hipLaunchKernelGGL(posconv_dw_kernel, dim3((unsigned)(groups * q.ntb)), dim3(256), DW_LDS, s, q);
  return cst_check_launch("cst_posconv_dw");
}
