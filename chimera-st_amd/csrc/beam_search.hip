// beam_search.hip — the search step of the device-resident decode loop (decode.hip holds the decoder-layer kernels of a step):
// search.py BeamSearch.step (:109-144), its Sampling and diverse variants, and the masks and eos / finalize bookkeeping of
// fairseq/sequence_generator.py:_generate (:286-541), as two kernels per step that read the step counter from DEVICE memory like the
// rest of the captured launch sequence: one workgroup per hypothesis row reduces the row's logits to its candidates, one workgroup per
// sentence merges them, finalises hypotheses and writes the next step's token / score / ancestry rows.
#include "cst_common.h"
#include <limits.h>
#include <type_traits>

namespace {

struct BeamP {
  int bsz, beam, vocab, max_len;
  int pad, unk, eos, min_len;
  float unk_penalty, len_penalty, inv_temperature;
  int normalize_scores;
  const void* logits; int64_t ld_logits;
  int32_t* step;
  int64_t* tokens; float* scores; int32_t* anc;
  uint8_t* cands_to_ignore; uint8_t* finished; int32_t* nfinal; int32_t* num_remaining;
  int64_t* fin_tokens; float* fin_pos; float* fin_score; int32_t* fin_len;
  int ngram, prefix_len;          // --no-repeat-ngram-size (0 = off, else >= 2) / width of prefix_tokens (0 = off)
  const int64_t* prefix_tokens;   // [bsz][prefix_len], padded with `pad`
  int sample_topk;                // --sampling-topk (0 = off); read by the sampling kernels only
  float sample_topp;              // --sampling-topp (<= 0 = off; wins over top-k)
  const uint32_t* sample_key;     // device [1]: the 32-bit key of this call's draws, read at every step
  int div_groups;                 // --diverse-beam-groups G (read by the DIV == 1 merge kernels only)
  float div_strength;             // --diverse-beam-strength S >= 0
  float sibling_rate;             // --diversity-rate R >= 0 (read by the DIV == 2 merge kernels only)
  int32_t* fin_anc;               // optional [bsz][beam][L1]: the ancestry row of every finalised hypothesis
};

__global__ void beam_init_kernel(BeamP p, int32_t* ticket) {
  const int h = blockIdx.x, bbsz = p.bsz * p.beam, L1 = p.max_len + 1, LT = p.max_len + 2;
  for (int buf = 0; buf < 2; ++buf) {
    int64_t* tk = p.tokens + ((int64_t)buf * bbsz + h) * LT;
    float* sc = p.scores + ((int64_t)buf * bbsz + h) * L1;
    int32_t* an = p.anc + ((int64_t)buf * bbsz + h) * L1;
    for (int j = threadIdx.x; j < LT; j += blockDim.x) tk[j] = j == 0 ? p.eos : p.pad;
    for (int j = threadIdx.x; j < L1; j += blockDim.x) {
      sc[j] = 0.0f;
      an[j] = j == 0 ? h : 0;
    }
  }
  if (threadIdx.x == 0) {
    p.fin_len[h] = 0;
    p.fin_score[h] = 0.0f;
    if (h % p.beam == 0) {
      const int s = h / p.beam;
      p.finished[s] = 0;
      p.nfinal[s] = 0;
      for (int b = 0; b < p.beam; ++b) p.cands_to_ignore[s * p.beam + b] = 0;
    }
    if (h == 0) {
      *p.step = 0;
      *p.num_remaining = p.bsz;
      *ticket = 0;
    }
  }
}

__device__ __forceinline__ bool cand_better(float x, int i, float y, int j) { return x > y || (x == y && i < j); }
constexpr int BEAM_MAX = 20, KMAX_ALL = 2 * BEAM_MAX;

// ---- beam search step, kernel 1 of 2: one workgroup per hypothesis ROW -------------------------------------------------------
// (a) fp32 log-softmax statistics of the row (utils.py:469-473 via models/fairseq_decoder.py:58-79; block_lse), (b) the masks of the
// generator (mask_lprob) and the cumulative-score add of search.py:121-126, (c) the row's top-(2*beam) candidates in descending (value,
// then ascending token) order -> cand_val / cand_tok [row][2*beam] — or, with SAMP, the row's draws (beam_row_sample_tail).
// Two bodies behind the one kernel template: beam_row_regs keeps the row in registers (NV 16-byte vectors per thread), beam_row_wide
// (NV == 0) re-reads a row of any length from memory on every scan.
constexpr int ENS_MAX = 8;

// ENS (checkpoint ensembles, sequence_generator.py EnsembleModel.forward_decoder :806-868): (a) becomes, over the e.n members' rows,
//   lse_n = logsumexp_v(l_n[v] / T),   lp[v] = log(sum_n exp(l_n[v] / T - lse_n)) - log N          (all fp32, never stored in bf16)
// in two sweeps over the members: the first gathers every member's (max, sum) — block_lse: wave shuffles, ONE barrier for all members —
// the second re-reads the rows (L2 hits) and folds a_n = l_n / T - lse_n into a per-element running (max, sum) over the members
// (lse_merge, then ens_lprob), so the exp never sees more than a_n - max_n a_n <= 0 and an element that is -inf in every member stays
// -inf.  A member whose row has no finite lse (NaN logits, an all -inf row) makes the whole row NaN like the reference's stack +
// logsumexp; (b) and (c) are shared.
struct EnsP {
  int n;
  float temperature, log_n;
  const void* logits[ENS_MAX];
  float* lprobs_out;  // optional [rows][ld_logits] fp32: lp before the masks of (b)
};
struct NoEns {};  // what a kernel without ENS takes in EnsP's place: no kernel argument bytes
template <bool ENS> using EnsArg = std::conditional_t<ENS, EnsP, NoEns>;

// LM (shallow fusion with a target-side language model, sequence_generator.py:318-324): the LM's logits row hs — same rows, vocabulary,
// ld_logits, dtype and alignment as `logits` — gets its own (max, sum) in the block_lse call of (a) (one more slot, no more barriers), and
//   lm_lp[v] = x_lm[v] - lse_lm   (NO temperature: the reference normalises the raw LM output),   lp'[v] = fl(lp[v] + fl(w * lm_lp[v]))
// replaces lp (single or ensemble-combined, after the temperature) before (b): the reference's `probs * w`, then `lprobs += probs`, before
// any mask.  The LM row is re-read (an L2 hit) where lp' is formed instead of being held in registers next to the model's row.  A NaN LM row
// or one without a finite entry has no finite lse: every lm_lp is NaN, so is the row, and the first mask of (b) makes it -inf.
struct LmP {
  const void* logits;
  float weight;
  float* lprobs_out;  // optional [rows][ld_logits] fp32: lp' before the masks of (b)
};
struct NoLm {};  // like NoEns
template <bool LM> using LmArg = std::conditional_t<LM, LmP, NoLm>;
// lp' of one element (no contraction to an fma: the reference rounds the product)
__device__ __forceinline__ float lm_fuse(float lp, float w, float x_lm, float lse_lm) { return __fadd_rn(lp, __fmul_rn(w, x_lm - lse_lm)); }

// LEX (lexical constraints, search.py LexicallyConstrainedBeamSearch :210-523 with token_generation_constraints.py; cst_beam_step_lex):
// every hypothesis row carries a constraint STATE, every sentence a TABLE its states move in, both int32 words in the workspace of
// cst_lex_desc (cst_lex_init builds the tables and the root states):
//   table  [LEX_TBL_W]: [0] nd = the sentence's DISTINCT constraint tokens, [1] n, [2] representation, then four arrays of LEX_NODES:
//          ordered (1): n = constraint tokens in all; A = the concatenated constraints, B = 1 where a constraint ends;
//          unordered (2): n = trie nodes, node 0 the root; A = the node's token, B = its parent, C = constraints that END at the node
//          (terminal), D = constraints that end at or below it (num_constraints).  A node's children are found by scanning the <= 32
//          nodes for (parent, token): the table sits in LDS wherever it is walked.
//   state  [LEX_SW]: NODE (ordered: the index into A, -1 = root), BANK (constraint tokens generated), FIN, NNEXT and NEXT[16] (the
//          state's next tokens, ascending and distinct — derived when the state is written, so the row kernel only reads them), NCOMP and,
//          one byte per node, GEN (passes through the node) and COMP (constraints completed at it) of the unordered representation.
// States live in a ping-pong pair [2][bsz * beam][LEX_SW] indexed by the step's parity like tokens / scores.
constexpr int LEX_TOK_MAX = 32, LEX_NODES = LEX_TOK_MAX + 1, LEX_NEXT_MAX = 16, LEX_WIDTH_MAX = 1 + 2 * LEX_TOK_MAX;
constexpr int LEX_TBL_W = 4 + 4 * LEX_NODES, LEX_SW = 44;
constexpr int LEX_A = 4, LEX_B = LEX_A + LEX_NODES, LEX_C = LEX_B + LEX_NODES, LEX_D = LEX_C + LEX_NODES;
constexpr int LS_NODE = 0, LS_BANK = 1, LS_FIN = 2, LS_NNEXT = 3, LS_NCOMP = 4, LS_NEXT = 8, LS_GEN = 24, LS_COMP = 33;
static_assert(LS_NEXT + LEX_NEXT_MAX <= LS_GEN && LS_GEN * 4 + LEX_NODES <= LS_COMP * 4 && LS_COMP * 4 + LEX_NODES <= LEX_SW * 4, "state layout");
constexpr int LEX_L_MAX = KMAX_ALL + BEAM_MAX + BEAM_MAX * LEX_NEXT_MAX;  // the candidate list of one sentence
struct LexP {
  const int32_t* tbl;   // [bsz][LEX_TBL_W]
  int32_t* state;       // [2][bsz * beam][LEX_SW]; nullptr: no lexical constraints (the CON row kernels without them)
  float* nval;          // [bsz * beam][LEX_NEXT_MAX]: the row kernel's values of the row's next tokens
  int32_t* ntok;        // [bsz * beam][LEX_NEXT_MAX]
};
struct NoLex {};  // like NoEns
template <bool LEX> using LexArg = std::conditional_t<LEX, LexP, NoLex>;

// the node below `node` that token t leads to (unordered; 0 = none: the root is nobody's child)
__device__ __forceinline__ int lex_child(const int32_t* tbl, int node, int t) {
  int c = 0;
  for (int q = 1; q < tbl[1]; ++q) c = (tbl[LEX_B + q] == node && tbl[LEX_A + q] == t) ? q : c;
  return c;
}
// The bank of advance(st, t) (token_generation_constraints.py OrderedConstraintState.advance :463-506, UnorderedConstraintState.advance
// :298-358).  out != nullptr: a copy of st that becomes the advanced state (NODE, BANK, NCOMP, GEN, COMP; lex_derive does the rest).
// Ordered: finished -> stay; the next token -> on; at the end of a constraint -> stay (the ROOT reads the reference's endpoints[-1], the
// last entry, always true: a token that does not start the constraints keeps the root); the first token of all -> state 0; else the root.
// Unordered: the node's child by t if that edge is open (GEN < num_constraints of the child), else back to the root — onto the root's
// child by t if open — and the path left behind is settled from the old node upwards: the first node with an unfinished terminal gets
// one more COMP and the walk ends, every node before it loses one GEN.  All tests read the OLD state.
__device__ __forceinline__ int lex_advance(const int32_t* tbl, const int32_t* st, int t, int32_t* out) {
  const int n = tbl[1];
  if (tbl[2] == 1) {
    const int idx = st[LS_NODE];
    int ni;
    if (idx + 1 >= n) ni = idx;
    else if (tbl[LEX_A + idx + 1] == t) ni = idx + 1;
    else if (idx < 0 || tbl[LEX_B + idx] != 0) ni = idx;
    else if (t == tbl[LEX_A]) ni = 0;
    else ni = -1;
    if (out) { out[LS_NODE] = ni; out[LS_BANK] = ni + 1; }
    return ni + 1;
  }
  const uint8_t* gen = reinterpret_cast<const uint8_t*>(st + LS_GEN);
  const uint8_t* comp = reinterpret_cast<const uint8_t*>(st + LS_COMP);
  uint8_t* ogen = out ? reinterpret_cast<uint8_t*>(out + LS_GEN) : nullptr;
  uint8_t* ocomp = out ? reinterpret_cast<uint8_t*>(out + LS_COMP) : nullptr;
  const int node = st[LS_NODE];
  int bank = st[LS_BANK];
  int c = lex_child(tbl, node, t);
  bool rewind = false;
  if (!(c != 0 && (int)gen[c] < tbl[LEX_D + c])) {
    c = lex_child(tbl, 0, t);
    if (!(c != 0 && (int)gen[c] < tbl[LEX_D + c])) c = 0;
    rewind = true;
  }
  if (c != 0) {
    ++bank;
    if (out) ogen[c] = (uint8_t)(gen[c] + 1);
  }
  if (out) out[LS_NODE] = c;
  if (rewind) {
    int q = node;
    for (int hop = 0; hop < LEX_NODES && q > 0 && q < n; ++hop) {
      if (tbl[LEX_C + q] != 0 && (int)comp[q] < tbl[LEX_C + q]) {
        if (out) { ocomp[q] = (uint8_t)(comp[q] + 1); out[LS_NCOMP] = st[LS_NCOMP] + 1; }
        break;
      }
      --bank;
      if (out) ogen[q] = (uint8_t)(ogen[q] - 1);  // (ogen, not gen: q may be the node just entered)
      q = tbl[LEX_B + q];
    }
  }
  if (out) out[LS_BANK] = bank;
  return bank;
}
// FIN, NNEXT and NEXT of a state whose other words are final (finished / next_tokens of the two state classes :271-296, :434-461).
// Ordered: the first token of all once the state is PAST it (state > 0), and the token that advances.  Unordered: the root's children
// and the node's.  Ascending, distinct, at most LEX_NEXT_MAX (the caller's host check keeps real lists below that).
__device__ __forceinline__ void lex_derive(const int32_t* tbl, int32_t* st) {
  const int n = tbl[1], node = st[LS_NODE];
  int cnt = 0;
  auto add = [&](int t) {
    int pos = 0;
    while (pos < cnt && st[LS_NEXT + pos] < t) ++pos;
    if ((pos < cnt && st[LS_NEXT + pos] == t) || cnt == LEX_NEXT_MAX) return;
    for (int q = cnt; q > pos; --q) st[LS_NEXT + q] = st[LS_NEXT + q - 1];
    st[LS_NEXT + pos] = t;
    ++cnt;
  };
  if (tbl[2] == 1) {
    const bool fin = node + 1 >= n;
    st[LS_FIN] = fin ? 1 : 0;
    if (node > 0) add(tbl[LEX_A]);
    if (!fin) add(tbl[LEX_A + node + 1]);
  } else {
    const uint8_t* comp = reinterpret_cast<const uint8_t*>(st + LS_COMP);
    const int pending = (node > 0 && tbl[LEX_C + node] != 0 && (int)comp[node] < tbl[LEX_C + node]) ? 1 : 0;
    st[LS_FIN] = (tbl[LEX_D] - (st[LS_NCOMP] + pending) == 0) ? 1 : 0;
    for (int q = 1; q < n; ++q)
      if (tbl[LEX_B + q] == 0 || tbl[LEX_B + q] == node) add(tbl[LEX_A + q]);
  }
  st[LS_NNEXT] = cnt;
}

// cst_lex_init: one workgroup per sentence turns its packed row [count, tokens of c0, 0, tokens of c1, 0, ...] into the table and sets
// every row's state to the root in both halves of the ping-pong pair.  Tokens beyond LEX_TOK_MAX are not read (the host refuses them).
__global__ __launch_bounds__(64) void lex_init_kernel(const int64_t* packed, int width, int rep, int beam, int bbsz, int32_t* tbl_out, int32_t* state) {
  const int sent = blockIdx.x, tid = threadIdx.x;
  __shared__ int row[LEX_WIDTH_MAX];
  __shared__ int32_t tbl[LEX_TBL_W], st[LEX_SW];
  for (int i = tid; i < LEX_WIDTH_MAX; i += blockDim.x) row[i] = i < width ? (int)packed[(int64_t)sent * width + i] : 0;
  for (int i = tid; i < LEX_TBL_W; i += blockDim.x) tbl[i] = 0;
  for (int i = tid; i < LEX_SW; i += blockDim.x) st[i] = 0;
  __syncthreads();
  if (tid == 0) {
    const int W = width < LEX_WIDTH_MAX ? width : LEX_WIDTH_MAX;
    int count = row[0] < 0 ? 0 : (row[0] > LEX_TOK_MAX ? LEX_TOK_MAX : row[0]);
    int at = 1, n = rep == 1 ? 0 : 1, ntok = 0;
    for (int c = 0; c < count && at < W; ++c) {
      int node = 0, len = 0;
      for (; at < W && row[at] != 0 && ntok < LEX_TOK_MAX; ++at, ++ntok, ++len) {
        const int t = row[at];
        if (rep == 1) {
          tbl[LEX_A + n] = t;
          tbl[LEX_B + n] = 0;
          ++n;
        } else {
          tbl[1] = n;  // (lex_child scans the nodes made so far)
          int ch = lex_child(tbl, node, t);
          if (ch == 0) {
            ch = n++;
            tbl[LEX_A + ch] = t;
            tbl[LEX_B + ch] = node;
          }
          node = ch;
        }
      }
      if (len > 0) {
        if (rep == 1) tbl[LEX_B + n - 1] = 1;
        else {
          tbl[LEX_C + node] += 1;
          for (int q = node, hop = 0; hop < LEX_NODES; ++hop) {
            tbl[LEX_D + q] += 1;
            if (q == 0) break;
            q = tbl[LEX_B + q];
          }
        }
      }
      while (at < W && row[at] != 0) ++at;  // (the unread tail of a constraint past the limit)
      ++at;
    }
    tbl[1] = n;
    tbl[2] = rep;
    int nd = 0;
    for (int i = rep == 1 ? 0 : 1; i < n; ++i) {
      bool seen = false;
      for (int j = rep == 1 ? 0 : 1; j < i; ++j) seen = seen || tbl[LEX_A + j] == tbl[LEX_A + i];
      nd += seen ? 0 : 1;
    }
    tbl[0] = nd;
    st[LS_NODE] = rep == 1 ? -1 : 0;
    lex_derive(tbl, st);
  }
  __syncthreads();
  for (int i = tid; i < LEX_TBL_W; i += blockDim.x) tbl_out[(int64_t)sent * LEX_TBL_W + i] = tbl[i];
  for (int i = tid; i < 2 * beam * LEX_SW; i += blockDim.x) {
    const int half = i / (beam * LEX_SW), r = i % (beam * LEX_SW);
    state[((int64_t)half * bbsz + (int64_t)sent * beam) * LEX_SW + r] = st[r % LEX_SW];
  }
}

// member n's copy of logits row hs (without ENS: the row itself)
template <typename T, bool ENS>
__device__ __forceinline__ const T* member_row(const BeamP& p, const EnsArg<ENS>& e, int n, int hs) {
  const void* base = p.logits;
  if constexpr (ENS) base = e.logits[n];
  return reinterpret_cast<const T*>(base) + (int64_t)hs * p.ld_logits;
}
// logit / T.  The plain step multiplies by 1 / T, the ensemble step divides by T: the two round differently and tests pin both.
template <bool ENS>
__device__ __forceinline__ float temper(float x, const BeamP& p, const EnsArg<ENS>& e) {
  if constexpr (ENS) return x / e.temperature;
  else return x * p.inv_temperature;
}

// (max, sum exp(x - max)) of two partial softmax statistics
__device__ __forceinline__ void lse_merge(float& mx, float& sum, float m2, float s2) {
  const float M = fmaxf(mx, m2);
  sum = (mx == -INFINITY ? 0.0f : sum * expf(mx - M)) + (m2 == -INFINITY ? 0.0f : s2 * expf(m2 - M));
  mx = M;
}
// lse_merge(mx, sum, x, 1.0f) of one element with ONE expf.  An x of -inf adds nothing and is skipped: while mx is still -inf,
// expf(x - mx) would be expf(NaN).
__device__ __forceinline__ void lse_push(float& mx, float& sum, float x) {
  if (x > mx) { sum = (mx == -INFINITY ? 0.0f : sum * expf(mx - x)) + 1.0f; mx = x; }
  else if (x != -INFINITY) sum += expf(x - mx);
}
// a thread's statistics of the values it holds in registers: the maximum first, then one expf per element.  NaN anywhere: sum NaN ->
// lse NaN -> every candidate of the row becomes -inf (the first mask of mask_lprob)
template <int NV, int VEC>
__device__ __forceinline__ void lse_thread(const float (&x)[NV][VEC], float& mx, float& sum) {
  mx = -INFINITY;
  sum = 0.0f;
  bool nan = false;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < VEC; ++k) { nan = nan || x[i][k] != x[i][k]; mx = fmaxf(mx, x[i][k]); }
  if (mx != -INFINITY) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < VEC; ++k) sum += expf(x[i][k] - mx);
  }
  if (nan) sum = NAN;
}
// The block's log-sum-exp of nmem rows (the members' rows; 1 without ENS).  thread_stats(n, mx, sum) yields this thread's share of row n;
// the lanes of a wave merge theirs by shuffles, lane 0 leaves the wave's pair in LDS, and after ONE barrier for all rows thread n merges
// the waves' pairs of row n in wave order -> st.lse[n], valid for every thread on return.
template <int NMAX, int NW>
struct LseSm {
  float m[NMAX][NW], s[NMAX][NW], lse[NMAX];
};
template <int NMAX, int NW, typename F>
__device__ __forceinline__ void block_lse(int nmem, LseSm<NMAX, NW>& st, F&& thread_stats) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int n = 0; n < nmem; ++n) {
    float mx, sum;
    thread_stats(n, mx, sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(mx, sum, __shfl_xor(mx, o, 64), __shfl_xor(sum, o, 64));
    if (lane == 0) { st.m[n][wave] = mx; st.s[n][wave] = sum; }
  }
  __syncthreads();
  if (tid < nmem) {
    float mm = -INFINITY, ss = 0.0f;
    for (int w = 0; w < NW; ++w) lse_merge(mm, ss, st.m[tid][w], st.s[tid][w]);
    st.lse[tid] = mm + logf(ss);
  }
  __syncthreads();
}
// a member without a finite lse (NaN or +-inf): its log-softmax is NaN, and so is the ensemble's row
__device__ __forceinline__ bool ens_bad(const float* lse, int n) {
  bool bad = false;
  for (int i = 0; i < n; ++i) bad = bad || !(lse[i] - lse[i] == 0.0f);
  return bad;
}
// lp of an element from its running (max m, sum a) over the members' a_n (the small term first: one rounding at the magnitude of lp)
__device__ __forceinline__ float ens_lprob(float m, float a, bool bad, float log_n) {
  return bad ? NAN : (m == -INFINITY ? -INFINITY : m + (logf(a) - log_n));
}

// CON (the constraints of --prefix-size / --no-repeat-ngram-size, compiled in only where one of them is on):
//   prefix (_prefix_tokens :543-575; the masks themselves are in mask_lprob): at steps s < prefix_len, s < max_len every candidate of the
//   sentence's rows but token t = prefix_tokens[sentence][s] becomes -inf (t == pad: unconstrained); the min-len mask is suspended for
//   the WHOLE batch at those steps (the reference's `elif`); t == eos: the reference copies tokens, scores and log-probabilities of
//   the sentence's first beam to all its beams — here every row of that sentence READS the first row (logits, cumulative score,
//   tokens) and beam_merge_kernel takes the first row as the parent.
// step s forces prefix tokens (for the sentences whose entry is not pad) and suspends the min-len mask
__device__ __forceinline__ bool prefix_step(const BeamP& p, int s) { return s < p.prefix_len && s < p.max_len; }

struct RowCtx {
  int s, h, r;  // the step, the row, the row's number within its sentence
  int hs;       // the row whose logits, score and tokens this row reads (the sentence's first row where the prefix holds eos)
  int pt;       // the forced token (-1: none)
  bool pfx;     // a prefix step (no min-len mask)
};
// false: the row has nothing to do at this step
template <bool CON>
__device__ __forceinline__ bool row_prologue(const BeamP& p, RowCtx& c) {
  c.s = *p.step;
  if (c.s > p.max_len) return false;
  c.h = blockIdx.x;
  c.r = c.h % p.beam;
  if (c.s == 0 && c.r != 0) return false;  // all hypotheses are equal at step 0: only the first beam competes (search.py:121-124)
  c.hs = c.h;
  c.pt = -1;
  c.pfx = false;
  if constexpr (CON) {
    c.pfx = prefix_step(p, c.s);
    if (c.pfx) {
      const int64_t t = p.prefix_tokens[(int64_t)(c.h / p.beam) * p.prefix_len + c.s];
      if (t != p.pad) c.pt = (int)t;
      if (t == p.eos) c.hs = c.h - c.r;
    }
  }
  return true;
}
// the tokens tk[0 .. s] of the row that c reads, and its cumulative score (search.py:125)
__device__ __forceinline__ const int64_t* row_tokens(const BeamP& p, const RowCtx& c) {
  return p.tokens + ((int64_t)(c.s & 1) * p.bsz * p.beam + c.hs) * (p.max_len + 2);
}
__device__ __forceinline__ float row_prev_score(const BeamP& p, const RowCtx& c) {
  const int L1 = p.max_len + 1;
  return c.s > 0 ? (p.scores + (int64_t)(c.s & 1) * p.bsz * p.beam * L1)[(int64_t)c.hs * L1 + c.s - 1] : 0.0f;
}

// the row's lexical-constraint state at this step (nullptr without LEX: the kernels without CON, or a null state pointer)
template <bool CON>
__device__ __forceinline__ const int32_t* lex_row_state(const BeamP& p, const LexArg<CON>& lx, const RowCtx& c) {
  if constexpr (CON) {
    if (lx.state != nullptr) return lx.state + ((int64_t)(c.s & 1) * p.bsz * p.beam + c.h) * LEX_SW;
  }
  return nullptr;
}

// n-gram blocking (_no_repeat_ngram :734-767): with last = tk[s+2-n .. s], every i in [0, s+1-n] with tk[i .. i+n-2] == last bans token
// tk[i+n-1].  (The reference also scans the pad tail of its buffer; for n >= 2 that only ever bans pad, which is -inf already.)
// Calls ban(token) for every such token; tk = the row's tokens tk[0 .. s].  The workgroup's threads test the positions i in parallel
// and set the banned tokens' bits in an LDS bitmap.  beam_row_regs holds an exact bitmap and reads one word per 16-byte vector where the
// candidate values are formed; beam_row_wide, whose vocabulary has no bound, holds a FILTER of BANW * 32 bits indexed by the token's low
// bits and confirms a set bit against the row's tokens — banned tokens are few, so almost every element costs the one LDS read.
template <typename F>
__device__ __forceinline__ void ngram_banned(const int64_t* tk, int s, int n, int tid, int nth, F&& ban) {
  const int first = s + 2 - n;  // last = tk[first .. s], n - 1 tokens
  if (n < 2 || first < 0) return;
  for (int i = tid; i <= s + 1 - n; i += nth) {
    bool eq = true;
    for (int k = 0; k < n - 1; ++k) eq = eq && tk[i + k] == tk[first + k];
    if (eq) ban(tk[i + n - 1]);
  }
}

// (b): the masks of sequence_generator.py on the log-probability lp of token v, in the generator's order.  banned(value so far) says
// whether the n-gram ban takes the token (CON only; the wide body's test is costly, so it looks at the value first).  The cumulative
// score is added by the caller: a draw (SAMP) wants the value without it.
template <bool CON, typename B>
__device__ __forceinline__ float mask_lprob(const BeamP& p, const RowCtx& c, int v, float lp, B&& banned) {
  const float NEG = -INFINITY;
  float val = lp;
  if (val != val) val = NEG;                               // lprobs[lprobs != lprobs] = -inf        (:311)
  if (v == p.pad) val = NEG;                               // never select pad                        (:313)
  if (v == p.unk) val -= p.unk_penalty;                    //                                         (:314)
  if (c.s >= p.max_len && v != p.eos) val = NEG;           // force eos at max length                 (:317-319)
  if constexpr (CON) {
    if (c.pt >= 0 && v != c.pt) val = NEG;                 // forced prefix token                     (:336-344, :543-553)
    if (!c.pfx && c.s < p.min_len && v == p.eos) val = NEG;  // (`elif`: not at a prefix step)       (:345-347)
    if (banned(val)) val = NEG;                            // the token would repeat an n-gram        (:368-369)
  } else {
    if (c.s < p.min_len && v == p.eos) val = NEG;          // minimum length constraint               (:329-331)
  }
  return val;
}

// arg-max of (cv, ci) in the candidate order over groups of 2 * O lanes (xor tree: every lane of a group ends with the group's best).
// Selects, not branches: it sits in the register body's selection loop (see the rescan there for what exec-mask branches cost).
template <int O>
__device__ __forceinline__ void wave_argmax(float& cv, int& ci) {
#pragma unroll
  for (int o = O; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(cv, o, 64);
    const int i2 = __shfl_xor(ci, o, 64);
    const bool b = (v2 > cv) | ((v2 == cv) & (i2 < ci));
    cv = b ? v2 : cv;
    ci = b ? i2 : ci;
  }
}

// ---- sampling (search.py Sampling.step :676-742): stage (c) of the row kernel when cst_beam_desc.sampling is set -------------------
// In: x = the row's masked log-probabilities in registers (NaN = not a candidate), BEFORE the cumulative score is added.  With
// q_v = exp(x_v) (not renormalised after the masks, like the reference's multinomial input):
//   cut   top-p (p > 0, wins): in the total order (value desc, token asc — cand_better) element j is kept iff the mass in front of it is
//         < p (_sample_topp :630-673: cumsum.lt(p) plus one more element; whole mass < p: everything).  Found WITHOUT sorting: values map
//         to order-preserving 32-bit keys, and 32 block-wide sums S(c) = sum of q over {key >= c} build, bit by bit, the largest c with
//         S(c) >= p — the key of the last kept value.  Elements that share that key are kept in token order while the mass in front of
//         them stays < p: the number m of them follows from S(> key) and their common q, and where m is less than their number a second
//         bisection (15 block-wide counts, over the token id) finds the m-th of them.
//         top-k (k > 0): the same bisection over COUNTS: the largest c with #{key >= c} >= k; ties at the k-th value in token order.
//   draw  u = (cst_drop_bits32(key, cst_drop_key2(key), idx) >> 8) * 2^-24, idx = (sentence * beam + slot) * (max_len + 1) + step, key read
//         from device memory; the token is the smallest kept v whose inclusive kept mass in VOCABULARY order exceeds u * Z (Z = kept
//         mass).  Vocabulary order is (vector i, thread, element): per i a wave-wide inclusive scan of the threads' sums by shuffles, the
//         wave totals through LDS, added by every thread in the fixed order (i, wave); each thread then walks its own elements.  The
//         block-wide minimum over the threads' first hits is the draw; if rounding lets no element exceed u * Z (u * Z within an ulp of
//         Z), the last kept element with q > 0 is taken.  A step-0 row draws `beam` tokens (slots 0 .. beam-1, with replacement), any
//         other row one (its own slot).  Output: (x_v + cumulative score, v) at cand[sentence * beam + slot]; a row without mass
//         writes (-inf, pad) — what the selection kernel writes for a missing candidate.
// Every sum has a fixed order (no floating-point atomics): thread-serial over (i, element), a shuffle tree, then the waves in wave
// order.  LONGEST ADDITION CHAIN of a sum that decides the cut or the draw: 64 (NV * VEC = 40 in a thread + 6 shuffle levels + 8 waves
// for the masses; 7 + 6 for a wave total, NV * 8 = 40 wave totals, + 1 + 8 inside the thread for an inclusive kept mass).
__device__ __forceinline__ uint32_t samp_key(float v) {  // order-preserving: larger value <-> larger key; NaN (not a candidate) -> 0
  const uint32_t b = __float_as_uint(v + 0.0f);           // (-0 -> +0)
  return v != v ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ __forceinline__ float samp_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int NV, int VEC>
__device__ __forceinline__ void beam_row_sample_tail(const BeamP& p, float (&x)[NV][VEC], int s, int h, float prev, float* cand_val,
                                                     int32_t* cand_tok) {
  constexpr int NTH = 512, NW = NTH / 64;
  static_assert(NV * NTH * VEC <= 32768, "the tie bisection walks 15 bits of the token id");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ float sm_f[2][NW];
  __shared__ int sm_i[2][NW];
  __shared__ float sm_tot[NV][NW];
  __shared__ int sm_pick[BEAM_MAX][NW], sm_last[NW];
  int par = 0;
  // block-wide sums whose result is the same bit pattern in every thread (one barrier each: the two LDS rows alternate)
  auto block_sum_f = [&](float v) -> float {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sm_f[par][wave] = v;
    __syncthreads();
    float t = sm_f[par][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += sm_f[par][w];
    par ^= 1;
    return t;
  };
  auto block_sum_i = [&](int v) -> int {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sm_i[par][wave] = v;
    __syncthreads();
    int t = sm_i[par][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += sm_i[par][w];
    par ^= 1;
    return t;
  };
  float q[NV][VEC];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[i][e] = x[i][e] == x[i][e] ? expf(x[i][e]) : 0.0f;
  const bool topp = p.sample_topp > 0.0f, topk = !topp && p.sample_topk > 0;
  if (topp || topk) {
    const float pp = p.sample_topp;
    const int kk = p.sample_topk;
    uint32_t F = 0u;  // the largest c with S(c) >= p / #(c) >= k: the key of the last kept value (0: everything is kept)
    for (int b = 31; b >= 0; --b) {
      const uint32_t c = F | (1u << b);
      bool ge;
      if (topp) {
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
          for (int e = 0; e < VEC; ++e) part += samp_key(x[i][e]) >= c ? q[i][e] : 0.0f;
        ge = block_sum_f(part) >= pp;
      } else {
        int part = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
          for (int e = 0; e < VEC; ++e) part += samp_key(x[i][e]) >= c ? 1 : 0;
        ge = block_sum_i(part) >= kk;
      }
      if (ge) F = c;
    }
    // the elements that share the key F: n_tie of them, the first m in token order are kept
    int tie_part = 0, gt_cnt = 0;
    float gt_part = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const uint32_t k = samp_key(x[i][e]);
        tie_part += k == F ? 1 : 0;
        gt_cnt += k > F ? 1 : 0;
        gt_part += k > F ? q[i][e] : 0.0f;
      }
    const int n_tie = block_sum_i(tie_part);
    int m = n_tie;
    if (F != 0u) {
      if (topp) {
#pragma clang fp contract(off)
        const float s_gt = block_sum_f(gt_part), qs = expf(samp_unkey(F));  // (the same expf of the same value as the elements' own q)
        if (qs > 0.0f && n_tie > 1) {
          // the smallest j with s_gt + j * qs >= p: ties 0 .. j-1 have less than p in front of them
          float jf = ceilf((pp - s_gt) / qs);
          jf = fminf(fmaxf(jf, 1.0f), (float)n_tie);
          int j = (int)jf;
          while (j > 1 && s_gt + (float)(j - 1) * qs >= pp) --j;
          while (j < n_tie && s_gt + (float)j * qs < pp) ++j;
          m = j < n_tie ? j : n_tie;
        }
      } else {
        m = kk - block_sum_i(gt_cnt);
        m = m < n_tie ? m : n_tie;
      }
    }
    int cut = INT_MAX;  // ties are kept up to this token id
    if (m < n_tie) {    // (block-uniform) the m-th tie in token order: the largest c with #{ties with token < c} < m
      cut = 0;
      for (int b = 14; b >= 0; --b) {
        const int c = cut | (1 << b);
        int part = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
          for (int e = 0; e < VEC; ++e) part += (samp_key(x[i][e]) == F && (tid + i * NTH) * VEC + e < c) ? 1 : 0;
        if (block_sum_i(part) < m) cut = c;
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const uint32_t k = samp_key(x[i][e]);
        const bool kept = k > F || (k == F && (tid + i * NTH) * VEC + e <= cut);
        q[i][e] = kept ? q[i][e] : 0.0f;
      }
  }
  // inclusive kept mass in vocabulary order
  float base[NV], exc[NV];
  int last = -1;  // this thread's last element with kept mass
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float t = q[i][0];
#pragma unroll
    for (int e = 1; e < VEC; ++e) t += q[i][e];
#pragma unroll
    for (int e = 0; e < VEC; ++e) last = q[i][e] > 0.0f ? (tid + i * NTH) * VEC + e : last;
    float inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float n = __shfl_up(inc, o, 64);
      if (lane >= o) inc += n;
    }
    const float up = __shfl_up(inc, 1, 64);
    exc[i] = lane == 0 ? 0.0f : up;
    if (lane == 63) sm_tot[i][wave] = inc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int l2 = __shfl_xor(last, o, 64); last = l2 > last ? l2 : last; }
  if (lane == 0) sm_last[wave] = last;
  __syncthreads();
  float run = 0.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w == wave) base[i] = run;
      run += sm_tot[i][w];
    }
  const float Z = run;
  const int nd = s == 0 ? p.beam : 1;
  const uint32_t key = *p.sample_key, key2 = cst_drop_key2(key);
  const int L1 = p.max_len + 1;
  for (int d = 0; d < nd; ++d) {
    const float u = (float)(cst_drop_bits32(key, key2, (uint32_t)((h + d) * L1 + s)) >> 8) * 5.9604644775390625e-8f;
    const float target = u * Z;
    int pick = INT_MAX;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float c = base[i] + exc[i];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        c += q[i][e];
        const bool hit = (q[i][e] > 0.0f) & (c > target) & (pick == INT_MAX);
        pick = hit ? (tid + i * NTH) * VEC + e : pick;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int p2 = __shfl_xor(pick, o, 64); pick = p2 < pick ? p2 : pick; }
    if (lane == 0) sm_pick[d][wave] = pick;
  }
  __syncthreads();
  int fall = sm_last[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) fall = sm_last[w] > fall ? sm_last[w] : fall;
  for (int d = 0; d < nd; ++d) {
    int tok = sm_pick[d][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) tok = sm_pick[d][w] < tok ? sm_pick[d][w] : tok;
    if (tok == INT_MAX) tok = fall;
    if (!(Z > 0.0f) || tok < 0) {  // no mass: a missing candidate
      if (tid == 0) { cand_val[h + d] = -INFINITY; cand_tok[h + d] = p.pad; }
      continue;
    }
    // the thread that holds the token writes it
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if ((tid + i * NTH) * VEC + e == tok) {
          cand_val[h + d] = s > 0 ? x[i][e] + prev : x[i][e];
          cand_tok[h + d] = tok;
        }
  }
}

// The register-resident body: the row's logits stay in registers (NV 16-byte vectors per thread) between the statistics pass and
// stage (c); the selection is 2*beam wave-wide arg-max rounds in which only the winning thread rescans its registers (an earlier
// version kept a sorted top-K list per thread for a whole sentence per workgroup: the divergent insertion chains made it 105 us per step).
template <typename T, int NV, bool ENS, bool CON, bool SAMP, bool LM>
__device__ __forceinline__ void beam_row_regs(const BeamP& p, const EnsArg<ENS>& e, const LmArg<LM>& lm, const LexArg<CON>& lx, float* cand_val,
                                              int32_t* cand_tok) {
  constexpr int VEC = DT<T>::VEC, NTH = 512, NW = NTH / 64;
  RowCtx c;
  if (!row_prologue<CON>(p, c)) return;
  const int s = c.s, h = c.h, hs = c.hs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = p.vocab, K = 2 * p.beam;
  const int nvec = (V + VEC - 1) / VEC;
  const float NEG = -INFINITY;
  __shared__ uint32_t ban[CON ? NV * NTH * VEC / 32 : 1];  // the bitmap of n-gram-banned tokens
  if constexpr (CON) {
#pragma unroll
    for (int i = 0; i < NV * VEC / 32 + 1; ++i)
      if (tid + i * NTH < NV * NTH * VEC / 32) ban[tid + i * NTH] = 0u;
    __syncthreads();
    ngram_banned(row_tokens(p, c), s, p.ngram, tid, NTH, [&](int64_t v) {
      if (v >= 0 && v < V) atomicOr(&ban[v >> 5], 1u << (v & 31));
    });  // (visible after the barriers of the statistics pass below)
  }
  __shared__ LseSm<(ENS ? ENS_MAX : 1) + (LM ? 1 : 0), NW> st;
  __shared__ float w_val[NW * KMAX_ALL];
  __shared__ int w_tok[NW * KMAX_ALL];
  static_assert(KMAX_ALL <= 64 && NW <= 64, "the merge keeps one output candidate / one list head per lane of wave 0");

  float x[NV][VEC];
  auto load_row = [&](int n, float (&t)[NV][VEC]) {  // member n's row / T; -inf behind the vocabulary
    const T* ln = member_row<T, ENS>(p, e, n, hs);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = tid + i * NTH;
      if (vi < nvec) ld_vec<T>(ln + (int64_t)vi * VEC, t[i]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) t[i][k] = (vi < nvec && vi * VEC + k < V) ? temper<ENS>(t[i][k], p, e) : NEG;
    }
  };
  [[maybe_unused]] auto load_lm_row = [&](float (&t)[NV][VEC]) {  // the LM's row, untempered; -inf behind the vocabulary
    if constexpr (LM) {
      const T* ln = reinterpret_cast<const T*>(lm.logits) + (int64_t)hs * p.ld_logits;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int vi = tid + i * NTH;
        if (vi < nvec) ld_vec<T>(ln + (int64_t)vi * VEC, t[i]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[i][k] = (vi < nvec && vi * VEC + k < V) ? t[i][k] : NEG;
      }
    }
  };
  int nmod = 1;  // the model's rows; the LM's statistics take slot nmod
  if constexpr (ENS) nmod = e.n;
  float lse = 0.0f;
  if constexpr (ENS) {
    float t[NV][VEC];
    block_lse(nmod + (LM ? 1 : 0), st, [&](int n, float& mx, float& sum) {
      if (LM && n == nmod) load_lm_row(t);
      else load_row(n, t);
      lse_thread(t, mx, sum);
    });
    const bool bad = ens_bad(st.lse, e.n);
    float acc[NV][VEC];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < VEC; ++k) { x[i][k] = NEG; acc[i][k] = 0.0f; }
    for (int n = 0; n < e.n; ++n) {
      load_row(n, t);
      const float ln = st.lse[n];
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int k = 0; k < VEC; ++k) lse_merge(x[i][k], acc[i][k], t[i][k] - ln, 1.0f);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) x[i][k] = ens_lprob(x[i][k], acc[i][k], bad, e.log_n);
      const int vi = tid + i * NTH;
      if (e.lprobs_out && vi < nvec) {
        float* o = e.lprobs_out + (int64_t)h * p.ld_logits + (int64_t)vi * VEC;
#pragma unroll
        for (int k = 0; k < VEC; k += 4) { f32x4 o4 = {x[i][k], x[i][k + 1], x[i][k + 2], x[i][k + 3]}; *reinterpret_cast<f32x4*>(o + k) = o4; }
      }
    }  // x holds log-probabilities already: lse stays 0
  } else if constexpr (LM) {
    float t[NV][VEC];
    block_lse(2, st, [&](int n, float& mx, float& sum) {
      if (n == 0) { load_row(0, x); lse_thread(x, mx, sum); }
      else { load_lm_row(t); lse_thread(t, mx, sum); }
    });
    lse = st.lse[0];
  } else {
    block_lse(1, st, [&](int, float& mx, float& sum) { load_row(0, x); lse_thread(x, mx, sum); });
    lse = st.lse[0];
  }
  if constexpr (LM) {  // x <- lp' (second sweep over the LM row); lse is spent
    float t[NV][VEC];
    load_lm_row(t);
    const float lse_lm = st.lse[nmod];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) x[i][k] = lm_fuse(x[i][k] - lse, lm.weight, t[i][k], lse_lm);
      const int vi = tid + i * NTH;
      if (lm.lprobs_out && vi < nvec) {
        float* o = lm.lprobs_out + (int64_t)h * p.ld_logits + (int64_t)vi * VEC;
#pragma unroll
        for (int k = 0; k < VEC; k += 4) { f32x4 o4 = {x[i][k], x[i][k + 1], x[i][k + 2], x[i][k + 3]}; *reinterpret_cast<f32x4*>(o + k) = o4; }
      }
    }
    lse = 0.0f;
  }
  const float prev = row_prev_score(p, c);
  const int32_t* lex_st = lex_row_state<CON>(p, lx, c);  // the row's constraint state (nullptr: no lexical constraints)
  const bool lex_no_eos = lex_st != nullptr && s > 0 && lex_st[LS_FIN] == 0;
  // candidate values replace the logits in the registers
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = tid + i * NTH;
    uint32_t bw = 0u;  // the vector's VEC tokens share one word of the bitmap
    if constexpr (CON) bw = ban[(vi * VEC) >> 5];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int v = vi * VEC + k;
      float val = mask_lprob<CON>(p, c, v, x[i][k] - lse, [&](float) { return ((bw >> (v & 31)) & 1u) != 0u; });
      if (lex_no_eos && v == p.eos) val = NEG;             // eos only once the constraints are met      (search.py:308-321)
      if constexpr (!SAMP) {
        if (s > 0) val += prev;                          // search.py:125
      }
      x[i][k] = (vi < nvec && v < V) ? val : NAN;        // NaN = not a candidate (never compares better)
    }
  }
  if constexpr (SAMP) {  // x holds the masked log-probabilities WITHOUT the cumulative score: (c) is a draw, not a selection
    beam_row_sample_tail<NV, VEC>(p, x, s, h, prev, cand_val, cand_tok);
    return;
  }
  if constexpr (CON) {  // the values of the state's next tokens (search.py:398-410): the thread that holds the token writes it
    if (lex_st != nullptr) {
      const int nn = lex_st[LS_NNEXT] < LEX_NEXT_MAX ? lex_st[LS_NNEXT] : LEX_NEXT_MAX;
      for (int j = 0; j < nn; ++j) {
        const int t = lex_st[LS_NEXT + j];
        const bool inside = t >= 0 && t < V;
        const int vi = inside ? t / VEC : 0;
        if (tid != (inside ? vi % NTH : 0)) continue;
        float val = NEG;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
          for (int k = 0; k < VEC; ++k) val = (inside && i == vi / NTH && k == t % VEC) ? x[i][k] : val;
        lx.nval[(int64_t)h * LEX_NEXT_MAX + j] = val;
        lx.ntok[(int64_t)h * LEX_NEXT_MAX + j] = t;
      }
    }
  }
  // local best that is strictly worse than (tv, ti) — the thread's previously taken candidate
  float tv = INFINITY, bv;
  int ti = -1, bi;
  auto rescan = [&]() {
    bv = NEG; bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = tid + i * NTH;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        // (bitwise, not short-circuit: the && / || form compiled to ~5 exec-mask branches per element — 121 in the kernel, 3 us per scan)
        const float val = x[i][k];
        const int v = vi * VEC + k;
        const bool open = (val < tv) | ((val == tv) & (v > ti));          // NaN (not a candidate) compares false both ways
        const bool take = open & ((val > bv) | ((val == bv) & (v < bi)));
        bv = take ? val : bv;
        bi = take ? v : bi;
      }
    }
  };
  // Selection in two levels, ONE barrier (round 5; the block-wide arg-max per candidate it replaces cost two barriers and an LDS
  // round trip for each of the 2*beam candidates: 37 us per step): every wave first extracts ITS top-K in order — K rounds of a
  // wave-wide arg-max by shuffles, the winning lane rescans its registers — then wave 0 merges the NW sorted lists, lane w holding
  // the head of wave w's list.  The order is total (value, then token), so the result is the block-wide selection's.
  // the thread's best AND second best in one pass: a lane that wins a round usually has its next head at hand, and the wave enters
  // the (divergent, 24-element) rescan only when one of its lanes wins a third time
  float nv = NEG;
  int ni = INT_MAX;
  bv = NEG; bi = INT_MAX;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = tid + i * NTH;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float val = x[i][k];
      const int v = vi * VEC + k;
      const bool b1 = (val > bv) | ((val == bv) & (v < bi));    // NaN (not a candidate): false
      const bool b2 = (val > nv) | ((val == nv) & (v < ni));
      nv = b1 ? bv : (b2 ? val : nv);
      ni = b1 ? bi : (b2 ? v : ni);
      bv = b1 ? val : bv;
      bi = b1 ? v : bi;
    }
  }
  bool have_next = true;
  for (int k = 0; k < K; ++k) {
    float cv = bv;
    int ci = bi;
    wave_argmax<32>(cv, ci);
    const bool won = bi == ci && ci != INT_MAX;  // this lane owns the wave's winner: take it, bring up its next best
    if (won) {
      tv = bv; ti = bi;
      bv = nv; bi = ni;
    }
    if (__builtin_expect(__any(won && !have_next), 0)) {
      if (won && !have_next) rescan();
    }
    if (won) have_next = false;
    if (lane == 0) { w_val[wave * KMAX_ALL + k] = cv; w_tok[wave * KMAX_ALL + k] = ci; }
  }
  __syncthreads();
  if (wave == 0) {
    int pos = 0;  // lanes 0 .. NW-1: the next unread entry of wave `lane`'s list
    float hv = lane < NW ? w_val[lane * KMAX_ALL] : NEG;
    int hi_ = lane < NW ? w_tok[lane * KMAX_ALL] : INT_MAX;
    float ov = NEG;
    int ot = INT_MAX;
    for (int k = 0; k < K; ++k) {
      float cv = hv;
      int ci = hi_;
      wave_argmax<NW / 2>(cv, ci);
      cv = __shfl(cv, 0, 64);
      ci = __shfl(ci, 0, 64);
      if (lane < NW && hi_ == ci && ci != INT_MAX) {  // this list's head was taken: advance
        ++pos;
        hv = pos < K ? w_val[lane * KMAX_ALL + pos] : NEG;
        hi_ = pos < K ? w_tok[lane * KMAX_ALL + pos] : INT_MAX;
      }
      if (lane == k) { ov = cv; ot = ci == INT_MAX ? p.pad : ci; }
    }
    if (lane < K) {
      cand_val[(int64_t)h * K + lane] = ov;
      cand_tok[(int64_t)h * K + lane] = ot;
    }
  }
}

// The generic-width body: rows too long for registers are re-read from memory (L2-resident) on every scan; with ENS every scan
// recombines the N rows element by element, with CON every scan consults the ban filter.  It only selects.
template <typename T, bool ENS, bool CON, bool LM>
__device__ __forceinline__ void beam_row_wide(const BeamP& p, const EnsArg<ENS>& e, const LmArg<LM>& lm, const LexArg<CON>& lx, float* cand_val,
                                              int32_t* cand_tok) {
  constexpr int NTH = 512, NW = NTH / 64, BANW = 256;
  RowCtx c;
  if (!row_prologue<CON>(p, c)) return;
  const int s = c.s, h = c.h, hs = c.hs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = p.vocab, K = 2 * p.beam;
  const float NEG = -INFINITY;
  __shared__ uint32_t ban[CON ? BANW : 1];
  const int64_t* tk = nullptr;
  if constexpr (CON) {
    if (tid < BANW) ban[tid] = 0u;
    __syncthreads();
    tk = row_tokens(p, c);
    ngram_banned(tk, s, p.ngram, tid, NTH, [&](int64_t v) { atomicOr(&ban[(v >> 5) & (BANW - 1)], 1u << (v & 31)); });
  }
  auto banned = [&](int v) -> bool {
    if (!((ban[(v >> 5) & (BANW - 1)] >> (v & 31)) & 1u)) return false;
    bool hit = false;
    ngram_banned(tk, s, p.ngram, 0, 1, [&](int64_t b) { hit = hit || b == v; });
    return hit;
  };
  __shared__ LseSm<(ENS ? ENS_MAX : 1) + (LM ? 1 : 0), NW> st;
  __shared__ float wv[NW];
  __shared__ int wi[NW];
  __shared__ float o_val[KMAX_ALL];
  __shared__ int o_tok[KMAX_ALL];
  int nmem = 1;
  if constexpr (ENS) nmem = e.n;
  [[maybe_unused]] const T* lmrow = nullptr;  // the LM's row (untempered); its statistics take slot nmem
  if constexpr (LM) lmrow = reinterpret_cast<const T*>(lm.logits) + (int64_t)hs * p.ld_logits;
  block_lse(nmem + (LM ? 1 : 0), st, [&](int n, float& mx, float& sum) {
    mx = NEG;
    sum = 0.0f;
    if constexpr (LM) {
      if (n == nmem) {
        for (int v = tid; v < V; v += NTH) lse_push(mx, sum, DT<T>::ld(lmrow + v));  // (a NaN element makes the sum NaN)
        return;
      }
    }
    const T* ln = member_row<T, ENS>(p, e, n, hs);
    bool nan = false;
    for (int v = tid; v < V; v += NTH) {
      const float xv = temper<ENS>(DT<T>::ld(ln + v), p, e);
      if constexpr (ENS) { nan = nan || xv != xv; lse_merge(mx, sum, xv, 1.0f); }
      else lse_push(mx, sum, xv);
    }
    if (nan) sum = NAN;
  });
  float lse = 0.0f;
  bool bad = false;
  if constexpr (ENS) bad = ens_bad(st.lse, e.n);
  else lse = st.lse[0];
  [[maybe_unused]] const T* lg = member_row<T, ENS>(p, e, 0, hs);
  // the model's log-probability of token v
  auto lprob_model = [&](int v) -> float {
    if constexpr (ENS) {
      float m = NEG, a = 0.0f;
      for (int n = 0; n < e.n; ++n) lse_merge(m, a, temper<ENS>(DT<T>::ld(member_row<T, ENS>(p, e, n, hs) + v), p, e) - st.lse[n], 1.0f);
      return ens_lprob(m, a, bad, e.log_n);
    } else {
      return temper<ENS>(DT<T>::ld(lg + v), p, e) - lse;
    }
  };
  [[maybe_unused]] float lse_lm = 0.0f;
  if constexpr (LM) lse_lm = st.lse[nmem];
  // log-probability of token v before the masks (with LM: lp')
  auto lprob = [&](int v) -> float {
    if constexpr (LM) return lm_fuse(lprob_model(v), lm.weight, DT<T>::ld(lmrow + v), lse_lm);
    else return lprob_model(v);
  };
  if constexpr (ENS) {
    if (e.lprobs_out)
      for (int v = tid; v < V; v += NTH) e.lprobs_out[(int64_t)h * p.ld_logits + v] = lprob_model(v);
  }
  if constexpr (LM) {
    if (lm.lprobs_out)
      for (int v = tid; v < V; v += NTH) lm.lprobs_out[(int64_t)h * p.ld_logits + v] = lprob(v);
  }
  const float prev = row_prev_score(p, c);
  const int32_t* lex_st = lex_row_state<CON>(p, lx, c);  // the row's constraint state (nullptr: no lexical constraints)
  const bool lex_no_eos = lex_st != nullptr && s > 0 && lex_st[LS_FIN] == 0;
  // the candidate value of token v
  auto value = [&](int v) -> float {
    float val = mask_lprob<CON>(p, c, v, lprob(v), [&](float cur) { return cur != NEG && banned(v); });
    if (lex_no_eos && v == p.eos) val = NEG;  // eos only once the constraints are met (search.py:308-321)
    if (s > 0) val += prev;                   // search.py:125
    return val;
  };
  if constexpr (CON) {  // the values of the state's next tokens (search.py:398-410), by the thread whose share of the row holds the token
    if (lex_st != nullptr) {
      const int nn = lex_st[LS_NNEXT] < LEX_NEXT_MAX ? lex_st[LS_NNEXT] : LEX_NEXT_MAX;
      for (int j = 0; j < nn; ++j) {
        const int t = lex_st[LS_NEXT + j];
        const bool inside = t >= 0 && t < V;
        if (tid != (inside ? t % NTH : 0)) continue;
        lx.nval[(int64_t)h * LEX_NEXT_MAX + j] = inside ? value(t) : NEG;
        lx.ntok[(int64_t)h * LEX_NEXT_MAX + j] = t;
      }
    }
  }
  // local best that is strictly worse than (tv, ti) — the thread's previously taken candidate
  float tv = INFINITY, bv;
  int ti = -1, bi;
  auto rescan = [&]() {
    bv = NEG; bi = INT_MAX;
    for (int v = tid; v < V; v += NTH) {
      const float val = value(v);
      const bool open = val < tv || (val == tv && v > ti);
      if (open && cand_better(val, v, bv, bi)) { bv = val; bi = v; }
    }
  };
  rescan();
  for (int k = 0; k < K; ++k) {  // a block-wide arg-max per candidate; the winning thread rescans its share of the row
    float cv = bv;
    int ci = bi;
    wave_argmax<32>(cv, ci);
    if (lane == 0) { wv[wave] = cv; wi[wave] = ci; }
    __syncthreads();
    cv = wv[0]; ci = wi[0];
    for (int w = 1; w < NW; ++w)
      if (cand_better(wv[w], wi[w], cv, ci)) { cv = wv[w]; ci = wi[w]; }
    if (bi == ci && ci != INT_MAX) { tv = bv; ti = bi; rescan(); }
    if (tid == 0) { o_val[k] = cv; o_tok[k] = ci == INT_MAX ? p.pad : ci; }
    __syncthreads();
  }
  if (tid < K) {
    cand_val[(int64_t)h * K + tid] = o_val[tid];
    cand_tok[(int64_t)h * K + tid] = o_tok[tid];
  }
}

// NV vectors per thread in registers; NV == 0: the wide body
template <typename T, int NV, bool ENS, bool CON, bool SAMP, bool LM>
__global__ __launch_bounds__(512) void beam_row_kernel(BeamP p, float* cand_val, int32_t* cand_tok, EnsArg<ENS> e, LmArg<LM> lm, LexArg<CON> lx) {
  static_assert(NV > 0 || !SAMP, "the wide body only selects");
  if constexpr (NV == 0) beam_row_wide<T, ENS, CON, LM>(p, e, lm, lx, cand_val, cand_tok);
  else beam_row_regs<T, NV, ENS, CON, SAMP, LM>(p, e, lm, lx, cand_val, cand_tok);
}

// ---- beam search step, kernel 2 of 2: one workgroup per SENTENCE -------------------------------------------------------------
// merges the rows' sorted candidate lists into the sentence's top-(2*beam) over beam*V (search.py:127-135: flat index =
// beam*V + token, ties to the smaller flat index), then (d) the eos / finalize / active-hypothesis bookkeeping of
// sequence_generator.py:340-499 and finalize_hypos :575-696, (e) the token / score / ancestry rows of the next step written
// into the other half of the ping-pong buffers; the last workgroup to finish advances the step counter.
// PFX (a prefix is given): where the sentence's prefix token of this step is eos, its rows all searched the FIRST row's distribution
// (see CON above), so that row is the parent of every candidate: `beam` identical hypotheses are finalised, as in the reference.
// SAMP (sampling, search.py Sampling.step :733-742): the sentence has K = beam candidates, candidate k drawn by row k from its own
// distribution (beams_buf = arange(beam); row 0 at step 0 and where the prefix holds eos) — there is nothing to rank, and (d), (e) run
// over K = beam: every slot yields exactly one sample.
// DIV = 1 (beam groups, search.py DiverseBeamSearch.step :568-618, Hamming diversity): with G = div_groups, mb = beam / G, group g owns
// the rows r with r % G == g (the reference's lprobs[:, g::G]) and selects, in the order g = 0 .. G-1, its top 2*mb over its mb * V
// candidates by  value = fl(fl(lp + cumulative score) + fl(-S * count_g(token)))  — the row kernel's candidate value plus the penalty;
// the reference adds the penalty to lp first, a difference of one fp32 rounding of the cumulative score.  count_g(t) = how many of the
// 2*mb selections of each of the groups 0 .. g-1 of this sentence at this step have token t (all of them: duplicates, eos and -inf
// candidates included, like the reference's scatter_add_).  Ties go to the smaller flat index local_row * V + token.  The group's j-th
// selection is the sentence's candidate j * G + g (torch.stack(..., dim=2)) with parent row local_row * G + g; the penalised value is
// the score that (d) and (e) write.  Step 0: every group searches the first row's list (the rows are equal there) and the parent is
// the first row.
// The rows' top 2*beam lists suffice: with S >= 0 the penalty only lowers values, and only those of the at most 2*beam - 2*mb distinct
// tokens the earlier groups selected.  A token outside its row's unpenalised top 2*beam has at least 2*beam tokens of that row in front
// of it, at least 2*mb of them unpenalised, which keep a value at least as large: it cannot enter the group's top 2*mb.
// The G rounds run inside the one workgroup: (1) one thread per candidate of the group's rows forms the penalised value (the count is a
// scan of an LDS list of at most 2*beam - 2*mb <= 38 tokens), (2) the one-thread-per-candidate rank loop below over the round's
// mb * 2*beam values, (3) rank < 2*mb writes the candidate and appends its token to the list.  Two barriers per round, no global
// traffic, no atomics.
// DIV = 2 (diverse siblings, search.py DiverseSiblingsSearch.step :765-814): at steps s > 0 the candidate at position p (from 0) of a
// row's sorted list has the value fl(v - fl((p + 1) * R)), formed where the lists are staged; the lists stay sorted, so the rank loop
// and its tie rule (smaller row * 2*beam + p) are the plain ones.  Step 0 is plain beam search.
// DIV = 3 (lexical constraints, search.py LexicallyConstrainedBeamSearch.step / step_sentence :263-523; the tables and states are
// described at LexP above).  After the plain selection, which yields the sentence's top 2*beam, the list L is staged in LDS:
//   (1) that top 2*beam; at steps s > 0 every row's own best candidate (the head of its sorted list) in row order; then per row in row
//       order (only the first row at s = 0) one candidate per next token of the row's state in ascending token order, with the value the
//       row kernel left in LexP::nval — formed by the same operations as a list entry, so a duplicate is bit-equal to its twin;
//   (2) one thread per candidate advances its PARENT's state by the candidate's token (lex_advance, nothing stored) for the bank, and
//       forms the fp32 key  fl(float((nd - bank) * -100) + value);
//   (3) rank by counting: key descending, stable with respect to L (the order IS that of the fp32 key, as the reference's sort_key);
//   (4) a candidate whose predecessor in that order — cyclically, the first looks at the last — has the same (parent, token) is dropped;
//   (5) the j-th survivor of a run of equal banks gets the stripe nd - bank + j * (survivors + 1); a second rank by counting, stripe
//       ascending and stable, and the first 2*beam are the sentence's candidates (score = value, token, parent).
// (d) and (e) then run over those; after them thread i < beam re-advances the parent state of candidate act[i] into a staging row,
// derives its FIN / NEXT words, and the workgroup copies the rows into the other half of the state pair (update_constraints :254-260).
template <bool PFX, bool SAMP = false, int DIV = 0>
__global__ __launch_bounds__(256) void beam_merge_kernel(BeamP p, const float* cand_val, const int32_t* cand_tok, int32_t* ticket,
                                                         LexArg<DIV == 3> lx) {
  constexpr bool LEX = DIV == 3;
  const int s = *p.step;
  const int sent = blockIdx.x, tid = threadIdx.x;
  const int beam = p.beam, K = SAMP ? beam : 2 * beam, bbsz = p.bsz * beam;
  const int L1 = p.max_len + 1, LT = p.max_len + 2;
  const int rows = s == 0 ? 1 : beam;
  const int cur = s & 1, nxt = cur ^ 1;
  const int64_t* tok_old = p.tokens + (int64_t)cur * bbsz * LT;
  int64_t* tok_new = p.tokens + (int64_t)nxt * bbsz * LT;
  const float* sc_old = p.scores + (int64_t)cur * bbsz * L1;
  float* sc_new = p.scores + (int64_t)nxt * bbsz * L1;
  const int32_t* anc_old = p.anc + (int64_t)cur * bbsz * L1;
  int32_t* anc_new = p.anc + (int64_t)nxt * bbsz * L1;
  const float NEG = -INFINITY;
  __shared__ float l_val[BEAM_MAX * KMAX_ALL];
  __shared__ int l_tok[BEAM_MAX * KMAX_ALL];
  __shared__ float c_score[KMAX_ALL];
  __shared__ int c_tok[KMAX_ALL], c_beam[KMAX_ALL], c_em[KMAX_ALL];
  __shared__ int act[BEAM_MAX], rec_k[BEAM_MAX], rec_r[BEAM_MAX], n_rec;
  __shared__ int ign[BEAM_MAX], ign_new[BEAM_MAX];
  __shared__ int32_t x_tbl[LEX ? LEX_TBL_W : 1], x_st[LEX ? BEAM_MAX * LEX_SW : 1], x_new[LEX ? BEAM_MAX * LEX_SW : 1];
  bool first_row_parent = false;
  if constexpr (PFX) first_row_parent = prefix_step(p, s) && p.prefix_tokens[(int64_t)sent * p.prefix_len + s] == p.eos;
  if (s <= p.max_len) {
    if constexpr (SAMP) {
      if (tid < beam) {
        c_score[tid] = cand_val[(int64_t)sent * beam + tid];
        c_tok[tid] = cand_tok[(int64_t)sent * beam + tid];
        c_beam[tid] = (s == 0 || first_row_parent) ? 0 : tid;
        ign[tid] = p.cands_to_ignore[sent * beam + tid];
      }
      __syncthreads();
    } else {
    for (int i = tid; i < rows * K; i += blockDim.x) {
      float v = cand_val[(int64_t)sent * beam * K + i];
      if constexpr (DIV == 2) { if (s > 0) v = __fsub_rn(v, __fmul_rn((float)(i % K + 1), p.sibling_rate)); }  // (no contraction to an fma)
      l_val[i] = v;
      l_tok[i] = cand_tok[(int64_t)sent * beam * K + i];
    }
    if (tid < beam) ign[tid] = p.cands_to_ignore[sent * beam + tid];
    __syncthreads();
    if constexpr (DIV == 1) {
      __shared__ float g_val[BEAM_MAX * KMAX_ALL];
      __shared__ int g_key[BEAM_MAX * KMAX_ALL];   // local_row * V + token (beam * V < INT_MAX)
      __shared__ int sel_tok[KMAX_ALL];            // the tokens the earlier groups selected at this step
      const int G = p.div_groups, mb = beam / G, Kg = 2 * mb, ng = (s == 0 ? 1 : mb) * K;
      const float alpha = -p.div_strength;
      for (int g = 0; g < G; ++g) {
        for (int i = tid; i < ng; i += blockDim.x) {
          const int lr = i / K, src = (s == 0 ? 0 : lr * G + g) * K + (i - lr * K);
          const int t = l_tok[src];
          int cnt = 0;
          for (int q = 0; q < g * Kg; ++q) cnt += sel_tok[q] == t ? 1 : 0;
          const float v = l_val[src];
          g_val[i] = cnt ? __fadd_rn(v, __fmul_rn(alpha, (float)cnt)) : v;
          g_key[i] = lr * p.vocab + t;
        }
        __syncthreads();
        for (int i = tid; i < ng; i += blockDim.x) {
          const float v = g_val[i];
          const int key = g_key[i];
          int rank = 0;
          for (int o = 0; o < ng; ++o) {
            const float vo = g_val[o];
            const int ko = g_key[o];
            rank += (vo > v || (vo == v && (ko < key || (ko == key && o < i)))) ? 1 : 0;  // (equal keys: missing candidates, (-inf, pad))
          }
          if (rank < Kg) {
            const int lr = i / K, k = rank * G + g, t = key - lr * p.vocab;
            c_score[k] = v; c_tok[k] = t; c_beam[k] = (s == 0 || first_row_parent) ? 0 : lr * G + g;
            sel_tok[g * Kg + rank] = t;
          }
        }
        __syncthreads();
      }
    } else {
    // rank of every row candidate among the sentence's rows*K candidates (ordered by value desc, then row asc = flat index asc,
    // then position in the row's list): rank < K -> it is the sentence's candidate number `rank`.  One thread per candidate; a
    // serial K-round head merge by one thread cost ~8 us of dependent LDS round trips.
    for (int i = tid; i < rows * K; i += blockDim.x) {
      const float v = l_val[i];
      const int r = i / K;
      int rank = 0;
      for (int o = 0; o < rows * K; ++o) {
        const float vo = l_val[o];
        rank += (vo > v || (vo == v && o < i)) ? 1 : 0;   // lists are sorted within a row, so o < i orders equal values by (row, position)
      }
      if (rank < K) { c_score[rank] = v; c_tok[rank] = l_tok[i]; c_beam[rank] = first_row_parent ? 0 : r; }
    }
    __syncthreads();
    if constexpr (LEX) {
      __shared__ float L_val[LEX_L_MAX], L_key[LEX_L_MAX];
      __shared__ int L_tok[LEX_L_MAX], L_par[LEX_L_MAX], L_bank[LEX_L_MAX];
      __shared__ int L_ord[LEX_L_MAX], L_keep[LEX_L_MAX], L_stripe[LEX_L_MAX];  // by position in the key order
      __shared__ int L_off[BEAM_MAX + 1];
      const int nthr = blockDim.x;
      for (int i = tid; i < LEX_TBL_W; i += nthr) x_tbl[i] = lx.tbl[(int64_t)sent * LEX_TBL_W + i];
      for (int i = tid; i < beam * LEX_SW; i += nthr) x_st[i] = lx.state[((int64_t)cur * bbsz + (int64_t)sent * beam) * LEX_SW + i];
      __syncthreads();
      if (tid == 0) {  // where each row's next-token candidates start in L
        int at = K + (s > 0 ? beam : 0);
        for (int r = 0; r < rows; ++r) {
          L_off[r] = at;
          const int nn = x_st[r * LEX_SW + LS_NNEXT];
          at += nn < 0 ? 0 : (nn < LEX_NEXT_MAX ? nn : LEX_NEXT_MAX);
        }
        L_off[rows] = at;
      }
      __syncthreads();
      const int nL = L_off[rows], nd = x_tbl[0];
      for (int i = tid; i < nL; i += nthr) {  // (1), (2)
        float v;
        int t, par;
        if (i < K) { v = c_score[i]; t = c_tok[i]; par = c_beam[i]; }
        else if (i < L_off[0]) { par = i - K; v = l_val[par * K]; t = l_tok[par * K]; }
        else {
          par = 0;
          while (par + 1 < rows && i >= L_off[par + 1]) ++par;
          const int j = i - L_off[par];
          v = lx.nval[((int64_t)sent * beam + par) * LEX_NEXT_MAX + j];
          t = x_st[par * LEX_SW + LS_NEXT + j];
        }
        const int bank = lex_advance(x_tbl, x_st + par * LEX_SW, t, nullptr);
        L_val[i] = v; L_tok[i] = t; L_par[i] = par; L_bank[i] = bank;
        L_key[i] = __fadd_rn((float)((nd - bank) * -100), v);
      }
      __syncthreads();
      for (int i = tid; i < nL; i += nthr) {  // (3)
        const float key = L_key[i];
        int rank = 0;
        for (int o = 0; o < nL; ++o) {
          const float ko = L_key[o];
          rank += (ko > key || (ko == key && o < i)) ? 1 : 0;
        }
        L_ord[rank] = i;
      }
      if (tid < K) { c_score[tid] = NEG; c_tok[tid] = p.pad; c_beam[tid] = 0; }  // (never left: L holds 2*beam distinct pairs)
      __syncthreads();
      for (int q = tid; q < nL; q += nthr) {  // (4)
        const int i = L_ord[q], o = L_ord[q == 0 ? nL - 1 : q - 1];
        L_keep[q] = (L_par[i] == L_par[o] && L_tok[i] == L_tok[o]) ? 0 : 1;
      }
      __syncthreads();
      for (int q = tid; q < nL; q += nthr) {  // (5): stripes
        int len = 0;
        for (int o = 0; o < nL; ++o) len += L_keep[o];
        const int bank = L_bank[L_ord[q]];
        int j = 0;
        for (int o = q - 1; o >= 0; --o) {
          if (!L_keep[o]) continue;
          if (L_bank[L_ord[o]] != bank) break;
          ++j;
        }
        L_stripe[q] = L_keep[q] ? nd - bank + j * (len + 1) : INT_MAX;
      }
      __syncthreads();
      for (int q = tid; q < nL; q += nthr) {  // (5): the first 2*beam by stripe
        if (!L_keep[q]) continue;
        const int st = L_stripe[q];
        int rank = 0;
        for (int o = 0; o < nL; ++o) rank += (L_keep[o] && (L_stripe[o] < st || (L_stripe[o] == st && o < q))) ? 1 : 0;
        if (rank < K) {
          const int i = L_ord[q];
          c_score[rank] = L_val[i]; c_tok[rank] = L_tok[i]; c_beam[rank] = L_par[i];
        }
      }
      __syncthreads();
    }
    }
    }
    if (tid == 0) {
      // ---- (d) bookkeeping (LDS / registers only: a global access inside these serial loops costs a memory round trip each) ----
      bool any_top_eos = false;
      int nr = 0;
      int nf = p.nfinal[sent];
      const bool was_finished = p.finished[sent] != 0;
      for (int k = 0; k < K; ++k) {
        bool e = c_tok[k] == p.eos && c_score[k] != NEG;                       // :341
        if (k < beam && ign[k]) e = false;                                     // :346
        c_em[k] = e ? 1 : 0;
        if (k < beam && e) {
          any_top_eos = true;
          if (!was_finished && nf < beam) { rec_k[nr] = k; rec_r[nr] = nf; ++nr; ++nf; }   // finalize_hypos :575-696
        }
      }
      n_rec = nr;
      p.nfinal[sent] = nf;
      if (any_top_eos && !was_finished && (nf == beam || s == p.max_len)) {     // is_finished :698-713
        p.finished[sent] = 1;
        atomicSub(p.num_remaining, 1);
      }
      // active hypotheses: the first `beam` candidates that are not eos / ignored, in candidate order (:465-499)
      int na = 0;
      for (int k = 0; k < K && na < beam; ++k) {
        const bool e = c_em[k] || (k < beam && ign[k]);
        if (!e) act[na++] = k;
      }
      const int n_live = na;
      for (int k = 0; k < K && na < beam; ++k) {
        const bool e = c_em[k] || (k < beam && ign[k]);
        if (e) act[na++] = k;
      }
      for (int i = 0; i < beam; ++i) ign_new[i] = i >= n_live ? 1 : 0;
    }
    __syncthreads();
    if (tid < beam) p.cands_to_ignore[sent * beam + tid] = (uint8_t)ign_new[tid];
    // ---- finalized hypotheses (tokens[bi, 1:step+2] with eos at [step]; positional scores = differences) ----
    for (int q = 0; q < n_rec; ++q) {
      const int k = rec_k[q], r = rec_r[q];
      const int64_t bi = sent * beam + c_beam[k], slot = (int64_t)sent * beam + r;
      const float sc = c_score[k];
      for (int j = tid; j <= s; j += blockDim.x) {
        p.fin_tokens[slot * L1 + j] = j == s ? (int64_t)p.eos : tok_old[bi * LT + j + 1];
        const float cum = j == s ? sc : sc_old[bi * L1 + j];
        const float before = j > 0 ? sc_old[bi * L1 + j - 1] : 0.0f;
        p.fin_pos[slot * L1 + j] = j > 0 ? cum - before : cum;
        if (p.fin_anc) p.fin_anc[slot * L1 + j] = anc_old[bi * L1 + j];
      }
      if (tid == 0) {
        p.fin_len[slot] = s + 1;
        p.fin_score[slot] = p.normalize_scores ? sc / (float)pow((double)(s + 1), (double)p.len_penalty) : sc;
      }
    }
    // ---- (e) rows of the next step ----
    if (s < p.max_len) {
      // (one flat loop over (row, position): a loop over the rows around a loop over the positions is `beam` dependent memory round trips)
      for (int idx = tid; idx < beam * (s + 1); idx += blockDim.x) {
        const int i = idx / (s + 1), j = idx - i * (s + 1);
        const int64_t src = sent * beam + c_beam[act[i]], dst = (int64_t)sent * beam + i;
        tok_new[dst * LT + j] = tok_old[src * LT + j];
        anc_new[dst * L1 + j] = anc_old[src * L1 + j];
        if (j < s) sc_new[dst * L1 + j] = sc_old[src * L1 + j];
      }
      if (tid < beam) {
        const int k = act[tid];
        const int64_t dst = (int64_t)sent * beam + tid;
        tok_new[dst * LT + s + 1] = c_tok[k];
        sc_new[dst * L1 + s] = c_score[k];
        anc_new[dst * L1 + s + 1] = (int32_t)dst;
      }
      if constexpr (LEX) {  // next row i takes the advanced state of its candidate
        if (tid < beam) {
          const int k = act[tid];
          const int32_t* from = x_st + c_beam[k] * LEX_SW;
          int32_t* to = x_new + tid * LEX_SW;
          for (int w = 0; w < LEX_SW; ++w) to[w] = from[w];
          lex_advance(x_tbl, from, c_tok[k], to);
          lex_derive(x_tbl, to);
        }
        __syncthreads();
        for (int i = tid; i < beam * LEX_SW; i += blockDim.x)
          lx.state[((int64_t)nxt * bbsz + (int64_t)sent * beam) * LEX_SW + i] = x_new[i];
      }
    }
  }
  // the last workgroup to get here advances the step (every workgroup has read *p.step by now)
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {
      *ticket = 0;
      if (s <= p.max_len) *p.step = s + 1;
      __threadfence();
    }
  }
}

int to_params(const cst_beam_desc* d, BeamP& p) {
  CST_REQUIRE(d != nullptr, "cst_beam: null descriptor");
  CST_REQUIRE(d->dtype == CST_F32 || d->dtype == CST_BF16, "cst_beam: bad dtype %d", d->dtype);
  CST_REQUIRE(d->bsz > 0 && d->beam > 0 && d->beam <= 20, "cst_beam: bsz %lld / beam %lld (beam <= 20)", (long long)d->bsz, (long long)d->beam);
  CST_REQUIRE(d->vocab > 2 * d->beam + 1 && d->beam * d->vocab < INT_MAX, "cst_beam: vocabulary %lld too small / large for beam %lld",
              (long long)d->vocab, (long long)d->beam);
  CST_REQUIRE(d->max_len >= 1 && d->min_len <= d->max_len, "cst_beam: max_len %lld / min_len %lld", (long long)d->max_len, (long long)d->min_len);
  CST_REQUIRE(d->temperature > 0.0f, "cst_beam: temperature must be positive");
  CST_REQUIRE(d->step && d->tokens && d->scores && d->anc && d->cands_to_ignore && d->finished && d->nfinal && d->num_remaining &&
                  d->fin_tokens && d->fin_pos && d->fin_score && d->fin_len, "cst_beam: null state buffer");
  p.bsz = (int)d->bsz; p.beam = (int)d->beam; p.vocab = (int)d->vocab; p.max_len = (int)d->max_len;
  p.pad = (int)d->pad; p.unk = (int)d->unk; p.eos = (int)d->eos; p.min_len = (int)d->min_len;
  p.unk_penalty = d->unk_penalty; p.len_penalty = d->len_penalty; p.inv_temperature = 1.0f / d->temperature;
  p.normalize_scores = d->normalize_scores;
  p.logits = d->logits; p.ld_logits = d->ld_logits;
  p.step = d->step; p.tokens = d->tokens; p.scores = d->scores; p.anc = d->anc;
  p.cands_to_ignore = d->cands_to_ignore; p.finished = d->finished; p.nfinal = d->nfinal; p.num_remaining = d->num_remaining;
  p.fin_tokens = d->fin_tokens; p.fin_pos = d->fin_pos; p.fin_score = d->fin_score; p.fin_len = d->fin_len;
  p.ngram = 0; p.prefix_len = 0; p.prefix_tokens = nullptr;  // cst_beam_step sets them
  p.sample_topk = 0; p.sample_topp = 0.0f; p.sample_key = nullptr;
  p.div_groups = 0; p.div_strength = 0.0f; p.sibling_rate = 0.0f;
  p.fin_anc = d->fin_anc;
  return CST_OK;
}

// Runtime choices -> template arguments: dispatch(f, Choice<A, B, ...>{i}, Choice<...>{j}, ...) calls f(X{}, Y{}, ...) with X the i-th
// type of the first list, Y the j-th of the second, ...; f is a generic lambda that reads its constants from the argument TYPES.
template <typename... Cs> struct Choice { int i; };
template <typename T> struct Type { using type = T; };
template <int N> using Int = std::integral_constant<int, N>;
using Bool = Choice<std::false_type, std::true_type>;
template <typename F>
void dispatch(F&& f) { f(); }
template <typename F, typename C0, typename... Cs, typename... Rest>
void dispatch(F&& f, Choice<C0, Cs...> c, Rest... rest) {
  if constexpr (sizeof...(Cs) == 0) dispatch([&](auto... a) { f(C0{}, a...); }, rest...);
  else if (c.i == 0) dispatch([&](auto... a) { f(C0{}, a...); }, rest...);
  else dispatch(f, Choice<Cs...>{c.i - 1}, rest...);
}

// what cst_lex_init and cst_beam_step_lex refuse alike; on CST_OK the workspace's four parts are in lp
int lex_params(const cst_beam_desc* d, const cst_lex_desc* x, LexP& lp) {
  CST_REQUIRE(x->representation == 1 || x->representation == 2, "cst_lex: representation %lld (1 ordered, 2 unordered)", (long long)x->representation);
  CST_REQUIRE(x->workspace != nullptr && ((uintptr_t)x->workspace % 16) == 0, "cst_lex: workspace of cst_lex_workspace() bytes required, 16-byte aligned");
  CST_REQUIRE(x->width >= 1, "cst_lex: width %lld (a packed row holds at least its count)", (long long)x->width);
  if (x->width > LEX_WIDTH_MAX) {
    cst_set_error("cst_lex: a packed row of width %lld holds more than %d constraint tokens: decode such sentences with the host loop",
                  (long long)x->width, LEX_TOK_MAX);
    return CST_ERR_UNSUPPORTED;
  }
  CST_REQUIRE(d->sampling == 0 && d->diverse_groups == 0 && d->diverse_siblings == 0,
              "cst_lex: sampling, the diverse strategies and lexical constraints are mutually exclusive search strategies");
  CST_REQUIRE(d->prefix_len == 0, "cst_lex: lexical constraints cannot be combined with forced prefixes (prefix_len %lld)", (long long)d->prefix_len);
  const int64_t rows = d->bsz * d->beam;
  int32_t* w = reinterpret_cast<int32_t*>(x->workspace);
  lp.tbl = w;
  lp.state = w + d->bsz * LEX_TBL_W;
  lp.nval = reinterpret_cast<float*>(lp.state + 2 * rows * LEX_SW);
  lp.ntok = reinterpret_cast<int32_t*>(lp.nval + rows * LEX_NEXT_MAX);
  return CST_OK;
}

int beam_step_impl(const cst_beam_desc* d, const cst_lm_fusion_desc* f, const cst_lex_desc* x, cst_stream stream);

}  // namespace

extern "C" {
int64_t cst_lex_workspace(int64_t bsz, int64_t beam, int64_t width) {
  // per sentence its table; per row two states and LEX_NEXT_MAX (value, token) next-token candidates.  (width: the packed rows are read
  // in place, the tables have one size)
  (void)width;
  return (bsz * LEX_TBL_W + bsz * beam * (2 * LEX_SW + 2 * LEX_NEXT_MAX)) * (int64_t)sizeof(int32_t);
}

int cst_lex_init(const cst_beam_desc* d, const cst_lex_desc* x, cst_stream stream) {
  BeamP p;
  const int rc = to_params(d, p);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(x != nullptr, "cst_lex_init: null descriptor");
  LexP lp;
  const int rx = lex_params(d, x, lp);
  if (rx != CST_OK) return rx;
  CST_REQUIRE(x->constraints != nullptr, "cst_lex_init: null constraints");
  hipLaunchKernelGGL(lex_init_kernel, dim3(p.bsz), dim3(64), 0, (hipStream_t)stream, x->constraints, (int)x->width, (int)x->representation, p.beam,
                     p.bsz * p.beam, const_cast<int32_t*>(lp.tbl), lp.state);
  return cst_check_launch("cst_lex_init");
}

int cst_beam_init(const cst_beam_desc* d, cst_stream stream) {
  BeamP p;
  const int rc = to_params(d, p);
  if (rc != CST_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  CST_REQUIRE(d->workspace != nullptr, "cst_beam_init: workspace of cst_beam_workspace() bytes required");
  hipLaunchKernelGGL(beam_init_kernel, dim3(p.bsz * p.beam), dim3(256), 0, s, p, reinterpret_cast<int32_t*>(d->workspace));
  return cst_check_launch("cst_beam_init");
}

int64_t cst_beam_workspace(int64_t bsz, int64_t beam) {
  // per row 2*beam (value, token) candidates + the step ticket
  return bsz * beam * 2 * beam * (int64_t)(sizeof(float) + sizeof(int32_t)) + 64;
}

int cst_beam_step(const cst_beam_desc* d, cst_stream stream) { return beam_step_impl(d, nullptr, nullptr, stream); }
int cst_beam_step_lm(const cst_beam_desc* d, const cst_lm_fusion_desc* f, cst_stream stream) { return beam_step_impl(d, f, nullptr, stream); }
int cst_beam_step_lex(const cst_beam_desc* d, const cst_lm_fusion_desc* f, const cst_lex_desc* x, cst_stream stream) {
  return beam_step_impl(d, f, x, stream);
}

}  // extern "C"

namespace {
int beam_step_impl(const cst_beam_desc* d, const cst_lm_fusion_desc* f, const cst_lex_desc* x, cst_stream stream) {
  BeamP p;
  const int rc = to_params(d, p);
  if (rc != CST_OK) return rc;
  CST_REQUIRE(d->logits != nullptr && d->ld_logits >= d->vocab, "cst_beam_step: null logits / ld_logits < vocab");
  const int64_t vec = d->dtype == CST_BF16 ? 8 : 4;
  CST_REQUIRE(d->ld_logits % vec == 0 && d->ld_logits >= cst_ceil_div(d->vocab, vec) * vec && ((uintptr_t)d->logits % 16) == 0,
              "cst_beam_step: logits rows must be 16-byte aligned and padded to a multiple of %lld elements", (long long)vec);
  CST_REQUIRE(d->workspace != nullptr && ((uintptr_t)d->workspace % 16) == 0, "cst_beam_step: workspace of cst_beam_workspace() bytes required");
  // constraints (ABI 10): both off in a zero-filled tail -> the kernels without them
  CST_REQUIRE(d->no_repeat_ngram == 0 || (d->no_repeat_ngram >= 2 && d->no_repeat_ngram <= INT_MAX),
              "cst_beam_step: no_repeat_ngram %lld (0 = off, else >= 2: 1 would ban the initial eos and no hypothesis could finish)",
              (long long)d->no_repeat_ngram);
  CST_REQUIRE(d->prefix_len >= 0 && d->prefix_len <= d->max_len, "cst_beam_step: prefix_len %lld outside [0, max_len %lld]",
              (long long)d->prefix_len, (long long)d->max_len);
  CST_REQUIRE(d->prefix_len == 0 || d->prefix_tokens != nullptr, "cst_beam_step: prefix_len %lld without prefix_tokens", (long long)d->prefix_len);
  p.ngram = (int)d->no_repeat_ngram;
  p.prefix_len = (int)d->prefix_len;
  p.prefix_tokens = d->prefix_len > 0 ? d->prefix_tokens : nullptr;
  const bool con = p.ngram > 0 || p.prefix_len > 0;
  // sampling (ABI 11): off in a zero-filled tail -> the selection kernels, launched as before
  CST_REQUIRE(d->sample_topk >= 0 && d->sample_topk <= d->vocab, "cst_beam_step: sample_topk %lld outside [0, vocab %lld]",
              (long long)d->sample_topk, (long long)d->vocab);
  const bool samp = d->sampling != 0;
  CST_REQUIRE(!samp || d->sample_key != nullptr, "cst_beam_step: sampling without sample_key (a device buffer holding the 32-bit key of the draws)");
  if (samp) {
    p.sample_topk = (int)d->sample_topk;
    p.sample_topp = d->sample_topp;
    p.sample_key = d->sample_key;
    if (cst_ceil_div(cst_ceil_div(d->vocab, d->dtype == CST_BF16 ? 8 : 4), 512) > 5) {
      cst_set_error("cst_beam_step: sampling covers the register-resident row kernels (vocabulary %lld needs the wide kernel, which only "
                    "selects): decode such vocabularies with the host loop", (long long)d->vocab);
      return CST_ERR_UNSUPPORTED;
    }
  }
  // diverse decoding (ABI 12): both strategies off in a zero-filled tail -> the merge kernels above, launched as before
  CST_REQUIRE(d->diverse_groups >= 0, "cst_beam_step: diverse_groups %lld (0 = off, else G >= 1)", (long long)d->diverse_groups);
  const bool groups = d->diverse_groups > 0, siblings = d->diverse_siblings != 0;
  CST_REQUIRE((samp ? 1 : 0) + (groups ? 1 : 0) + (siblings ? 1 : 0) <= 1,
              "cst_beam_step: sampling, diverse_groups and diverse_siblings are mutually exclusive search strategies");
  if (groups) {
    CST_REQUIRE(d->diverse_groups <= d->beam && d->beam % d->diverse_groups == 0,
                "cst_beam_step: beam %lld must be divisible by diverse_groups %lld", (long long)d->beam, (long long)d->diverse_groups);
    CST_REQUIRE(d->diverse_strength >= 0.0f, "cst_beam_step: diverse_strength %g must be >= 0 (a reward would reach tokens outside the "
                "rows' top 2 * beam lists)", (double)d->diverse_strength);
    p.div_groups = (int)d->diverse_groups;
    p.div_strength = d->diverse_strength;
  }
  if (siblings) {
    CST_REQUIRE(d->sibling_rate >= 0.0f, "cst_beam_step: sibling_rate %g must be >= 0", (double)d->sibling_rate);
    p.sibling_rate = d->sibling_rate;
  }
  // checkpoint ensembles: members >= 2 (0 and 1 both mean the single matrix `logits`, today's kernels with today's arguments)
  CST_REQUIRE(d->members >= 0 && d->members <= ENS_MAX, "cst_beam_step: %lld ensemble members (at most %d)", (long long)d->members, ENS_MAX);
  EnsP e;
  e.n = (int)d->members;
  e.temperature = d->temperature;
  e.log_n = logf((float)(d->members > 0 ? d->members : 1));
  e.lprobs_out = d->lprobs_out;
  const bool ens = d->members >= 2;
  CST_REQUIRE(ens || d->lprobs_out == nullptr, "cst_beam_step: lprobs_out is written by the ensemble kernel (members >= 2)");
  CST_REQUIRE(d->lprobs_out == nullptr || ((uintptr_t)d->lprobs_out % 16) == 0, "cst_beam_step: lprobs_out must be 16-byte aligned");
  for (int n = 0; n < ENS_MAX; ++n) {
    e.logits[n] = n == 0 ? d->logits : (n < e.n ? d->logits_n[n - 1] : nullptr);
    CST_REQUIRE(n >= e.n || (e.logits[n] != nullptr && ((uintptr_t)e.logits[n] % 16) == 0),
                "cst_beam_step: logits of ensemble member %d null or not 16-byte aligned", n);
  }
  // shallow fusion (an entry point of its own, added at ABI 13): off without f or without f->lm_logits -> the kernels without it
  const bool lmf = f != nullptr && f->lm_logits != nullptr;
  LmP lmp{nullptr, 0.0f, nullptr};
  if (lmf) {
    CST_REQUIRE(((uintptr_t)f->lm_logits % 16) == 0, "cst_beam_step_lm: lm_logits must be 16-byte aligned (rows laid out like `logits`)");
    CST_REQUIRE(f->lm_weight - f->lm_weight == 0.0f, "cst_beam_step_lm: lm_weight %g is not finite", (double)f->lm_weight);
    CST_REQUIRE(f->lprobs_out == nullptr || ((uintptr_t)f->lprobs_out % 16) == 0, "cst_beam_step_lm: lprobs_out must be 16-byte aligned");
    lmp.logits = f->lm_logits; lmp.weight = f->lm_weight; lmp.lprobs_out = f->lprobs_out;
  }
  // lexical constraints (an entry point of its own, added at ABI 13 like the LM's): off without x -> the kernels and arguments above
  const bool lex = x != nullptr;
  LexP lexp{nullptr, nullptr, nullptr, nullptr};
  if (lex) {
    const int rx = lex_params(d, x, lexp);
    if (rx != CST_OK) return rx;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)p.bsz * p.beam, K = 2 * p.beam;
  int32_t* ticket = reinterpret_cast<int32_t*>(d->workspace);
  float* cand_val = reinterpret_cast<float*>(reinterpret_cast<char*>(d->workspace) + 64);
  int32_t* cand_tok = reinterpret_cast<int32_t*>(cand_val + rows * K);
  {
    CstProfScope prof(CST_K_ELEMENTWISE, s, 0.0, (double)rows * p.vocab * cst_dtype_size(d->dtype) * ((ens ? 2 * e.n : 1) + (lmf ? 2 : 0)));
    // vectors per thread: the register-resident bodies up to 5, the wide body (NV = 0) beyond.  The constraints, the ensemble and
    // sampling are template flags: a descriptor with all of them off launches the instantiations it always did.
    const int64_t per_thread = cst_ceil_div(cst_ceil_div(d->vocab, vec), 512);
    const int bucket = per_thread <= 1 ? 0 : per_thread <= 3 ? 1 : per_thread <= 5 ? 2 : 3;
    dispatch(
        [&](auto type, auto nv, auto ens_c, auto con_c, auto samp_c, auto lm_c) {
          using T = typename decltype(type)::type;
          constexpr int NV = decltype(nv)::value;
          constexpr bool ENS = decltype(ens_c)::value, CON = decltype(con_c)::value, SAMP = decltype(samp_c)::value, LM = decltype(lm_c)::value;
          if constexpr (NV > 0 || !SAMP) {  // (sampling with a wide vocabulary was refused above)
            EnsArg<ENS> ea{};
            if constexpr (ENS) ea = e;
            LmArg<LM> la{};
            if constexpr (LM) la = lmp;
            LexArg<CON> xa{};
            if constexpr (CON) xa = lexp;  // (a null state pointer without lexical constraints)
            hipLaunchKernelGGL((beam_row_kernel<T, NV, ENS, CON, SAMP, LM>), dim3((unsigned)rows), dim3(512), 0, s, p, cand_val, cand_tok, ea, la, xa);
          }
        },
        Choice<Type<float>, Type<bf16_t>>{d->dtype == CST_BF16}, Choice<Int<1>, Int<3>, Int<5>, Int<0>>{bucket}, Bool{ens}, Bool{con || lex}, Bool{samp},
        Bool{lmf});
    dispatch(
        [&](auto pfx_c, auto samp_c, auto div_c) {
          constexpr bool PFX = decltype(pfx_c)::value, SAMP = decltype(samp_c)::value;
          constexpr int DIV = decltype(div_c)::value;
          if constexpr ((!SAMP || DIV == 0) && !(DIV == 3 && PFX)) {  // (exclusive strategies, checked above; no prefix with lexical constraints)
            LexArg<DIV == 3> xa{};
            if constexpr (DIV == 3) xa = lexp;
            hipLaunchKernelGGL((beam_merge_kernel<PFX, SAMP, DIV>), dim3(p.bsz), dim3(256), 0, s, p, (const float*)cand_val, (const int32_t*)cand_tok,
                               ticket, xa);
          }
        },
        Bool{p.prefix_len > 0}, Bool{samp}, Choice<Int<0>, Int<1>, Int<2>, Int<3>>{groups ? 1 : siblings ? 2 : lex ? 3 : 0});
  }
  return cst_check_launch(lex ? "cst_beam_step_lex" : lmf ? "cst_beam_step_lm" : "cst_beam_step");
}

}  // namespace
