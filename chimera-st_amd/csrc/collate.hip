// collate.hip — one launch assembles a translation batch from a device-resident binarised corpus (cst_collate_pairs): the padded
// src_tokens [B, S], prev_output_tokens [B, T], target [B, T] and src_lengths [B] that LanguagePairDataset.collater builds on the host
// (fairseq/data/language_pair_dataset.py:16-126 over data_utils.collate_tokens :34-64) from per-sentence slices, three padded copies and
// four H2D transfers.  The token streams stay in their stored type (uint8 / uint16 / int32 / int64) and are widened to int64 here.
//
// Output-centric: the four outputs are ONE int64 buffer [B*S | B*T | B*T | B]; a thread owns two consecutive words of it and stores them
// as one 16-byte vector (the buffer is 16-byte aligned, the word pair starts at an even index), whichever rows or sections the two
// words fall into.  A word is a pure function of its index: the section, the row b and column c, the sentence i = idx[b], its length
// n = off[i + 1] - off[i] and the column's position j inside the sentence — a token, eos (prev_output_tokens, j = 0) or pad.  Every
// word is written exactly once, padding included; nothing is read from the outputs, there are no atomics and no order between
// threads: the result is bit-reproducible.  Token loads are one element wide (a sentence starts at any element offset, so no wider
// load would be aligned); adjacent lanes read adjacent tokens.  A batch is a few hundred KB at most: the launch, not the bandwidth, is
// what this costs.  An index outside [0, N) yields an all-pad row and length 0 and reads nothing.
//
// cst_collate_blocks (below) is the same launch for the language_modeling task: token blocks of ONE stream, source = target shifted.
#include "cst_common.h"

namespace {

struct CollateArgs {
  const void* src; const void* tgt;
  const int64_t* src_off; const int64_t* tgt_off;
  const int64_t* idx;
  int64_t N, B, S, T, pad, eos;
  int tok_dtype, left_pad_src, left_pad_tgt;
};

__device__ __forceinline__ int64_t collate_load(const void* p, int64_t e, int dt) {
  switch (dt) {  // (wave-uniform)
    case CST_TOK_U8: return (int64_t)((const uint8_t*)p)[e];
    case CST_TOK_U16: return (int64_t)((const uint16_t*)p)[e];
    case CST_TOK_I32: return (int64_t)((const int32_t*)p)[e];
    default: return ((const int64_t*)p)[e];
  }
}

// word e of [src_tokens | prev_output_tokens | target | src_lengths]
__device__ __forceinline__ int64_t collate_word(const CollateArgs& a, int64_t e) {
  const int64_t nsrc = a.B * a.S, ntgt = a.B * a.T;
  if (e >= nsrc + 2 * ntgt) {  // src_lengths
    const int64_t i = a.idx[e - nsrc - 2 * ntgt];
    return (i < 0 || i >= a.N) ? 0 : a.src_off[i + 1] - a.src_off[i];
  }
  const bool is_src = e < nsrc;
  const bool shifted = !is_src && e < nsrc + ntgt;  // prev_output_tokens: eos first, then the target without its last token
  const int64_t r = is_src ? e : (shifted ? e - nsrc : e - nsrc - ntgt);
  const int64_t W = is_src ? a.S : a.T;
  const int64_t b = r / W, c = r - b * W;
  const int64_t i = a.idx[b];
  if (i < 0 || i >= a.N) return a.pad;
  const int64_t* off = is_src ? a.src_off : a.tgt_off;
  const int64_t o = off[i];
  int64_t n = off[i + 1] - o;
  if (n > W) n = W;  // (the host sets W = the batch's longest sentence; a shorter W truncates instead of writing elsewhere)
  const int64_t j = c - ((is_src ? a.left_pad_src : a.left_pad_tgt) ? W - n : 0);
  if (j < 0 || j >= n) return a.pad;
  if (shifted) return j == 0 ? a.eos : collate_load(a.tgt, o + j - 1, a.tok_dtype);
  return collate_load(is_src ? a.src : a.tgt, o + j, a.tok_dtype);
}

__global__ __launch_bounds__(256) void collate_pairs_kernel(CollateArgs a, int64_t* out, int64_t total) {
  const int64_t e = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (e >= total) return;
  const int64_t w0 = collate_word(a, e);
  if (e + 1 < total) {
    longlong2 v;
    v.x = w0;
    v.y = collate_word(a, e + 1);
    *reinterpret_cast<longlong2*>(out + e) = v;
  } else {
    out[e] = w0;
  }
}

// ---- cst_collate_blocks: a language_modeling batch from the split's ONE stream -------------------------------------------------------
// The same form: out = [src_tokens B*T | target B*T | src_lengths B], a thread owns two consecutive words.  Block i = idx[b] is
// (start, len, prev) of `blocks`; n = min(len, T).  target[b, j] = stream[start + j]; src_tokens is the target shifted right by one:
// stream[start + j - 1] for j >= 1, and at j = 0 the token before the block — stream[prev] when the block begins inside a sentence,
// the dictionary's eos when it begins at a sentence's first token (prev < 0), which is NOT stream[start - 1] on a corpus whose
// sentences do not end in eos (token_block_dataset.py:137-138).
struct BlockArgs {
  const void* tok;
  const int64_t* blocks;
  const int64_t* idx;
  int64_t N, B, T, pad, eos;
  int tok_dtype;
};

__device__ __forceinline__ int64_t block_word(const BlockArgs& a, int64_t e) {
  const int64_t nt = a.B * a.T;
  if (e >= 2 * nt) {  // src_lengths
    const int64_t i = a.idx[e - 2 * nt];
    if (i < 0 || i >= a.N) return 0;
    const int64_t n = a.blocks[3 * i + 1];
    return n < a.T ? (n < 0 ? 0 : n) : a.T;
  }
  const bool is_src = e < nt;
  const int64_t r = is_src ? e : e - nt;
  const int64_t b = r / a.T, j = r - b * a.T;
  const int64_t i = a.idx[b];
  if (i < 0 || i >= a.N) return a.pad;
  const int64_t start = a.blocks[3 * i];
  int64_t n = a.blocks[3 * i + 1];
  if (n > a.T) n = a.T;
  if (j >= n) return a.pad;
  if (!is_src) return collate_load(a.tok, start + j, a.tok_dtype);
  if (j > 0) return collate_load(a.tok, start + j - 1, a.tok_dtype);
  const int64_t prev = a.blocks[3 * i + 2];
  return prev < 0 ? a.eos : collate_load(a.tok, prev, a.tok_dtype);
}

__global__ __launch_bounds__(256) void collate_blocks_kernel(BlockArgs a, int64_t* out, int64_t total) {
  const int64_t e = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (e >= total) return;
  const int64_t w0 = block_word(a, e);
  if (e + 1 < total) {
    longlong2 v;
    v.x = w0;
    v.y = block_word(a, e + 1);
    *reinterpret_cast<longlong2*>(out + e) = v;
  } else {
    out[e] = w0;
  }
}

}  // namespace

extern "C" int cst_collate_blocks(const void* stream_tokens, int tok_dtype, const int64_t* blocks, int64_t n_blocks, const int64_t* idx,
                                  int64_t B, int64_t T, int64_t pad, int64_t eos, int64_t* out, cst_stream stream) {
  CST_REQUIRE(stream_tokens && blocks && idx && out, "cst_collate_blocks: null operand");
  CST_REQUIRE(tok_dtype >= CST_TOK_U8 && tok_dtype <= CST_TOK_I64, "cst_collate_blocks: bad token dtype %d", tok_dtype);
  CST_REQUIRE(n_blocks > 0 && B > 0 && T > 0, "cst_collate_blocks: bad shape N %lld B %lld T %lld", (long long)n_blocks, (long long)B, (long long)T);
  CST_REQUIRE(B <= ((int64_t)1 << 31) && T <= ((int64_t)1 << 30) && B * (2 * T + 1) <= ((int64_t)1 << 31),  // (no overflow in the product)
              "cst_collate_blocks: batch too large (B %lld T %lld)", (long long)B, (long long)T);
  CST_REQUIRE((uintptr_t)out % 16 == 0, "cst_collate_blocks: the output buffer is not 16-byte aligned");
  const size_t esz = tok_dtype == CST_TOK_U8 ? 1 : tok_dtype == CST_TOK_U16 ? 2 : tok_dtype == CST_TOK_I32 ? 4 : 8;
  CST_REQUIRE((uintptr_t)stream_tokens % esz == 0, "cst_collate_blocks: the token stream is not element-aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = B * (2 * T + 1);
  CstProfScope prof(CST_K_ELEMENTWISE, s, 0.0, (double)total * 8.0 + 2.0 * (double)B * (double)T * (double)esz);
  BlockArgs a = {stream_tokens, blocks, idx, n_blocks, B, T, pad, eos, tok_dtype};
  const int64_t threads = (total + 1) / 2;
  hipLaunchKernelGGL(collate_blocks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a, out, total);
  return cst_check_launch("cst_collate_blocks");
}

extern "C" int cst_collate_pairs(const void* src_stream, const void* tgt_stream, int tok_dtype, const int64_t* src_offsets,
                                 const int64_t* tgt_offsets, int64_t n_sentences, const int64_t* idx, int64_t B, int64_t S, int64_t T,
                                 int64_t pad, int64_t eos, int left_pad_source, int left_pad_target, int64_t* out, cst_stream stream) {
  CST_REQUIRE(src_stream && tgt_stream && src_offsets && tgt_offsets && idx && out, "cst_collate_pairs: null operand");
  CST_REQUIRE(tok_dtype >= CST_TOK_U8 && tok_dtype <= CST_TOK_I64, "cst_collate_pairs: bad token dtype %d", tok_dtype);
  CST_REQUIRE(n_sentences > 0 && B > 0 && S > 0 && T > 0, "cst_collate_pairs: bad shape N %lld B %lld S %lld T %lld",
              (long long)n_sentences, (long long)B, (long long)S, (long long)T);
  CST_REQUIRE(B <= (1 << 20) && S <= (1 << 20) && T <= (1 << 20) && B * (S + 2 * T + 1) <= ((int64_t)1 << 31),
              "cst_collate_pairs: batch too large (B %lld S %lld T %lld)", (long long)B, (long long)S, (long long)T);
  CST_REQUIRE((uintptr_t)out % 16 == 0, "cst_collate_pairs: the output buffer is not 16-byte aligned");
  const size_t esz = tok_dtype == CST_TOK_U8 ? 1 : tok_dtype == CST_TOK_U16 ? 2 : tok_dtype == CST_TOK_I32 ? 4 : 8;
  CST_REQUIRE((uintptr_t)src_stream % esz == 0 && (uintptr_t)tgt_stream % esz == 0, "cst_collate_pairs: a token stream is not element-aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = B * (S + 2 * T + 1);
  CstProfScope prof(CST_K_ELEMENTWISE, s, 0.0, (double)total * 8.0 + (double)B * (S + 2 * T) * (double)esz);
  CollateArgs a = {src_stream, tgt_stream, src_offsets, tgt_offsets, idx, n_sentences, B, S, T, pad, eos, tok_dtype,
                   left_pad_source != 0, left_pad_target != 0};
  const int64_t threads = (total + 1) / 2;
  hipLaunchKernelGGL(collate_pairs_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a, out, total);
  return cst_check_launch("cst_collate_pairs");
}
