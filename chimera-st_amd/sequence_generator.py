"""Beam-search decoding — mirror of fairseq/sequence_generator.py (SequenceGenerator._generate :179-541,
finalize_hypos :575-696, EnsembleModel.forward_encoder/forward_decoder :800-868) and fairseq/search.py BeamSearch.step
(:109-144), for one model or a checkpoint ensemble (`--path a.pt:b.pt:c.pt`: the members' next-token distributions are
averaged at every step).  Decoder steps run through the incremental-state path of the HIP modules (K/V caches kept
batch-major [B*beam, T, C]; single-query fused attention).  The constraints `no_repeat_ngram_size` (_no_repeat_ngram :734-767) and
`prefix_tokens` (_prefix_tokens :543-575) run inside the beam-step kernel on the engine and as tensor operations on the device
in the host loop (the reference copies the token matrix to the host every step and keys Python dictionaries by strings).

`Sampling` (search.py:621-742: --sampling, --sampling-topk, --sampling-topp) is the one search strategy besides beam search that the
device engine runs (cst_beam_step draws inside its row kernel); its draws are counter-based — a function of (key, sentence, slot,
step), like the dropout masks of rng.py — so the engine and the host loop below draw the same tokens from the same distributions.

`DiverseBeamSearch` (search.py:551-618: --diverse-beam-groups, --diverse-beam-strength) and `DiverseSiblingsSearch` (search.py:745-814:
--diversity-rate) are the two diverse strategies; the engine runs both inside the per-sentence merge kernel of cst_beam_step
(include/cst.h, ABI 12), the classes below are the host loop's form of the same selections.

`LexicallyConstrainedBeamSearch` (search.py:210-523: --constraints [ordered|unordered]) keeps a constraint state per hypothesis
(lexical_constraints.py) and shapes each sentence's candidate list by them; the engine runs it as the third selection rule of the merge
kernel (cst_beam_step_lex), the class below is the host loop's form of the same rule.

Models without an encoder (a `transformer_lm`: EnsembleModel.has_encoder :790-803) are generated from too: the batch size and the source
length of max_len come from `src_tokens` — the prompt batch of tasks.LanguageModelingTask, which hands the prompts over as prefix_tokens —
nothing is encoded or reordered, and the engine runs such members as decoders without a cross block (decode_engine.py).

Differences that do not change results: finished sentences are masked out instead of being removed from the batch
(the reference shrinks the batch, :427-463 — an optimisation only; every sentence's search is independent)."""
import dataclasses
import math
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor

from . import lexical_constraints as LC
from . import rng
from .decode_engine import BeamDecodeEngine, DecodeOptions


class BeamSearch:
    """search.py:100-144."""

    def __init__(self, tgt_dict):
        self.pad, self.unk, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos()
        self.vocab_size = len(tgt_dict)

    def step(self, step: int, lprobs, scores):
        bsz, beam_size, vocab_size = lprobs.size()
        if step == 0:
            lprobs = lprobs[:, ::beam_size, :].contiguous()  # all hypotheses equal at step 0: use the first beam only
        else:
            lprobs = lprobs + scores[:, :, step - 1].unsqueeze(-1)
        top = torch.topk(lprobs.view(bsz, -1), k=min(beam_size * 2, lprobs.view(bsz, -1).size(1) - 1))
        scores_buf, indices_buf = top[0], top[1]
        beams_buf = indices_buf // vocab_size
        indices_buf = indices_buf.fmod(vocab_size)
        return scores_buf, indices_buf, beams_buf


def sample_uniforms(key, idx):
    """The uniforms of the sampling draws, u = (cst_drop_bits32(key, cst_drop_key2(key), idx) >> 8) * 2^-24 in [0, 1) (float64, exact):
    the numpy twin of the device code (csrc/cst_common.h).  idx: integer array, idx = (sentence * beam + slot) * (max_len + 1) + step."""
    key = int(key) & 0xFFFFFFFF
    key2 = (key * 0x2C1B3C6D + 0x297A2D39) & 0xFFFFFFFF
    bits = rng._bits32(key, key2, np.asarray(idx, dtype=np.uint64) & np.uint64(0xFFFFFFFF))
    return (bits >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def sample_key_of(seed, ordinal):
    """The 32-bit key of the `ordinal`-th generate() call of a generator seeded with `seed` (rng.DropoutState.next_key's mixing)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return rng._hash32((seed & 0xFFFFFFFF) ^ rng._hash32(int(ordinal) * 0x9E3779B1 + (seed >> 32)))


class Sampling:
    """search.py:621-742 with counter-based draws.  After the generator's masks, q_v = exp(lprob_v) (not renormalised):
      top-p (sampling_topp > 0, wins): in the order (value descending, token ascending) keep every element with less than p of mass in
            front of it (_sample_topp :630-673: cumsum.lt(p) plus one more element; whole mass < p: everything);
      top-k (sampling_topk > 0): keep the first k of that order;
      draw: the smallest kept token v whose inclusive kept mass in vocabulary order exceeds u * Z (Z = the kept mass), u from
            sample_uniforms(key, (sentence * beam + slot) * (max_len + 1) + step).
    Step 0 draws `beam` tokens from each sentence's first row; later steps one token per row, and row i continues hypothesis i.  The
    score of a draw is its masked log-probability + the row's cumulative score.  A row without mass yields (-inf, pad)."""

    def __init__(self, tgt_dict, sampling_topk=-1, sampling_topp=-1.0):
        self.pad, self.unk, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos()
        self.vocab_size = len(tgt_dict)
        self.sampling_topk, self.sampling_topp = int(sampling_topk), float(sampling_topp)
        if self.sampling_topk > self.vocab_size:
            raise ValueError("sampling_topk %d exceeds the vocabulary (%d symbols)" % (self.sampling_topk, self.vocab_size))

    def kept(self, lprobs):
        """bool [..., V]: the elements the draw chooses among."""
        if self.sampling_topp <= 0 and self.sampling_topk <= 0:
            return torch.ones_like(lprobs, dtype=torch.bool)
        val, order = torch.sort(lprobs, dim=-1, descending=True, stable=True)  # equal values keep their token order
        if self.sampling_topp > 0:
            q = val.exp().double()
            keep = (q.cumsum(-1) - q) < self.sampling_topp
        else:
            keep = torch.arange(lprobs.size(-1), device=lprobs.device).expand_as(val) < self.sampling_topk
        return torch.zeros_like(keep).scatter(-1, order, keep)

    def step(self, step: int, lprobs, scores, key=0, max_len=None):
        """lprobs [bsz, beam, V] after the generator's masks, scores [bsz, beam, >= step] cumulative; key: the call's 32-bit key;
        max_len: the generator's step limit (part of the draw index).  Returns `beam` candidates per sentence."""
        bsz, beam_size, V = lprobs.size()
        assert max_len is not None, "Sampling.step needs the generator's max_len: it is part of the index of a draw"
        if step == 0:
            lprobs = lprobs[:, ::beam_size, :]  # the first row of every sentence serves all its slots
        q = torch.where(self.kept(lprobs), lprobs.exp(), torch.zeros_like(lprobs)).double()
        cdf = q.cumsum(-1)
        Z = cdf[..., -1:]
        slot = np.arange(bsz * beam_size, dtype=np.int64) * (max_len + 1) + step
        u = torch.from_numpy(sample_uniforms(key, slot)).to(lprobs.device).view(bsz, beam_size, 1)
        if step == 0:
            q, cdf, lprobs = (t.expand(bsz, beam_size, V) for t in (q, cdf, lprobs))
        ids = torch.arange(V, device=lprobs.device).expand(bsz, beam_size, V)
        hit = (cdf > u * Z) & (q > 0)
        tok = torch.where(hit, ids, torch.full_like(ids, V)).amin(-1)
        last = torch.where(q > 0, ids, torch.full_like(ids, -1)).amax(-1)  # (rounding at the top of the CDF: the last kept token)
        tok = torch.where(tok == V, last, tok)
        none = tok < 0
        tok = torch.where(none, torch.full_like(tok, self.pad), tok)
        scores_buf = lprobs.gather(2, tok.unsqueeze(-1)).squeeze(-1)
        scores_buf = torch.where(none, torch.full_like(scores_buf, -math.inf), scores_buf)
        if step == 0:
            beams_buf = torch.zeros_like(tok)
        else:
            beams_buf = torch.arange(beam_size, device=tok.device).repeat(bsz, 1)
            scores_buf = scores_buf + scores[:, :, step - 1]
        return scores_buf, tok, beams_buf


class DiverseBeamSearch:
    """search.py:551-618, Hamming diversity.  The `beam` rows of a sentence are dealt to `num_groups` groups (group g: rows g, g + G,
    ...).  The groups search one after the other, each a beam search of width beam / G over its own rows, and every token loses
    diversity_strength per candidate that an earlier group selected with that token at this step (all 2 * beam / G candidates of a group
    count, whatever their value).  The groups' candidate lists are interleaved: the j-th candidate of group g is the sentence's
    candidate j * G + g, its parent row local_row * G + g.  The penalised value is the score a hypothesis carries on."""

    def __init__(self, tgt_dict, num_groups, diversity_strength):
        self.pad, self.unk, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos()
        self.vocab_size = len(tgt_dict)
        self.num_groups, self.diversity_strength = int(num_groups), float(diversity_strength)
        if self.num_groups < 1:
            raise ValueError("DiverseBeamSearch needs at least one group, got %d" % self.num_groups)
        self.beam = BeamSearch(tgt_dict)

    def step(self, step: int, lprobs, scores):
        bsz, beam_size, V = lprobs.size()
        G = self.num_groups
        if beam_size % G != 0:
            raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups")
        counts = torch.zeros(bsz, V, dtype=lprobs.dtype, device=lprobs.device)  # selections of the earlier groups, per token
        out = []
        for g in range(G):
            lp = lprobs[:, g::G, :]
            if g > 0:
                lp = torch.add(lp, counts.unsqueeze(1), alpha=-self.diversity_strength)
            sc, tok, parent = self.beam.step(step, lp, scores[:, g::G, :] if step > 0 else None)
            out.append((sc, tok, parent * G + g))
            counts.scatter_add_(1, tok, torch.ones_like(sc))
        return tuple(torch.stack([o[i] for o in out], dim=2).view(bsz, -1) for i in range(3))


class DiverseSiblingsSearch:
    """search.py:745-814.  Step 0 is plain beam search.  Later every row lists its own best 2 * beam continuations (cumulative score
    added), the one at position p (from 0) loses (p + 1) * diversity_rate, and the sentence's best 2 * beam of the beam * 2 * beam
    penalised values are its candidates: the siblings of one hypothesis compete on unequal terms.  Rate 0 is plain beam search."""

    def __init__(self, tgt_dict, diversity_rate):
        self.pad, self.unk, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos()
        self.vocab_size = len(tgt_dict)
        self.diversity_rate = float(diversity_rate)
        self.beam = BeamSearch(tgt_dict)

    def step(self, step: int, lprobs, scores):
        if step == 0:
            return self.beam.step(step, lprobs, scores)
        bsz, beam_size, V = lprobs.size()
        k = min(2 * beam_size, beam_size * V - 1)
        val, tok = torch.topk(lprobs + scores[:, :, step - 1].unsqueeze(-1), k, dim=2)          # [bsz, beam, k], sorted
        val = val - torch.arange(1, k + 1, device=val.device).to(val) * self.diversity_rate
        scores_buf, pick = torch.topk(val.view(bsz, -1), k)
        return scores_buf, tok.view(bsz, -1).gather(1, pick), pick // k


class LexicallyConstrainedBeamSearch:
    """search.py:210-523.  Every hypothesis carries a constraint state (lexical_constraints.py).  One step of one sentence:
      1. eos ban: at step > 0 a row whose state is not finished gets lp[eos] = -inf (after the generator's masks, before the cumulative
         score is added);
      2. the list L: the sentence's plain top 2*beam; at step > 0 every row's own best candidate, in row order; per row in row order
         (only the first row at step 0) one candidate per next token of the row's state, in ascending token order, value lp + score;
      3. per candidate bank = the bank of its parent's state advanced by its token, and the fp32 key = float((nd - bank) * -100) + value,
         nd = the sentence's number of distinct constraint tokens; L is sorted by the key, descending, stably;
      4. a candidate whose predecessor in that order (cyclically: the first looks at the last) has the same (parent, token) is dropped;
      5. the j-th survivor of a run of equal banks gets the stripe nd - bank + j * (survivors + 1); a stable ascending sort by stripe
         deals the banks round-robin; the first 2*beam are the sentence's candidates, each with its advanced state.
    update_constraints(active_hypos) then hands next row i the state of candidate active_hypos[i]."""

    def __init__(self, tgt_dict, representation):
        self.pad, self.unk, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos()
        self.vocab_size = len(tgt_dict)
        if representation not in LC.REPRESENTATIONS:
            raise ValueError("constraint representation %r (ordered | unordered)" % (representation,))
        self.representation = representation
        self.constraint_states = []
        self.supports_constraints = True

    def init_constraints(self, batch_constraints, beam_size):
        """batch_constraints: the packed int64 [bsz, W] (lexical_constraints.pack_constraints)."""
        self.constraint_states = []
        for row in batch_constraints.tolist():
            state = LC.create_state(self.representation, row)
            self.constraint_states.append([state] * beam_size)  # (states are immutable values)

    def update_constraints(self, active_hypos):
        for sent, act in enumerate(active_hypos.tolist()):
            self.constraint_states[sent] = [self.constraint_states[sent][i] for i in act]

    def step(self, step: int, lprobs, scores):
        bsz, beam_size, V = lprobs.size()
        K = min(2 * beam_size, beam_size * V - 1)
        states = self.constraint_states
        if not states:  # no constraints were given to this call: plain beam search (search.py:341-343)
            return BeamSearch.step(self, step, lprobs, scores)
        assert len(states) == bsz, "init_constraints() was given another batch"
        if step > 0:
            ban = torch.tensor([[not st.finished for st in sent] for sent in states], device=lprobs.device)
            lprobs = lprobs.clone()
            lprobs[:, :, self.eos] = lprobs[:, :, self.eos].masked_fill(ban, -math.inf)
        if step == 0:
            lprobs = lprobs[:, ::beam_size, :].contiguous()
        else:
            lprobs = lprobs + scores[:, :, step - 1].unsqueeze(-1)
        flat = lprobs.view(bsz, -1)
        order = torch.sort(flat, dim=1, descending=True, stable=True)[1][:, :K]  # equal values keep their flat-index order
        top_val, top_tok, top_par = torch.gather(flat, 1, order).tolist(), (order % V).tolist(), (order // V).tolist()
        if step > 0:  # every row's best, ties to the smaller token
            best = lprobs.amax(dim=2, keepdim=True)
            ids = torch.arange(V, device=lprobs.device).expand_as(lprobs)
            best_tok = torch.where(lprobs == best, ids, torch.full_like(ids, V)).amin(dim=2).tolist()
            best_val = best.squeeze(2).tolist()
        host = lprobs.cpu()
        out_val, out_tok, out_par = [], [], []
        for b in range(bsz):
            cand = list(zip(top_val[b], top_tok[b], top_par[b]))
            if step > 0:
                cand += [(best_val[b][r], best_tok[b][r], r) for r in range(beam_size)]
            for r in range(1 if step == 0 else beam_size):
                cand += [(float(host[b, r, t]), t, r) for t in states[b][r].next_tokens()]
            val, tok, par, new_states = self._select(cand, states[b], K)
            states[b] = new_states
            out_val.append(val), out_tok.append(tok), out_par.append(par)
        dev = lprobs.device
        return (torch.tensor(out_val, dtype=torch.float32, device=dev), torch.tensor(out_tok, dtype=torch.long, device=dev),
                torch.tensor(out_par, dtype=torch.long, device=dev))

    @staticmethod
    def _select(cand, states, K):
        """Rules 3-5 over the list `cand` of (value, token, parent) of one sentence; states: its rows' states."""
        nd = states[0].num_distinct
        adv = [states[p].advance(t) for _, t, p in cand]
        value = np.array([v for v, _, _ in cand], dtype=np.float32)
        bank = np.array([a.bank for a in adv], dtype=np.int64)
        with np.errstate(invalid="ignore"):
            key = ((nd - bank) * -100).astype(np.float32) + value
        order = sorted(range(len(cand)), key=lambda i: -key[i])  # (sorted() is stable; -(-inf) = inf sorts last)
        pair = [cand[i][1:] for i in order]
        keep = [i for q, i in enumerate(order) if pair[q] != pair[q - 1]]  # (q = 0 looks at the last one)
        stripes, run = [], 0
        for q, i in enumerate(keep):
            run = run + 1 if q > 0 and bank[i] == bank[keep[q - 1]] else 0
            stripes.append(nd - int(bank[i]) + run * (len(keep) + 1))
        chosen = [keep[q] for q in sorted(range(len(keep)), key=lambda q: stripes[q])][:K]
        return ([cand[i][0] for i in chosen], [cand[i][1] for i in chosen], [cand[i][2] for i in chosen], [adv[i] for i in chosen])


class SequenceGenerator:
    def __init__(self, models, tgt_dict, beam_size=1, max_len_a=0, max_len_b=200, min_len=1, normalize_scores=True,
                 len_penalty=1.0, unk_penalty=0.0, temperature=1.0, match_source_len=False, no_repeat_ngram_size=0,
                 search_strategy=None, eos=None, fused=True, use_graph=True, cross_kernel=None, seed=1, lm_model=None, lm_weight=1.0,
                 return_attention=False):
        self.models = list(models) if isinstance(models, (list, tuple)) else [models]
        self.model = self.models[0]
        self.tgt_dict = tgt_dict
        for i, m in enumerate(self.models):  # the members' distributions are averaged token by token: one target vocabulary
            n = getattr(getattr(m.decoder, "embed_tokens", None), "num_embeddings", len(tgt_dict))
            if n != len(tgt_dict):
                raise ValueError("ensemble member %d has a target vocabulary of %d symbols, the dictionary has %d: the members of an "
                                 "ensemble must share the target dictionary" % (i, n, len(tgt_dict)))
        # decoder-only members (sequence_generator.py:790-803 has_encoder): language models, decoded from prompts given as prefix_tokens
        n_enc = sum(1 for m in self.models if getattr(m, "encoder", None) is not None)
        if n_enc not in (0, len(self.models)):
            raise ValueError("an ensemble mixes %d encoder-decoder models with %d decoder-only language models: the members must be "
                             "of one kind" % (n_enc, len(self.models) - n_enc))
        self.has_encoder = n_enc > 0
        if not self.has_encoder and lm_model is not None:
            raise ValueError("shallow fusion (lm_model, --lm-path) into a model that is itself a language model is not built: decode "
                             "the two as an ensemble (--path a.pt:b.pt)")
        if not self.has_encoder and return_attention:
            raise ValueError("return_attention (--print-alignment) needs cross attention: a decoder-only language model has none")
        self.pad, self.unk = tgt_dict.pad(), tgt_dict.unk()
        self.eos = tgt_dict.eos() if eos is None else eos
        self.vocab_size = len(tgt_dict)
        self.beam_size = min(beam_size, self.vocab_size - 1)
        self.max_len_a, self.max_len_b, self.min_len = max_len_a, max_len_b, min_len
        self.normalize_scores, self.len_penalty, self.unk_penalty = normalize_scores, len_penalty, unk_penalty
        self.temperature = temperature
        # return_attention (--print-alignment): every hypothesis' "attention" is the fp32 [src_len, tgt_len] matrix of the reference
        # (sequence_generator.py:349-355, :523-526, :609-611, :664-674): per emitted token the LAST decoder layer's cross attention,
        # averaged over the heads and over the members of an ensemble.  Off: "attention" is None and nothing is computed for it.
        self.return_attention = bool(return_attention)
        # shallow fusion (sequence_generator.py:36-37, :103-106, :318-324): lm_weight x the LM's next-token log-softmax (no temperature)
        # is added to the models' log-probabilities at every step, before any mask
        self.lm_model, self.lm_weight = lm_model, float(lm_weight)
        if lm_model is not None:
            n = getattr(getattr(lm_model.decoder, "embed_tokens", None), "num_embeddings", len(tgt_dict))
            if n != len(tgt_dict):
                raise ValueError("the language model has a vocabulary of %d symbols, the target dictionary has %d: the LM's dictionary "
                                 "must be the target dictionary" % (n, len(tgt_dict)))
            if not math.isfinite(self.lm_weight):
                raise ValueError("lm_weight must be finite, got %r" % lm_weight)
            lm_model.eval()
        assert temperature > 0 and not match_source_len
        if no_repeat_ngram_size < 0 or no_repeat_ngram_size == 1:
            raise ValueError("no_repeat_ngram_size must be 0 (off) or at least 2, got %d: with 1 the initial eos of every hypothesis is "
                             "itself a banned 1-gram, so eos can never be emitted and no hypothesis can finish (the reference dies "
                             "with a bare AssertionError there)" % no_repeat_ngram_size)
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)
        self.search = BeamSearch(tgt_dict) if search_strategy is None else search_strategy
        # fused=True (default): the device-resident loop of decode_engine.py (one captured HIP graph per step, no per-step host
        # sync); fused=False: the module-by-module mirror of the reference loop below (same kernels, host-driven) — kept as the
        # readable restatement and as the cross-check of the engine.  A custom search strategy needs the host loop — except Sampling,
        # DiverseBeamSearch and DiverseSiblingsSearch (exactly those classes: a subclass may select differently), which cst_beam_step
        # runs itself.
        self.sampling = isinstance(self.search, Sampling)  # (the host loop hands key and max_len to any Sampling, a subclass included)
        # `strategy`: the strategy as engine options; None = it needs the host loop.  (A negative strength or rate is a reward: the
        # reference accepts it, cst_beam_step does not — a reward can lift tokens from outside the rows' top 2 * beam lists or unsort
        # them — so such a search takes the host loop.)
        kind, s, strategy = type(self.search), self.search, None
        if search_strategy is None:
            strategy = {}
        elif kind is Sampling:
            strategy = dict(sampling=True, topk=s.sampling_topk, topp=s.sampling_topp)
        elif kind is DiverseBeamSearch and s.diversity_strength >= 0:
            strategy = dict(diverse_groups=s.num_groups, diverse_strength=s.diversity_strength)
        elif kind is DiverseSiblingsSearch and s.diversity_rate >= 0:
            strategy = dict(sibling_rate=s.diversity_rate)
        elif kind is LexicallyConstrainedBeamSearch:  # (not an option of cst_beam_desc: the engine's `lexical` keyword)
            strategy = {}
        # lexical constraints: the representation; a call hands the constraints themselves to generate()
        self.lexical = s.representation if isinstance(s, LexicallyConstrainedBeamSearch) else None
        self.fused = bool(fused) and strategy is not None and (eos is None or eos == tgt_dict.eos())
        if isinstance(self.search, DiverseBeamSearch) and self.beam_size % self.search.num_groups != 0:
            raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups (beam %d, %d groups)"
                             % (self.beam_size, self.search.num_groups))
        # the engine's options but for max_len, which a call's source length decides
        self.options = DecodeOptions(self.beam_size, 0, min_len, normalize_scores, len_penalty, unk_penalty, temperature,
                                     self.no_repeat_ngram_size, lm_weight=self.lm_weight, **strategy) if self.fused else None
        # sampling: the key of a call's draws = hash of (seed, the call's ordinal in this generator)
        self.seed, self.calls = int(seed), 0
        self._engine = None
        self.use_graph, self.cross_kernel = use_graph, cross_kernel
        for m in self.models:
            m.eval()

    @torch.no_grad()
    def generate(self, models, sample, prefix_tokens=None, sample_key=None, constraints=None, bos_token=None, **kwargs):
        """sample_key: the 32-bit key of this call's draws (sampling only); default: the next key of the generator's own stream.
        constraints: the packed lexical constraints of the batch, int64 [bsz, W] (lexical_constraints.pack_constraints); needs a
        LexicallyConstrainedBeamSearch as the search strategy.  None: the search without them.
        bos_token: the token every hypothesis starts from (sequence_generator.py:256); only eos, what the kernels start from, is built."""
        if bos_token is not None and int(bos_token) != self.eos:
            raise NotImplementedError("bos_token %d: hypotheses start from eos (%d); --add-bos-token is not built" % (int(bos_token), self.eos))
        return self._generate(sample, prefix_tokens=prefix_tokens, sample_key=sample_key, constraints=constraints)

    def _check_constraints(self, constraints, prefix_tokens, bsz):
        if self.lexical is None:
            raise ValueError("constraints need a LexicallyConstrainedBeamSearch as the search strategy (--constraints)")
        if prefix_tokens is not None:  # (the reference copies the first beam's rows at a prefix eos, but not its constraint states)
            raise ValueError("lexical constraints cannot be combined with prefix_tokens (--prefix-size)")
        constraints = torch.as_tensor(constraints).to(device="cpu", dtype=torch.long)
        if constraints.dim() != 2 or constraints.size(0) != bsz:
            raise ValueError("constraints must be the packed [batch %d, width] tensor, got %s" % (bsz, tuple(constraints.shape)))
        for row in constraints.tolist():  # the packed layout itself: 0 terminates, pad and eos cannot be asked for
            LC.pack_constraints([LC.unpack_constraints(row)], pad=self.pad, eos=self.eos)
        return constraints

    @staticmethod
    def _unmet(finalized):
        missing = [b for b, hyps in enumerate(finalized) if not hyps]
        if missing:
            raise RuntimeError("lexical constraints not met within max_len: sentences %s" % missing)

    def _check_prefix(self, prefix_tokens, bsz, max_len):
        if prefix_tokens.dim() != 2 or prefix_tokens.size(0) != bsz:
            raise ValueError("prefix_tokens must be [batch %d, width], got %s" % (bsz, tuple(prefix_tokens.shape)))
        if prefix_tokens.size(1) > max_len:
            raise ValueError("prefix_tokens is %d tokens wide, the step limit max_len is %d" % (prefix_tokens.size(1), max_len))
        first = prefix_tokens[:, 0]
        if bool((first.eq(self.eos) | first.eq(self.pad)).any()):
            raise ValueError("a row of prefix_tokens starts with eos or pad: every sentence needs at least one real prefix token")

    def _ban_repeated_ngrams(self, tokens, lprobs, step):
        """_no_repeat_ngram (:734-767) as tensor operations: with last = tokens[:, step+2-n : step+1], every window
        tokens[:, i : i+n-1] (i <= step+1-n) equal to it makes tokens[:, i+n-1] -inf.  (The reference also scans the pad tail of the
        buffer; for n >= 2 that only ever bans pad.)"""
        n = self.no_repeat_ngram_size
        if step + 1 - n < 0:
            return lprobs
        last = tokens[:, step + 2 - n:step + 1]
        windows = tokens[:, :step].unfold(1, n - 1, 1)                       # [rows, step+2-n, n-1]
        match = windows.eq(last.unsqueeze(1)).all(dim=-1)
        follow = tokens[:, n - 1:step + 1]                                   # the token after each window
        zero = torch.zeros((), dtype=lprobs.dtype, device=lprobs.device)
        return lprobs.scatter_add(1, follow, torch.where(match, zero - math.inf, zero))  # x + 0 = x; x + -inf = -inf in any order

    def _force_prefix(self, step, lprobs, scores, tokens, prefix_tokens, beam_size):
        """_prefix_tokens (:543-575): rows whose prefix token t is not pad keep only t; where t is eos, the sentence's first beam is
        copied over its other beams (tokens, scores, lprobs)."""
        t = prefix_tokens[:, step].repeat_interleave(beam_size).unsqueeze(1)
        only_t = torch.full_like(lprobs, -math.inf).scatter(1, t, lprobs.gather(1, t))
        lprobs = torch.where(t.ne(self.pad), only_t, lprobs)
        rows = torch.arange(lprobs.size(0), device=lprobs.device)
        src = torch.where(t.squeeze(1).eq(self.eos), rows - rows % beam_size, rows)
        return lprobs[src], tokens[src], scores[src]

    def _forward_decoder(self, tokens, encoder_outs, incremental_states):
        """sequence_generator.py:806-868: per member the last-step logits / temperature -> fp32 log-softmax; an ensemble averages the
        members' DISTRIBUTIONS: logsumexp over the members - log N (:862-864).  Returns (lprobs, attention): attention is None, or with
        return_attention the members' last-layer head-averaged cross attention of this step, fp32 [rows, S], summed / N (:829-868)."""
        log_probs, avg_attn = [], None
        for model, encoder_out, incremental_state in zip(self.models, encoder_outs, incremental_states):
            last = len(model.decoder.layers) - 1 if self.return_attention else None
            logits, extra = model.decoder.forward(tokens, encoder_out=encoder_out, incremental_state=incremental_state, alignment_layer=last)
            if self.return_attention:
                a = extra["attn"][0][:, -1, :]
                if avg_attn is not None and avg_attn.shape != a.shape:
                    raise ValueError("attention of an ensemble needs members of one encoder length, got %d and %d" % (avg_attn.size(1), a.size(1)))
                avg_attn = a if avg_attn is None else avg_attn + a
            logits = logits[:, -1:, :]
            if self.temperature != 1.0:
                logits = logits / self.temperature
            log_probs.append(model.get_normalized_probs((logits, None), log_probs=True)[:, -1, :])
        if len(log_probs) == 1:
            return log_probs[0], avg_attn
        if avg_attn is not None:
            avg_attn = avg_attn / len(log_probs)
        return torch.logsumexp(torch.stack(log_probs, dim=0), dim=0) - math.log(len(log_probs)), avg_attn

    def _lm_lprobs(self, tokens, incremental_state):
        """sequence_generator.py:318-324: lm_weight x the LM's log-softmax at the last position (the reference recomputes the whole
        prefix at every step; the incremental state gives the same numbers)."""
        out = self.lm_model.decoder.forward(tokens, incremental_state=incremental_state)
        probs = self.lm_model.get_normalized_probs((out[0][:, -1:, :], None), log_probs=True)[:, -1, :]
        return probs * self.lm_weight

    def _generate(self, sample, prefix_tokens=None, sample_key=None, constraints=None):
        self.calls += 1
        key = (sample_key_of(self.seed, self.calls) if sample_key is None else int(sample_key) & 0xFFFFFFFF) if self.sampling else 0
        net_input = sample["net_input"]
        src_tokens = net_input["src_tokens"]
        bsz, src_len = src_tokens.size()[:2]
        beam_size = self.beam_size
        device = src_tokens.device
        max_len = min(int(self.max_len_a * src_len + self.max_len_b), min(m.max_decoder_positions() for m in self.models) - 1)  # :796-797
        assert self.min_len <= max_len
        if prefix_tokens is not None:
            prefix_tokens = prefix_tokens.to(device=device, dtype=torch.long)
            self._check_prefix(prefix_tokens, bsz, max_len)
            if prefix_tokens.size(1) == 0:
                prefix_tokens = None
        if constraints is not None:
            if not self.has_encoder:  # (language_modeling.py:301-304)
                raise NotImplementedError("constrained decoding with a decoder-only language model is not supported")
            constraints = self._check_constraints(constraints, prefix_tokens, bsz)
        # decoder-only members (:801-803, :883-884): bsz and src_len are the prompt batch's, there is nothing to encode or to reorder
        encoder_outs = [m.encoder.forward_torchscript(net_input) for m in self.models] if self.has_encoder else None
        if self.fused:
            member_ok = BeamDecodeEngine.supported if self.has_encoder else BeamDecodeEngine.lm_supported
            ok = len(self.models) <= 8 and all(member_ok(m.decoder) for m in self.models)  # else the whole ensemble takes the host loop
            if self.lm_model is not None:  # (an LM the engine cannot take sends the whole decode to the host loop)
                ok = ok and BeamDecodeEngine.lm_supported(self.lm_model.decoder)
            if self.sampling:  # (the wide-vocabulary row kernel only selects: such vocabularies are sampled by the host loop)
                store = encoder_outs[0].encoder_out.dtype if self.has_encoder else self.model.decoder.embed_tokens.weight.dtype
                ok = ok and BeamDecodeEngine.sampling_supported(self.vocab_size, store)
            if constraints is not None:  # (more constraint tokens or next tokens than cst_lex_init holds: the host loop)
                ok = ok and BeamDecodeEngine.lexical_supported(constraints, beam_size)
            if ok:
                if self._engine is None or self._engine.opt.max_len != max_len:
                    self._engine = BeamDecodeEngine([m.decoder for m in self.models], self.tgt_dict,
                                                    dataclasses.replace(self.options, max_len=max_len),
                                                    lm_decoder=None if self.lm_model is None else self.lm_model.decoder,
                                                    use_graph=self.use_graph, cross_kernel=self.cross_kernel, lexical=self.lexical,
                                                    attention=self.return_attention)
                return self._engine.generate(encoder_outs, bsz, prefix_tokens=prefix_tokens, sample_key=key, constraints=constraints)
        if self.lexical is not None:  # (sequence_generator.py:216-222; without constraints the strategy steps like BeamSearch)
            self.search.constraint_states = []
            if constraints is not None:
                self.search.init_constraints(constraints, beam_size)
        if self.has_encoder:
            new_order = torch.arange(bsz, device=device).view(-1, 1).repeat(1, beam_size).view(-1)
            encoder_outs = [m.encoder.reorder_encoder_out(e, new_order) for m, e in zip(self.models, encoder_outs)]
        else:
            encoder_outs = [None] * len(self.models)
        incremental_states: List[Dict[str, Dict[str, Optional[Tensor]]]] = [{} for _ in self.models]
        lm_state: Dict[str, Dict[str, Optional[Tensor]]] = {}

        scores = torch.zeros(bsz * beam_size, max_len + 1, device=device, dtype=torch.float32)
        tokens = torch.full((bsz * beam_size, max_len + 2), self.pad, device=device, dtype=torch.long)
        tokens[:, 0] = self.eos
        cands_to_ignore = torch.zeros(bsz, beam_size, device=device).eq(-1)
        finalized: List[List[Dict[str, Tensor]]] = [[] for _ in range(bsz)]
        finished = [False] * bsz
        num_remaining = bsz
        cand_size = 2 * beam_size
        bbsz_offsets = (torch.arange(0, bsz, device=device) * beam_size).unsqueeze(1)
        cand_offsets = torch.arange(0, cand_size, device=device)
        reorder_state = None
        attn = None  # return_attention: [bbsz, S, max_len + 2], column step + 1 written at `step`, reordered with the tokens (:349-355)

        for step in range(max_len + 1):
            if reorder_state is not None:
                for m, inc in zip(self.models, incremental_states):
                    m.decoder.reorder_incremental_state_scripting(inc, reorder_state)
                if self.has_encoder:
                    encoder_outs = [m.encoder.reorder_encoder_out(e, reorder_state) for m, e in zip(self.models, encoder_outs)]
                if self.lm_model is not None:
                    self.lm_model.decoder.reorder_incremental_state_scripting(lm_state, reorder_state)
            lprobs, avg_attn = self._forward_decoder(tokens[:, :step + 1], encoder_outs, incremental_states)
            if avg_attn is not None:
                if attn is None:
                    attn = torch.zeros(bsz * beam_size, avg_attn.size(1), max_len + 2, device=device, dtype=torch.float32)
                attn[:, :, step + 1].copy_(avg_attn)
            if self.lm_model is not None:
                lprobs = lprobs + self._lm_lprobs(tokens[:, :step + 1], lm_state)
            lprobs[lprobs != lprobs] = -math.inf
            lprobs[:, self.pad] = -math.inf
            lprobs[:, self.unk] -= self.unk_penalty
            if step >= max_len:
                lprobs[:, :self.eos] = -math.inf
                lprobs[:, self.eos + 1:] = -math.inf
            if prefix_tokens is not None and step < prefix_tokens.size(1) and step < max_len:
                lprobs, tokens, scores = self._force_prefix(step, lprobs, scores, tokens, prefix_tokens, beam_size)
            elif step < self.min_len:  # (not at a prefix step of the batch)
                lprobs[:, self.eos] = -math.inf
            if self.no_repeat_ngram_size > 0:
                lprobs = self._ban_repeated_ngrams(tokens, lprobs, step)
            extra = dict(key=key, max_len=max_len) if self.sampling else {}  # (Sampling returns beam candidates per sentence, not 2 * beam)
            cand_scores, cand_indices, cand_beams = self.search.step(
                step, lprobs.view(bsz, -1, self.vocab_size), scores.view(bsz, beam_size, -1)[:, :, :step], **extra)
            cand_bbsz_idx = cand_beams.add(bbsz_offsets)
            eos_mask = cand_indices.eq(self.eos) & cand_scores.ne(-math.inf)
            eos_mask[:, :beam_size][cands_to_ignore] = False
            # finalize hypotheses whose eos is among the top beam_size candidates (:385-416)
            top_eos = eos_mask[:, :beam_size]
            if top_eos.any():
                for sent, col in top_eos.nonzero(as_tuple=False).tolist():
                    if finished[sent] or len(finalized[sent]) >= beam_size:
                        continue
                    bi = int(cand_bbsz_idx[sent, col])
                    sc = cand_scores[sent, col].clone()
                    toks = tokens[bi, 1:step + 2].clone()
                    toks[step] = self.eos
                    pos = scores[bi, :step + 1].clone()
                    pos[step] = sc
                    pos[1:] = pos[1:] - pos[:-1].clone()
                    if self.normalize_scores:
                        sc = sc / (step + 1) ** self.len_penalty
                    finalized[sent].append({"tokens": toks, "score": sc, "attention": None if attn is None else attn[bi, :, 1:step + 2].clone(),
                                            "alignment": None, "positional_scores": pos})
                for sent in set(s for s, _ in top_eos.nonzero(as_tuple=False).tolist()):
                    if not finished[sent] and (len(finalized[sent]) == beam_size or step == max_len):
                        finished[sent] = True
                        num_remaining -= 1
            if num_remaining == 0 or step >= max_len:
                break
            # choose the first beam_size non-eos candidates as the next active hypotheses (:465-499)
            eos_mask[:, :beam_size] = ~((~cands_to_ignore) & (~eos_mask[:, :beam_size]))
            active_mask = eos_mask.type_as(cand_offsets) * cand_size + cand_offsets[:eos_mask.size(1)]
            new_cands_to_ignore, active_hypos = torch.topk(active_mask, k=beam_size, dim=1, largest=False)
            cands_to_ignore = new_cands_to_ignore.ge(cand_size)[:, :beam_size]
            if constraints is not None:  # next row i carries the state of its candidate (:519-520)
                self.search.update_constraints(active_hypos)
            active_bbsz_idx = torch.gather(cand_bbsz_idx, dim=1, index=active_hypos).view(-1)
            tokens[:, :step + 1] = torch.index_select(tokens[:, :step + 1], dim=0, index=active_bbsz_idx)
            tokens.view(bsz, beam_size, -1)[:, :, step + 1] = torch.gather(cand_indices, dim=1, index=active_hypos)
            if step > 0:
                scores[:, :step] = torch.index_select(scores[:, :step], dim=0, index=active_bbsz_idx)
            scores.view(bsz, beam_size, -1)[:, :, step] = torch.gather(cand_scores, dim=1, index=active_hypos)
            if attn is not None:
                attn[:, :, :step + 2] = torch.index_select(attn[:, :, :step + 2], dim=0, index=active_bbsz_idx)
            reorder_state = active_bbsz_idx

        if constraints is not None:  # (the reference dies in `assert step < max_len` there)
            self._unmet(finalized)
        for sent in range(bsz):
            sc = torch.tensor([float(h["score"]) for h in finalized[sent]])
            _, order = torch.sort(sc, descending=True)
            finalized[sent] = [finalized[sent][i] for i in order.tolist()]
        return finalized
