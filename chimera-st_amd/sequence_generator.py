"""Beam-search decoding — mirror of fairseq/sequence_generator.py (SequenceGenerator._generate :179-541,
finalize_hypos :575-696, EnsembleModel.forward_encoder/forward_decoder :800-868) and fairseq/search.py BeamSearch.step
(:109-144), for one model or a checkpoint ensemble (`--path a.pt:b.pt:c.pt`: the members' next-token distributions are
averaged at every step).  Decoder steps run through the incremental-state path of the HIP modules (K/V caches kept
batch-major [B*beam, T, C]; single-query fused attention).  The constraints `no_repeat_ngram_size` (_no_repeat_ngram :734-767) and
`prefix_tokens` (_prefix_tokens :543-575) run inside the beam-step kernel on the engine and as tensor operations on the device
in the host loop (the reference copies the token matrix to the host every step and keys Python dictionaries by strings).

Differences that do not change results: finished sentences are masked out instead of being removed from the batch
(the reference shrinks the batch, :427-463 — an optimisation only; every sentence's search is independent)."""
import math
from typing import Dict, List, Optional

import torch
from torch import Tensor


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


class SequenceGenerator:
    def __init__(self, models, tgt_dict, beam_size=1, max_len_a=0, max_len_b=200, min_len=1, normalize_scores=True,
                 len_penalty=1.0, unk_penalty=0.0, temperature=1.0, match_source_len=False, no_repeat_ngram_size=0,
                 search_strategy=None, eos=None, fused=True, use_graph=True, cross_kernel=None):
        self.models = list(models) if isinstance(models, (list, tuple)) else [models]
        self.model = self.models[0]
        self.tgt_dict = tgt_dict
        for i, m in enumerate(self.models):  # the members' distributions are averaged token by token: one target vocabulary
            n = getattr(getattr(m.decoder, "embed_tokens", None), "num_embeddings", len(tgt_dict))
            if n != len(tgt_dict):
                raise ValueError("ensemble member %d has a target vocabulary of %d symbols, the dictionary has %d: the members of an "
                                 "ensemble must share the target dictionary" % (i, n, len(tgt_dict)))
        self.pad, self.unk = tgt_dict.pad(), tgt_dict.unk()
        self.eos = tgt_dict.eos() if eos is None else eos
        self.vocab_size = len(tgt_dict)
        self.beam_size = min(beam_size, self.vocab_size - 1)
        self.max_len_a, self.max_len_b, self.min_len = max_len_a, max_len_b, min_len
        self.normalize_scores, self.len_penalty, self.unk_penalty = normalize_scores, len_penalty, unk_penalty
        self.temperature = temperature
        assert temperature > 0 and not match_source_len
        if no_repeat_ngram_size < 0 or no_repeat_ngram_size == 1:
            raise ValueError("no_repeat_ngram_size must be 0 (off) or at least 2, got %d: with 1 the initial eos of every hypothesis is "
                             "itself a banned 1-gram, so eos can never be emitted and no hypothesis can finish (the reference dies "
                             "with a bare AssertionError there)" % no_repeat_ngram_size)
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)
        self.search = BeamSearch(tgt_dict) if search_strategy is None else search_strategy
        # fused=True (default): the device-resident loop of decode_engine.py (one captured HIP graph per step, no per-step host
        # sync); fused=False: the module-by-module mirror of the reference loop below (same kernels, host-driven) — kept as the
        # readable restatement and as the cross-check of the engine.  A custom search strategy needs the host loop.
        self.fused = bool(fused) and search_strategy is None and (eos is None or eos == tgt_dict.eos())
        self._engine = None
        self.use_graph, self.cross_kernel = use_graph, cross_kernel
        for m in self.models:
            m.eval()

    @torch.no_grad()
    def generate(self, models, sample, prefix_tokens=None, **kwargs):
        return self._generate(sample, prefix_tokens=prefix_tokens)

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
        members' DISTRIBUTIONS: logsumexp over the members - log N (:862-864)."""
        log_probs = []
        for model, encoder_out, incremental_state in zip(self.models, encoder_outs, incremental_states):
            logits, _ = model.decoder.forward(tokens, encoder_out=encoder_out, incremental_state=incremental_state)
            logits = logits[:, -1:, :]
            if self.temperature != 1.0:
                logits = logits / self.temperature
            log_probs.append(model.get_normalized_probs((logits, None), log_probs=True)[:, -1, :])
        if len(log_probs) == 1:
            return log_probs[0]
        return torch.logsumexp(torch.stack(log_probs, dim=0), dim=0) - math.log(len(log_probs))

    def _generate(self, sample, prefix_tokens=None):
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
        encoder_outs = [m.encoder.forward_torchscript(net_input) for m in self.models]
        if self.fused:
            from .decode_engine import BeamDecodeEngine
            if len(self.models) <= 8 and all(BeamDecodeEngine.supported(m.decoder) for m in self.models):  # else the whole ensemble takes the host loop
                if self._engine is None or self._engine.max_len != max_len:
                    decs = [m.decoder for m in self.models]
                    self._engine = BeamDecodeEngine(decs if len(decs) > 1 else decs[0], self.tgt_dict, beam_size, max_len, self.min_len,
                                                    self.normalize_scores, self.len_penalty, self.unk_penalty, self.temperature,
                                                    use_graph=self.use_graph, cross_kernel=self.cross_kernel,
                                                    no_repeat_ngram_size=self.no_repeat_ngram_size)
                return self._engine.generate(encoder_outs if len(encoder_outs) > 1 else encoder_outs[0], bsz, prefix_tokens=prefix_tokens)
        new_order = torch.arange(bsz, device=device).view(-1, 1).repeat(1, beam_size).view(-1)
        encoder_outs = [m.encoder.reorder_encoder_out(e, new_order) for m, e in zip(self.models, encoder_outs)]
        incremental_states: List[Dict[str, Dict[str, Optional[Tensor]]]] = [{} for _ in self.models]

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

        for step in range(max_len + 1):
            if reorder_state is not None:
                for m, inc in zip(self.models, incremental_states):
                    m.decoder.reorder_incremental_state_scripting(inc, reorder_state)
                encoder_outs = [m.encoder.reorder_encoder_out(e, reorder_state) for m, e in zip(self.models, encoder_outs)]
            lprobs = self._forward_decoder(tokens[:, :step + 1], encoder_outs, incremental_states)
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
            cand_scores, cand_indices, cand_beams = self.search.step(
                step, lprobs.view(bsz, -1, self.vocab_size), scores.view(bsz, beam_size, -1)[:, :, :step])
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
                    finalized[sent].append({"tokens": toks, "score": sc, "attention": None, "alignment": None,
                                            "positional_scores": pos})
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
            active_bbsz_idx = torch.gather(cand_bbsz_idx, dim=1, index=active_hypos).view(-1)
            tokens[:, :step + 1] = torch.index_select(tokens[:, :step + 1], dim=0, index=active_bbsz_idx)
            tokens.view(bsz, beam_size, -1)[:, :, step + 1] = torch.gather(cand_indices, dim=1, index=active_hypos)
            if step > 0:
                scores[:, :step] = torch.index_select(scores[:, :step], dim=0, index=active_bbsz_idx)
            scores.view(bsz, beam_size, -1)[:, :, step] = torch.gather(cand_scores, dim=1, index=active_hypos)
            reorder_state = active_bbsz_idx

        for sent in range(bsz):
            sc = torch.tensor([float(h["score"]) for h in finalized[sent]])
            _, order = torch.sort(sc, descending=True)
            finalized[sent] = [finalized[sent][i] for i in order.tolist()]
        return finalized
