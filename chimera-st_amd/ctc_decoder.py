"""Decoders of a CTC acoustic model's emissions for fairseq_infer.py — what examples/speech_recognition/w2l_decoder.py is to the
reference's infer.py.

CtcViterbiDecoder   W2lViterbiDecoder (:91-127) for the ctc criterion: CpuViterbiPath over an all-zero transition matrix is the per-frame
                    argmax, groupby and dropping the blank — cst_ctc_greedy.  The score is 0, as the reference's.
CtcBeamDecoder      CTC prefix beam search (Graves 2006 §7.5.3; Hannun et al. 2014, Alg. 1) on the device: cst_ctc_topn + cst_ctc_beam
                    (include/cst.h states the rules).  It is NOT flashlight's lexicon-free decoder (W2lKenLMDecoder / W2lFairseqLMDecoder
                    without a lexicon): that one keeps the best alignment per state, this one sums all alignments of a prefix, and the
                    language model rescores the n best here instead of steering the search.  CST_CTC_BEAM=host, or a request beyond the
                    kernel's envelope, takes the host route: prefix_beam_search_host, a plain numpy restatement with the same rules.

Both expose generate(models, sample, **unused) -> per utterance a list of {"tokens", "score", "ctc_score", "lm_score"}, best first, the
shape process_predictions of infer.py consumes, and decode(emissions [T, B, V], input_len) for emissions that are already there
(--load-emissions)."""
import math
import os

import numpy as np
import torch

from .dictionary import post_process

NINF = float("-inf")


def host_route():
    return os.environ.get("CST_CTC_BEAM", "") == "host"


def _lae(a, b):
    m, n = (a, b) if a >= b else (b, a)
    if m == NINF:
        return NINF
    return m + math.log1p(math.exp(n - m))


def _search_one(lp, blank, K, N, theta, nbest):
    """One utterance: lp [T, V] float64 log-probabilities -> [(tokens, score)] best first.  The rules and the tie order of cst_ctc_beam."""
    T, V = lp.shape
    ids_all = np.array([v for v in range(V) if v != blank], dtype=np.int64)
    par, tok, kids = [-1], [-1], {}  # kids: (parent, token) -> node, so a prefix that comes back has the node it had
    beam = [(0, 0.0, NINF)]  # (node, p_b, p_nb) in rank order
    for t in range(T):
        row = lp[t]
        lst = ids_all[np.lexsort((ids_all, -row[ids_all]))[:N]] if ids_all.size else ids_all
        lpl = row[lst]
        inlist = {int(c): n for n, c in enumerate(lst)}
        pos = {e[0]: i for i, e in enumerate(beam)}
        tots = [_lae(pb, pnb) for _, pb, pnb in beam]
        spb = [tt + row[blank] for tt in tots]
        spnb = [pnb + row[tok[nd]] if nd else NINF for nd, _, pnb in beam]
        vals = np.empty((len(beam), len(lst)), dtype=np.float64)
        for i, (nd, pb, _) in enumerate(beam):
            vals[i] = tots[i] + lpl
            n = inlist.get(tok[nd])
            if n is not None:
                vals[i, n] = pb + lpl[n]
        for j, (nd, _, _) in enumerate(beam):
            if nd:
                i, n = pos.get(par[nd]), inlist.get(tok[nd])
                if i is not None and n is not None:
                    spnb[j] = _lae(spnb[j], float(vals[i, n]))
                    vals[i, n] = NINF
        cands = [(-_lae(spb[i], spnb[i]), i, 0, -1) for i in range(len(beam))]
        ii, nn = np.nonzero(vals > NINF)
        cands += [(-float(vals[i, n]), int(i), 1, int(lst[n])) for i, n in zip(ii, nn)]
        cands.sort()
        cut = -cands[0][0] - theta if cands else NINF
        nxt = []
        for ns, i, kind, c in cands:
            if len(nxt) == K or -ns == NINF or -ns < cut:
                break
            if kind == 0:
                nxt.append((beam[i][0], spb[i], spnb[i]))
            else:
                nd = kids.get((beam[i][0], c))
                if nd is None:
                    nd = kids[(beam[i][0], c)] = len(par)
                    par.append(beam[i][0])
                    tok.append(c)
                nxt.append((nd, NINF, -ns))
        beam = nxt
        if not beam:
            break
    out = []
    for nd, pb, pnb in beam[:nbest]:
        seq = []
        while nd > 0:
            seq.append(tok[nd])
            nd = par[nd]
        out.append((seq[::-1], _lae(pb, pnb)))
    return out


def prefix_beam_search_host(logits, input_len, blank, beam, beam_size_token, beam_threshold, nbest):
    """The host route of functional.ctc_prefix_beam_search: logits [T, B, V] (any device and dtype), the same result structure; float64
    on the host."""
    x = logits.detach().to("cpu", torch.float64)
    T, B, V = x.shape
    lp = torch.log_softmax(x, dim=-1).numpy()
    N = max(1, min(int(beam_size_token), V - 1))
    nb = max(1, min(int(nbest), int(beam)))
    lens = [max(0, min(int(n), T)) for n in (input_len.tolist() if torch.is_tensor(input_len) else input_len)]
    return [_search_one(lp[:lens[b], b], int(blank), int(beam), N, float(beam_threshold), nb) for b in range(B)]


def greedy_host(logits, input_len, blank):
    """The host route of functional.ctc_greedy: per utterance the list of ids (argmax — the first of equal maxima —, runs collapsed,
    blank dropped)."""
    x = logits.detach().to("cpu", torch.float32).numpy()
    out = []
    for b, n in enumerate(input_len.tolist() if torch.is_tensor(input_len) else input_len):
        am = np.argmax(x[:max(0, min(int(n), x.shape[0])), b], axis=1).tolist()
        out.append([a for i, a in enumerate(am) if a != blank and (i == 0 or a != am[i - 1])])
    return out


def ctc_blank(tgt_dict):
    """infer.py / w2l_decoder.py:57-61: <ctc_blank> where the dictionary has it, else bos."""
    return tgt_dict.index("<ctc_blank>") if "<ctc_blank>" in tgt_dict.indices else tgt_dict.bos()


class _CtcDecoder:
    def __init__(self, args, tgt_dict):
        self.tgt_dict = tgt_dict
        self.vocab_size = len(tgt_dict)
        self.nbest = max(1, int(getattr(args, "nbest", 1)))
        self.blank = ctc_blank(tgt_dict)

    @torch.no_grad()
    def get_emissions(self, models, sample):
        """models[0]'s raw logits [T, B, V] and the input lengths int64 [B] (w2l_decoder.py:70-81 takes models[0] as well; the
        normalisation to log-probabilities is fused into the kernels)."""
        model = models[0] if isinstance(models, (list, tuple)) else models
        model.eval()
        out = model(**sample["net_input"])
        logits = out["encoder_out"]
        T, B = logits.shape[0], logits.shape[1]
        if out.get("padding_mask") is not None:
            lens = (~out["padding_mask"]).long().sum(-1)
        else:
            lens = torch.full((B,), T, dtype=torch.int64, device=logits.device)
        return logits, lens

    def generate(self, models, sample, **unused):
        return self.decode(*self.get_emissions(models, sample))


class CtcViterbiDecoder(_CtcDecoder):
    def decode(self, emissions, input_len):
        from . import functional as CF
        T, B = emissions.shape[0], emissions.shape[1]
        if host_route():
            ids = greedy_host(emissions, input_len, self.blank)
        else:
            host = CF.ctc_greedy(emissions.cuda(), input_len.cuda().to(torch.int64), self.blank)[2].cpu()
            ids = [host[b * T:b * T + int(host[B * T + b])].tolist() for b in range(B)]
        return [[{"tokens": torch.tensor(s, dtype=torch.int64), "score": 0, "ctc_score": 0, "lm_score": 0}] for s in ids]


class CtcBeamDecoder(_CtcDecoder):
    """args: beam, nbest, beam_threshold, beam_size_token, lm_weight, word_score, post_process.  lm_model: a transformer_lm over the
    SAME dictionary (checked symbol for symbol by check_lm_dictionary), on the device; None: no rescoring."""

    def __init__(self, args, tgt_dict, lm_model=None, lm_dict=None):
        super().__init__(args, tgt_dict)
        self.beam = int(args.beam)
        if self.beam < 1:
            raise ValueError("--beam must be at least 1, got %d" % self.beam)
        self.beam_threshold = float(args.beam_threshold)
        self.beam_size_token = int(args.beam_size_token) if getattr(args, "beam_size_token", None) else self.vocab_size
        self.lm_weight, self.word_score = float(getattr(args, "lm_weight", 0.0)), float(getattr(args, "word_score", 0.0))
        self.post_process = getattr(args, "post_process", "letter")
        self.lm = lm_model
        if lm_model is not None:
            check_lm_dictionary(lm_dict, tgt_dict)
        self.last_route = None

    def search(self, emissions, input_len):
        """[(tokens, score)] per utterance; the route taken is left in self.last_route ("device" / "host")."""
        from . import functional as CF
        from . import kernels as K
        V = emissions.shape[2]
        N = max(1, min(self.beam_size_token, V - 1))
        if host_route() or not K.ctc_beam_supported(self.beam, N):
            self.last_route = "host"
            return prefix_beam_search_host(emissions, input_len, self.blank, self.beam, N, self.beam_threshold, self.nbest)
        self.last_route = "device"
        return CF.ctc_prefix_beam_search(emissions.cuda(), input_len.cuda().to(torch.int64), self.blank, self.beam, N, self.beam_threshold,
                                         self.nbest)

    def lm_scores(self, seqs):
        """The sum of the natural-log token scores, eos included, of each sequence under the language model: teacher-forced, input
        [eos, y...], target [y..., eos]; kernels.score_tokens on the logits, one batch and one transfer per hypothesis length."""
        from . import kernels as K
        d = self.tgt_dict
        limit = self.lm.max_positions()
        longest = max(len(s) for s in seqs) + 1
        if limit is not None and longest > int(limit):
            raise ValueError("a hypothesis of %d tokens (eos included) exceeds the language model's %d positions: rescoring cannot "
                             "score it (lower --max-tokens of the LM's training is not the cure: shorten the audio or train the LM "
                             "with more positions)" % (longest, int(limit)))
        dev = next(self.lm.parameters()).device
        self.lm.eval()
        out = [0.0] * len(seqs)
        by_len = {}
        for i, s in enumerate(seqs):
            by_len.setdefault(len(s), []).append(i)
        for n, idx in sorted(by_len.items()):  # hypotheses of one length form a batch: no row is padded
            y = torch.tensor([seqs[i] for i in idx], dtype=torch.int64).view(len(idx), n)
            eos = torch.full((len(idx), 1), d.eos(), dtype=torch.int64)
            src, tgt = torch.cat([eos, y], dim=1).to(dev), torch.cat([y, eos], dim=1).to(dev)
            logits = self.lm(src, src_lengths=torch.full((len(idx),), n + 1, dtype=torch.int64, device=dev))[0]
            packed = K.score_tokens([logits], tgt, -1)[3].cpu()  # no row is padded, so no id is skipped: the search may emit any class but
            # the blank, the dictionary's pad symbol included, and its probability counts like any other
            pos = packed[:len(idx) * (n + 1)].view(len(idx), n + 1)
            for r, i in enumerate(idx):
                out[i] = float(pos[r].sum())
        return out

    def rescore(self, hyps, lm_scores):
        """hyps: one utterance's [(tokens, ctc_score)] in first-pass order -> the result dicts, sorted (stably) by
        total = ctc_score + lm_weight * lm_score + word_score * n_words, descending."""
        out = []
        for (seq, sc), lm in zip(hyps, lm_scores):
            n_words = len(post_process(self.tgt_dict.string(seq), self.post_process).split())
            out.append({"tokens": torch.tensor(seq, dtype=torch.int64), "score": sc + self.lm_weight * lm + self.word_score * n_words,
                        "ctc_score": sc, "lm_score": lm, "words": n_words})
        out.sort(key=lambda h: -h["score"])  # (list.sort is stable: ties keep the first-pass order)
        return out

    @torch.no_grad()
    def decode(self, emissions, input_len):
        hyps = self.search(emissions, input_len)
        if self.lm is None:
            return [[{"tokens": torch.tensor(seq, dtype=torch.int64), "score": sc, "ctc_score": sc, "lm_score": 0} for seq, sc in utt]
                    for utt in hyps]
        flat = [seq for utt in hyps for seq, _ in utt]
        scores = self.lm_scores(flat) if flat else []
        out, o = [], 0
        for utt in hyps:
            out.append(self.rescore(utt, scores[o:o + len(utt)]))
            o += len(utt)
        return out


def check_lm_dictionary(lm_dict, tgt_dict):
    """The language model must index the very symbols the acoustic model emits: equal length, equal symbol at every id."""
    if lm_dict is None:
        raise ValueError("--lm-model: the language model's dictionary is missing; it must equal the task's target dictionary")
    if len(lm_dict) != len(tgt_dict):
        raise ValueError("--lm-model: the language model's dictionary has %d symbols, the task's target dictionary %d: n-best rescoring "
                         "needs the same dictionary, symbol for symbol" % (len(lm_dict), len(tgt_dict)))
    for i in range(len(tgt_dict)):
        if lm_dict[i] != tgt_dict[i]:
            raise ValueError("--lm-model: symbol %d is %r in the language model's dictionary and %r in the task's target dictionary: "
                             "n-best rescoring needs the same dictionary, symbol for symbol" % (i, lm_dict[i], tgt_dict[i]))
