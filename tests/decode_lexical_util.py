"""Shared by tests/test_decode_lexical_cpu.py and tests/test_decode_lexical_gpu.py: a plain fp32 torch / Python restatement of ONE
search step with lexical constraints (cst_beam_step_lex, include/cst.h; search.py LexicallyConstrainedBeamSearch :210-523), written
from the rule and independently of chimera-st_amd/lexical_constraints.py, so that the two check each other:
  1. the masks of the beam step (NaN, pad, unk, max-len, min-len, n-gram ban — those of decode_diverse_util.search_step, whose
     synthetic logits, state and n-gram helper are reused), then at steps > 0 lp[eos] = -inf for a row whose state is not finished;
  2. the list L: the sentence's plain top 2*beam, at steps > 0 every row's own best, then per row (the first row only at step 0) one
     candidate per next token of the row's state, ascending;
  3. bank = bank of advance(parent's state, token); fp32 key = float((nd - bank) * -100) + value; stable descending order by key;
  4. adjacent duplicates (same parent and token; cyclic) dropped;
  5. stripes nd - bank + j * (survivors + 1) within runs of equal banks, stable ascending order, first 2*beam;
  6. the eos / finalisation / next-row bookkeeping of the beam step, and next row i takes the state of candidate act[i].
Constraint states are tiny classes of their own: an index into the concatenated constraints (ordered), a PATH in the trie — the tuple
of tokens from the root — with two counters keyed by paths (unordered).

Some constraint tokens lie OUTSIDE the HOT tokens of the ladder (a noise token costs about -13): a hypothesis gets them only through
the next-token and row-best additions, never through the plain top 2*beam.

While it runs the restatement gathers what the CPU test asserts: how often a selected candidate was not in the plain top 2*beam, and the
smallest key / value gaps at which rounding inside the kernel's log-softmax could flip an id."""
import math
from collections import Counter

import numpy as np
import torch

from decode_diverse_util import BSZ, CASES, EOS, HOT, MAX_LEN, PAD, UNK, banned_tokens, new_state, step_logits  # noqa: F401

LM_WEIGHT = 0.3
EOS_RISE_FROM = 2
# name -> (beam, representation, constraints per sentence, n-gram size, with an LM row)
VARIANTS = {
    "ord_single": (4, "ordered", [[[23]], [[50]], [[41]]], 0, False),
    "ord_multi": (6, "ordered", [[[9, 33], [21]], [], [[17, 17, 9]]], 0, False),
    "unord_shared": (4, "unordered", [[[9, 17], [9, 33], [7]], [[17, 5], [17, 9], [33]], [[5, 29], [5, 9], [17]]], 0, False),
    "unord_dup": (4, "unordered", [[[17], [17]], [[9, 33], [9, 33]], [[33], [33], [44]]], 0, False),
    "ord_ngram2": (4, "ordered", [[[9, 5]], [[23]], [[17, 9]]], 2, False),
    "ord_lm": (4, "ordered", [[[23]], [[17, 33]], [[17]]], 0, True),
}
# seed of the logits per (case, variant), chosen on the CPU so that the restatement meets the non-vacuity and margin conditions of
# tests/test_decode_lexical_cpu.py (a seed is a choice of inputs, not of a bound); absent: 0
SEEDS = {
    ("fp32", 60, 1, "unord_dup"): 7,
    ("bf16", 10000, 1, "ord_multi"): 2, ("bf16", 10000, 1, "unord_shared"): 2, ("bf16", 10000, 1, "unord_dup"): 2, ("bf16", 10000, 1, "ord_ngram2"): 4,
    ("bf16", 20488, 1, "ord_multi"): 2, ("bf16", 20488, 1, "unord_shared"): 1, ("bf16", 20488, 1, "unord_dup"): 5, ("bf16", 20488, 1, "ord_ngram2"): 1,
    ("fp32", 10248, 2, "unord_dup"): 11,
}


def pack(constraints):
    """The packed layout [count, tokens of c0, 0, tokens of c1, 0, ...], zero-padded, int64 [bsz, W]."""
    rows = [[len(cs)] + [x for c in cs for x in list(c) + [0]] for cs in constraints]
    W = max(len(r) for r in rows)
    return torch.tensor([r + [0] * (W - len(r)) for r in rows], dtype=torch.long)


class Ordered:
    def __init__(self, constraints, at=-1):
        self.cs, self.at = constraints, at
        self.seq = [t for c in constraints for t in c]
        self.ends = [j == len(c) - 1 for c in constraints for j in range(len(c))]
        self.nd = len(set(self.seq))

    @property
    def bank(self):
        return self.at + 1

    @property
    def finished(self):
        return self.at + 1 == len(self.seq)

    def next_tokens(self):
        out = []
        if self.at > 0:
            out.append(self.seq[0])
        if not self.finished:
            out.append(self.seq[self.at + 1])
        return sorted(set(out))

    def advance(self, t):
        if self.finished:
            to = self.at
        elif self.seq[self.at + 1] == t:
            to = self.at + 1
        elif self.at == -1 or self.ends[self.at]:  # (the reference reads endpoints[-1] at the root: its last entry, always true)
            to = self.at
        else:
            to = 0 if t == self.seq[0] else -1
        return Ordered(self.cs, to)

    def word(self):
        """What the device keeps in the state's first word."""
        return self.at


class Unordered:
    """path: the tokens from the trie's root to the current node; gen / comp: Counters keyed by paths."""

    def __init__(self, constraints, path=(), gen=None, comp=None):
        self.cs = [tuple(c) for c in constraints]
        self.path, self.gen, self.comp = tuple(path), Counter(gen or {}), Counter(comp or {})
        self.nd = len(set(t for c in self.cs for t in c))

    def _below(self, q):  # constraints that pass through or end at q
        return sum(1 for c in self.cs if c[:len(q)] == q)

    def _ends(self, q):
        return sum(1 for c in self.cs if c == q)

    @property
    def bank(self):
        return sum(self.gen.values())

    @property
    def finished(self):
        pending = 1 if self.path and self._ends(self.path) > self.comp[self.path] else 0
        return len(self.cs) - (sum(self.comp.values()) + pending) == 0

    def next_tokens(self):
        out = set()
        for q in ((), self.path):
            out |= {c[len(q)] for c in self.cs if len(c) > len(q) and c[:len(q)] == q}
        return sorted(out)

    def _open(self, q):
        return self._below(q) > 0 and self.gen[q] < self._below(q)

    def advance(self, t):
        gen, comp = Counter(self.gen), Counter(self.comp)
        down = self.path + (t,)
        if self._open(down):
            gen[down] += 1
            return Unordered(self.cs, down, gen, comp)
        to = (t,) if self._open((t,)) else ()
        if to:
            gen[to] += 1
        q = self.path
        while q:
            if self._ends(q) > self.comp[q]:
                comp[q] += 1
                break
            gen[q] -= 1
            q = q[:-1]
        return Unordered(self.cs, to, gen, comp)

    def word(self):
        """The device's node number: nodes are numbered in order of creation while the constraints are inserted one after the other."""
        nodes = [()]
        for c in self.cs:
            for j in range(1, len(c) + 1):
                if c[:j] not in nodes:
                    nodes.append(c[:j])
        return nodes.index(self.path)


def root_states(representation, constraints, beam):
    cls = Ordered if representation == "ordered" else Unordered
    return [[cls(cs)] * beam for cs in constraints]


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def select_sentence(cand, states, K, stats=None, n_plain=None):
    """Rules 3-5 over cand = [(value, token, parent)] of one sentence -> the chosen [(value, token, parent, state)]."""
    nd = states[0].nd
    adv = [states[p].advance(t) for _, t, p in cand]
    key = [float(np.float32(np.float32((nd - a.bank) * -100) + np.float32(v))) for (v, _, _), a in zip(cand, adv)]
    order = sorted(range(len(cand)), key=lambda i: -key[i])  # stable; -inf last
    kept = [i for q, i in enumerate(order) if cand[i][1:] != cand[order[q - 1]][1:]]
    stripe, j = [], 0
    for q, i in enumerate(kept):
        j = j + 1 if q > 0 and adv[i].bank == adv[kept[q - 1]].bank else 0
        stripe.append(nd - adv[i].bank + j * (len(kept) + 1))
    chosen = [kept[q] for q in sorted(range(len(kept)), key=lambda q: stripe[q])][:K]
    if stats is not None:
        plain = {cand[i][1:] for i in range(n_plain)}
        stats["places"] += 1
        stats["forced"] += int(any(cand[i][1:] not in plain for i in chosen))
        picked = {cand[i][1:] for i in chosen}
        for a, b in zip(order[:-1], order[1:]):  # gaps between distinct finite candidates adjacent in key order, one of them selected
            if cand[a][1:] == cand[b][1:] or not (math.isfinite(key[a]) and math.isfinite(key[b])):
                continue
            if cand[a][1:] in picked or cand[b][1:] in picked:
                stats["key_gap"] = min(stats["key_gap"], key[a] - key[b])
    return [cand[i] + (adv[i],) for i in chosen]


def masked_lprobs(st, logits, s, ngram=0, min_len=1, unk_penalty=0.0, lm_logits=None, lm_weight=LM_WEIGHT):
    """The log-probabilities [bbsz, V] of step s after the generator's masks (what a search strategy's step() is handed)."""
    bbsz, V = logits[0].shape
    dev = logits[0].device
    lps = [torch.log_softmax(x.float(), dim=-1) for x in logits]
    lp = lps[0] if len(lps) == 1 else torch.logsumexp(torch.stack(lps, 0), 0) - math.log(len(lps))
    if lm_logits is not None:
        lp = lp + torch.log_softmax(lm_logits.float(), dim=-1) * lm_weight
    lp[lp != lp] = -math.inf
    lp[:, PAD] = -math.inf
    lp[:, UNK] -= unk_penalty
    if s >= MAX_LEN:
        lp[:, :EOS] = -math.inf
        lp[:, EOS + 1:] = -math.inf
    if s < min_len:
        lp[:, EOS] = -math.inf
    if ngram:
        tk_all = st["tokens"].tolist()
        for h in range(bbsz):
            ban = banned_tokens(tk_all[h], s, ngram)
            if ban:
                lp[h, torch.tensor(sorted(set(ban)), device=dev)] = -math.inf
    return lp


def search_step(st, logits, s, beam, states, ngram=0, min_len=1, unk_penalty=0.0, lm_logits=None, lm_weight=LM_WEIGHT, stats=None,
                trace=None):
    """One constrained step at step s on state st and the rows' constraint states `states` [BSZ][beam] (both changed in place).
    logits: list of [bbsz, V] (members); lm_logits: [bbsz, V] or None.  trace: a dict that receives the step's candidates (c_score,
    c_tok, c_beam [BSZ, 2 * beam]) and the candidates the next rows continue (act [BSZ][beam])."""
    bbsz, V = logits[0].shape
    K = 2 * beam
    dev = logits[0].device
    lp = masked_lprobs(st, logits, s, ngram, min_len, unk_penalty, lm_logits, lm_weight)
    tokens, scores, anc = st["tokens"], st["scores"], st["anc"]
    if s > 0:  # rule 1
        for h in range(bbsz):
            if not states[h // beam][h % beam].finished:
                lp[h, EOS] = -math.inf
    lp3 = lp.view(BSZ, beam, V)
    val3 = lp3[:, :1] if s == 0 else lp3 + scores[:, s - 1].view(BSZ, beam, 1)
    flat = val3.reshape(BSZ, -1)
    sv, order = torch.sort(flat, dim=1, descending=True, stable=True)  # equal values keep their flat-index order
    if stats is not None:  # the plain top 2*beam: adjacent gaps, and the gap to the first one left out
        v = sv[:, :K + 1].double()
        gap = (v[:, :-1] - v[:, 1:])[torch.isfinite(v[:, :-1]) & torch.isfinite(v[:, 1:])]
        if gap.numel():
            stats["val_gap"] = min(stats["val_gap"], float(gap.min()))
    val_cpu = val3.cpu()
    c_score = torch.full((BSZ, K), -math.inf, device=dev)
    c_tok = torch.full((BSZ, K), PAD, dtype=torch.long, device=dev)
    c_beam = torch.zeros(BSZ, K, dtype=torch.long, device=dev)
    c_state = []
    for b in range(BSZ):
        cand = [(float(sv[b, k]), int(order[b, k]) % V, int(order[b, k]) // V) for k in range(K)]
        rows = 1 if s == 0 else beam
        if s > 0:
            rv, rt = torch.sort(val_cpu[b], dim=1, descending=True, stable=True)
            cand += [(float(rv[r, 0]), int(rt[r, 0]), r) for r in range(beam)]
        for r in range(rows):
            cand += [(float(val_cpu[b, r, t]), t, r) for t in states[b][r].next_tokens()]
        live = stats is not None and not bool(st["finished"][b]) and any(len(c) for c in [states[b][0].cs])
        chosen = select_sentence(cand, states[b], K, stats if live else None, K)
        for k, (v, t, p, _) in enumerate(chosen):
            c_score[b, k], c_tok[b, k], c_beam[b, k] = v, t, p
        c_state.append([c[3] for c in chosen])
    new_tokens, new_scores, new_anc = tokens.clone(), scores.clone(), anc.clone()
    if trace is not None:
        trace.update(c_score=c_score, c_tok=c_tok, c_beam=c_beam, act=[])
    for b in range(BSZ):
        ign = st["ignore"][b].tolist()
        was_finished = bool(st["finished"][b])
        nf = int(st["nfinal"][b])
        em, any_top_eos = [], False
        for k in range(K):
            e = int(c_tok[b, k]) == EOS and float(c_score[b, k]) != -math.inf
            if k < beam and ign[k]:
                e = False
            em.append(e)
            if k < beam and e:
                any_top_eos = True
                if not was_finished and nf < beam:
                    bi = b * beam + int(c_beam[b, k])
                    st["fin_tokens"][b, nf, :s] = tokens[bi, 1:s + 1]
                    st["fin_tokens"][b, nf, s] = EOS
                    st["fin_len"][b, nf] = s + 1
                    st["fin_score"][b, nf] = c_score[b, k] / float(s + 1)  # normalize_scores, len_penalty 1
                    nf += 1
        st["nfinal"][b] = nf
        if any_top_eos and not was_finished and (nf == beam or s == MAX_LEN):
            st["finished"][b] = 1
        dead = [em[k] or (k < beam and bool(ign[k])) for k in range(K)]
        live = [k for k in range(K) if not dead[k]][:beam]
        act = (live + [k for k in range(K) if dead[k]])[:beam]
        st["ignore"][b] = torch.tensor([1 if i >= len(live) else 0 for i in range(beam)], dtype=torch.uint8, device=dev)
        if trace is not None:
            trace["act"].append(act)
        if s < MAX_LEN:
            for i, k in enumerate(act):
                src, dst = b * beam + int(c_beam[b, k]), b * beam + i
                new_tokens[dst, :s + 1] = tokens[src, :s + 1]
                new_tokens[dst, s + 1] = c_tok[b, k]
                new_scores[dst, :s] = scores[src, :s]
                new_scores[dst, s] = c_score[b, k]
                new_anc[dst, :s + 1] = anc[src, :s + 1]
                new_anc[dst, s + 1] = dst
            states[b] = [c_state[b][k] for k in act]  # rule 6
    if s < MAX_LEN:
        st["tokens"], st["scores"], st["anc"] = new_tokens, new_scores, new_anc
    return st


def lex_step_logits(dtype_name, V, members, step, beam, seed=0):
    """The ladder of decode_diverse_util.step_logits with eos rising half a logit per step more from step 3 on: a constrained hypothesis
    spends steps on its constraints before it may end, and every sentence is to finish before the forced eos of step MAX_LEN.  (Multiples
    of 0.5: the bf16 lattice of step_logits keeps its residues; fp32 and bf16 both hold the sums exactly.)"""
    out = step_logits(dtype_name, V, members, step, beam, seed)
    for x in out:
        x[:, EOS] += 0.5 * max(0, step - EOS_RISE_FROM)
    return out


def lm_step_logits(dtype_name, V, step, beam, seed=0):
    """The LM row of variant ord_lm: unit noise with its own preferences among the HOT tokens, in the case's storage dtype."""
    g = torch.Generator().manual_seed(424243 * step + 31 * V + 1013 * beam + 7919 * seed + (7 if dtype_name == "bf16" else 0))
    x = torch.randn(BSZ * beam, V, generator=g)
    x[:, list(HOT) + [EOS]] += 8.0 + 2.0 * torch.randn(BSZ * beam, len(HOT) + 1, generator=g)  # (peaked: its weighted log-probs stay small)
    if step == 0:
        x = x.view(BSZ, beam, V)[:, :1].expand(BSZ, beam, V).reshape(BSZ * beam, V).clone()
    return x.to(torch.bfloat16 if dtype_name == "bf16" else torch.float32)


def contains(tokens, constraints, ordered):
    """The hypothesis holds every constraint as a contiguous run (ordered: in the given order, without overlap)."""
    tokens, at = list(tokens), 0
    for c in constraints:
        found = next((i for i in range(at if ordered else 0, len(tokens) - len(c) + 1) if tokens[i:i + len(c)] == list(c)), None)
        if found is None:
            return False
        at = found + len(c) if ordered else 0
    return True


_RUNS = {}


def run_restatement(dtype_name, V, members, variant, seed=None):
    """The whole search by the restatement alone, on the CPU, once per (case, variant): (final state, gathered figures)."""
    key = (dtype_name, V, members, variant)
    if seed is not None:
        key = key + (seed,)
    else:
        seed = SEEDS.get(key, 0)
    if key not in _RUNS:
        beam, representation, constraints, ngram, with_lm = VARIANTS[variant]
        st = new_state(beam)
        states = root_states(representation, constraints, beam)
        stats = dict(places=0, forced=0, key_gap=math.inf, val_gap=math.inf)
        for s in range(MAX_LEN + 1):
            lm = lm_step_logits(dtype_name, V, s, beam, seed) if with_lm else None
            search_step(st, lex_step_logits(dtype_name, V, members, s, beam, seed), s, beam, states, ngram=ngram, lm_logits=lm, stats=stats)
        _RUNS[key] = (st, stats)
    return _RUNS[key]
