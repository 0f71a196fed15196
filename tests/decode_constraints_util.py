"""Shared by tests/test_decode_constraints_cpu.py and tests/test_decode_constraints_gpu.py: the synthetic per-step logits of the
cst_beam_step kernel test and a plain fp32 torch restatement of ONE search step with the two decoding constraints
(--prefix-size, --no-repeat-ngram-size) — the same masks in the same order as include/cst.h describes them, top-2*beam over
beam x V with ties to the smaller flat index, and the eos / finalisation / next-row bookkeeping of the beam step.

The restatement runs on whatever device its inputs are on; the CPU test runs it alone to show that the kernel test is not vacuous
(the n-gram ban hits finite candidates in at least a quarter of the (row, step) pairs)."""
import math

import torch

PAD, EOS, UNK = 1, 2, 3
BSZ, BEAM, MAX_LEN = 3, 4, 12
# The tokens given a large margin, on a ladder of one logit per rung: the search prefers the first, so hypotheses repeat themselves and
# the ban bites, and whatever is banned, a next rung with a moderate log-probability is left.  (The scores are compared to 1e-5
# absolute, and two fp32 evaluations of a sum of a dozen log-probabilities agree to a few ulp of the SUM: one ulp is 1.9e-6 up to 32
# and 3.8e-6 beyond, so the inputs must keep the cumulative scores well inside 32.  Two equally likely tokens do not: once both are
# banned the search falls to the noise tokens at -12 each and the scores reach -40.)
HOT = (5, 9, 17, 33, 41, 50)
PREFIX = [[5, 9, 5], [9, EOS, PAD], [17, PAD, PAD]]  # full width / eos inside / shorter than the batch's width

# (dtype name, vocabulary, ensemble members): one case per dispatch family of cst_beam_step — fp32 vectors hold 4 elements, bf16
# vectors 8, 512 threads: NV = ceil(ceil(V / VEC) / 512) vectors per thread in registers for NV <= 5, the wide kernel beyond
CASES = [("fp32", 60, 1), ("fp32", 10000, 1), ("fp32", 10248, 1), ("bf16", 10000, 1), ("bf16", 20488, 1), ("fp32", 60, 2), ("fp32", 10248, 2)]
# (no_repeat_ngram_size, with prefix, min_len)
VARIANTS = {"ngram2": (2, False, 1), "ngram3": (3, False, 1), "prefix": (0, True, 1), "prefix_ngram2_minlen4": (2, True, 4)}


def family(dtype_name, V):
    vec = 8 if dtype_name == "bf16" else 4
    nv = -(-(-(-V // vec)) // 512)
    return "wide" if nv > 5 else "NV%d" % (1 if nv <= 1 else 3 if nv <= 3 else 5)


def step_logits(dtype_name, V, members, step):
    """Fresh random logits [members][BSZ * BEAM, V] of one step, in the case's storage dtype: unit noise, the HOT tokens 14 .. 9 above
    it (each with its own spread, so the beams disagree), eos rising with the step so that hypotheses end at different steps."""
    g = torch.Generator().manual_seed(100003 * step + 17 * V + members + (7 if dtype_name == "bf16" else 0))
    rows = BSZ * BEAM
    out = []
    for _ in range(members):
        x = torch.randn(rows, V, generator=g)
        x[:, list(HOT)] = 14.0 - torch.arange(len(HOT), dtype=torch.float32) + torch.randn(rows, len(HOT), generator=g)
        x[:, EOS] = 8.0 + 0.7 * step + torch.randn(rows, generator=g)
        out.append(x.to(torch.bfloat16 if dtype_name == "bf16" else torch.float32))
    return out


def new_state(device="cpu"):
    bbsz, L1, LT = BSZ * BEAM, MAX_LEN + 1, MAX_LEN + 2
    tokens = torch.full((bbsz, LT), PAD, dtype=torch.long, device=device)
    tokens[:, 0] = EOS
    anc = torch.zeros(bbsz, L1, dtype=torch.int32, device=device)
    anc[:, 0] = torch.arange(bbsz, dtype=torch.int32, device=device)
    return dict(tokens=tokens, scores=torch.zeros(bbsz, L1, device=device), anc=anc,
                ignore=torch.zeros(BSZ, BEAM, dtype=torch.uint8, device=device), finished=torch.zeros(BSZ, dtype=torch.uint8, device=device),
                nfinal=torch.zeros(BSZ, dtype=torch.int32, device=device), fin_tokens=torch.zeros(BSZ, BEAM, L1, dtype=torch.long, device=device),
                fin_score=torch.zeros(BSZ, BEAM, device=device), fin_len=torch.zeros(BSZ, BEAM, dtype=torch.int32, device=device),
                banned_pairs=0)


def banned_tokens(tk, s, n):
    """Row tokens tk[0 .. s] (tk[0] = eos): the tokens that would complete an n-gram the row already holds."""
    if n < 2 or s + 2 - n < 0:
        return []
    last = tk[s + 2 - n:s + 1]
    return [tk[i + n - 1] for i in range(0, s + 2 - n) if tk[i:i + n - 1] == last]


def search_step(st, logits, s, ngram=0, prefix=None, min_len=1, unk_penalty=0.0):
    """One step of the search at step s on state st (changed in place).  logits: list of [bbsz, V] (members), any float dtype."""
    bbsz, V = logits[0].shape
    beam, K = BEAM, 2 * BEAM
    dev = logits[0].device
    lps = [torch.log_softmax(x.float(), dim=-1) for x in logits]
    lp = lps[0] if len(lps) == 1 else torch.logsumexp(torch.stack(lps, 0), 0) - math.log(len(lps))
    lp[lp != lp] = -math.inf
    lp[:, PAD] = -math.inf
    lp[:, UNK] -= unk_penalty
    if s >= MAX_LEN:
        lp[:, :EOS] = -math.inf
        lp[:, EOS + 1:] = -math.inf
    tokens, scores, anc = st["tokens"], st["scores"], st["anc"]
    if prefix is not None and s < prefix.size(1) and s < MAX_LEN:
        for b in range(BSZ):
            t = int(prefix[b, s])
            rows = slice(b * beam, (b + 1) * beam)
            if t != PAD:
                keep = lp[rows, t].clone()
                lp[rows] = -math.inf
                lp[rows, t] = keep
            if t == EOS:  # the sentence's first beam stands for all its beams
                lp[rows] = lp[b * beam].clone()
                tokens[rows] = tokens[b * beam].clone()
                scores[rows] = scores[b * beam].clone()
                anc[rows] = anc[b * beam].clone()
    elif s < min_len:
        lp[:, EOS] = -math.inf
    if ngram:
        tk_all = tokens.tolist()
        for h in range(bbsz):
            if s == 0 and h % beam:
                continue  # only the first beam competes at step 0
            ban = [t for t in banned_tokens(tk_all[h], s, ngram)]
            if ban:
                idx = torch.tensor(sorted(set(ban)), device=dev)
                st["banned_pairs"] += int(torch.isfinite(lp[h, idx]).any())
                lp[h, idx] = -math.inf
    if s == 0:
        cand = lp.view(BSZ, beam, V)[:, :1].reshape(BSZ, -1)
    else:
        cand = (lp + scores[:, s - 1:s]).view(BSZ, -1)
    order = torch.sort(cand, dim=1, descending=True, stable=True)[1][:, :K]  # equal values keep their flat-index order
    c_score = torch.gather(cand, 1, order)
    c_tok, c_beam = order % V, order // V
    new_tokens, new_scores, new_anc = tokens.clone(), scores.clone(), anc.clone()
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
        if s < MAX_LEN:
            for i, k in enumerate(act):
                src, dst = b * beam + int(c_beam[b, k]), b * beam + i
                new_tokens[dst, :s + 1] = tokens[src, :s + 1]
                new_tokens[dst, s + 1] = c_tok[b, k]
                new_scores[dst, :s] = scores[src, :s]
                new_scores[dst, s] = c_score[b, k]
                new_anc[dst, :s + 1] = anc[src, :s + 1]
                new_anc[dst, s + 1] = dst
    if s < MAX_LEN:
        st["tokens"], st["scores"], st["anc"] = new_tokens, new_scores, new_anc
    return st


def run_restatement(dtype_name, V, members, variant, device="cpu"):
    """The whole search by the restatement alone: (state, fraction of (row, step) pairs in which the ban hit a finite candidate)."""
    ngram, with_prefix, min_len = VARIANTS[variant]
    prefix = torch.tensor(PREFIX, device=device) if with_prefix else None
    st = new_state(device)
    for s in range(MAX_LEN + 1):
        logits = [x.to(device) for x in step_logits(dtype_name, V, members, s)]
        search_step(st, logits, s, ngram=ngram, prefix=prefix, min_len=min_len)
    return st, st["banned_pairs"] / float(BSZ * BEAM * (MAX_LEN + 1))
