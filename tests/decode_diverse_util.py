"""Shared by tests/test_decode_diverse_cpu.py and tests/test_decode_diverse_gpu.py: the synthetic per-step logits of the cst_beam_step
kernel test and a plain fp32 torch restatement of ONE search step with the two diverse strategies (include/cst.h, ABI 12), in the
reference's order of operations:
  groups    search.py DiverseBeamSearch.step :568-618 — per group g (rows g::G) lp + (-S) * count, then + cumulative score, top 2*beam/G
            with ties to the smaller local_row * V + token, the groups' lists interleaved (candidate j * G + g, parent local_row * G + g);
  siblings  search.py DiverseSiblingsSearch.step :765-814 — per row the sorted top 2*beam of lp + score, minus (p + 1) * R at position p,
            the sentence's top 2*beam of those with ties to the smaller row * 2*beam + p; step 0 plain.
The masks (NaN, pad, unk, max-len, prefix, min-len, n-gram ban) and the eos / finalisation / next-row bookkeeping are those of
decode_constraints_util.search_step, restated here with the beam width as a parameter (that module fixes beam 4).

At step 0 the kernel reads the sentence's first row for every group and records it as the parent, the reference reads row g: the step-0
logits below are equal within a sentence, and the restatement records the first row.

While it runs, the restatement gathers what the CPU test asserts: how often the penalty changed a selection, the smallest margin at a
place where the kernel's order of additions (penalty added to lp + score, include/cst.h) could flip an id, and the smallest number of
finite candidates of an unforced row."""
import math

import torch

from decode_constraints_util import EOS, HOT, PAD, PREFIX, UNK, banned_tokens, family  # noqa: F401

BSZ, MAX_LEN = 3, 12
# (dtype name, vocabulary, ensemble members): the smallest shapes that reach each row-kernel family feeding the merge kernel
CASES = [("fp32", 60, 1), ("bf16", 10000, 1), ("bf16", 20488, 1), ("fp32", 10248, 2)]
# name -> (beam, ("groups", G, S) | ("siblings", R), n-gram size, with prefix)
VARIANTS = {
    "g2": (4, ("groups", 2, 0.5), 0, False),
    "g4": (4, ("groups", 4, 0.5), 0, False),
    "g3_b6": (6, ("groups", 3, 0.5), 0, False),
    "g3_b6_s03": (6, ("groups", 3, 0.3), 0, False),
    "sib_05": (4, ("siblings", 0.5), 0, False),
    "sib_03": (4, ("siblings", 0.3), 0, False),
    "g2_ngram2": (4, ("groups", 2, 0.5), 2, False),
    "g2_prefix": (4, ("groups", 2, 0.5), 0, True),
}


# seed of the logits per (case, variant), chosen so that the restatement meets the non-vacuity and margin conditions of
# tests/test_decode_diverse_cpu.py (margins are small at a decision boundary; a seed is a choice of inputs, not of a bound)
SEEDS = {
    ("fp32", 60, 1, "g3_b6_s03"): 2, ("fp32", 60, 1, "g4"): 1, ("fp32", 60, 1, "sib_03"): 1, ("fp32", 60, 1, "sib_05"): 1,
    ("bf16", 10000, 1, "g2_ngram2"): 1, ("bf16", 10000, 1, "g3_b6_s03"): 2, ("bf16", 10000, 1, "g4"): 4, ("bf16", 10000, 1, "sib_03"): 1,
    ("bf16", 20488, 1, "g2_ngram2"): 1,
    ("fp32", 10248, 2, "g3_b6_s03"): 2, ("fp32", 10248, 2, "g4"): 1, ("fp32", 10248, 2, "sib_03"): 1,
}


def step_logits(dtype_name, V, members, step, beam, seed=0):
    """The ladder of decode_constraints_util.step_logits (unit noise, the HOT tokens 14 .. 9 above it, eos rising with the step: the
    cumulative scores stay well inside 32, where 1e-5 is several ulp) for BSZ * beam rows; at step 0 the rows of a sentence are equal."""
    g = torch.Generator().manual_seed(100003 * step + 17 * V + members + (7 if dtype_name == "bf16" else 0) + 1009 * beam + 7919 * seed)
    rows = BSZ * beam
    out = []
    for _ in range(members):
        x = torch.randn(rows, V, generator=g)
        x[:, list(HOT)] = 14.0 - torch.arange(len(HOT), dtype=torch.float32) + torch.randn(rows, len(HOT), generator=g)
        x[:, EOS] = 8.0 + 0.7 * step + torch.randn(rows, generator=g)
        if dtype_name == "bf16":
            # bf16 logits below 16 lie on a lattice of 1/16, and so do the penalties 0.5 * count: two tokens of one row whose logits
            # differ by a multiple of 0.5 would tie EXACTLY in real numbers after the penalty, and rounding alone would decide the id.
            # So the large logits are multiples of 0.5 plus a residue of their own (k / 16 for the k-th, all below 16): no two of them
            # ever differ by a multiple of 0.5.
            rung = 14.0 - torch.arange(len(HOT), dtype=torch.float32)
            x[:, list(HOT)] = rung + ((x[:, list(HOT)] - rung) * 2).round().clamp(-6, 3) / 2 + torch.arange(len(HOT), dtype=torch.float32) / 16
            x[:, EOS] = ((x[:, EOS] * 2).round() / 2).clamp(max=15.5) + len(HOT) / 16.0
        if step == 0:
            x = x.view(BSZ, beam, V)[:, :1].expand(BSZ, beam, V).reshape(rows, V).clone()
        out.append(x.to(torch.bfloat16 if dtype_name == "bf16" else torch.float32))
    return out


def new_state(beam, device="cpu"):
    bbsz, L1, LT = BSZ * beam, MAX_LEN + 1, MAX_LEN + 2
    tokens = torch.full((bbsz, LT), PAD, dtype=torch.long, device=device)
    tokens[:, 0] = EOS
    anc = torch.zeros(bbsz, L1, dtype=torch.int32, device=device)
    anc[:, 0] = torch.arange(bbsz, dtype=torch.int32, device=device)
    return dict(tokens=tokens, scores=torch.zeros(bbsz, L1, device=device), anc=anc,
                ignore=torch.zeros(BSZ, beam, dtype=torch.uint8, device=device), finished=torch.zeros(BSZ, dtype=torch.uint8, device=device),
                nfinal=torch.zeros(BSZ, dtype=torch.int32, device=device), fin_tokens=torch.zeros(BSZ, beam, L1, dtype=torch.long, device=device),
                fin_score=torch.zeros(BSZ, beam, device=device), fin_len=torch.zeros(BSZ, beam, dtype=torch.int32, device=device),
                changed=0, places=0, dead_places=0, dead=[False] * BSZ, ended_by_prefix=[False] * BSZ, margin=math.inf, min_finite=10 ** 9)


def _margin(st, sorted_vals, n_sel):
    """sorted_vals [BSZ, n] descending: the gaps between adjacent selected values and between the last selected and the first unselected
    one.  Not counted, because the tie rule decides them on both sides alike: pairs of -inf, and the bit-equal values of the rows of a
    sentence at its forced steps and after its prefix's eos (st["dead"]: the rows all hold the first row's numbers, in the kernel as here)."""
    v = sorted_vals[:, :n_sel + 1].double()
    gap = v[:, :-1] - v[:, 1:]
    ok = torch.isfinite(v[:, :-1])  # (finite - -inf = inf: harmless)
    ok[[b for b in range(BSZ) if st["dead"][b]]] = False
    if bool(ok.any()):
        st["margin"] = min(st["margin"], float(gap[ok].min()))


def select(st, lp, s, beam, mode):
    """lp [BSZ * beam, V] after the masks -> (c_score, c_tok, c_beam) [BSZ, 2 * beam] by the strategy `mode` (None: plain beam search)."""
    V = lp.size(1)
    K = 2 * beam
    scores = st["scores"]
    lp3 = lp.view(BSZ, beam, V)
    prev = scores[:, s - 1].view(BSZ, beam, 1) if s > 0 else None
    if mode is None or (mode[0] == "siblings" and s == 0):
        cand = lp3[:, 0] if s == 0 else (lp3 + prev).view(BSZ, -1)
        order = torch.sort(cand, dim=1, descending=True, stable=True)[1][:, :K]  # equal values keep their flat-index order
        return torch.gather(cand, 1, order), order % V, order // V
    if mode[0] == "siblings":
        R = mode[1]
        val, tok = torch.sort(lp3 + prev, dim=2, descending=True, stable=True)
        val, tok = val[:, :, :K], tok[:, :, :K]
        pen = val - torch.arange(1, K + 1, device=lp.device).to(val) * R
        flat = pen.reshape(BSZ, -1)
        sv, order = torch.sort(flat, dim=1, descending=True, stable=True)
        plain = torch.sort(val.reshape(BSZ, -1), dim=1, descending=True, stable=True)[1][:, :K]
        for b in range(BSZ):
            st["places"] += 1
            st["dead_places"] += int(st["dead"][b])
            st["changed"] += int(set(order[b, :K].tolist()) != set(plain[b].tolist()))
        _margin(st, sv, K)
        order = order[:, :K]
        return torch.gather(flat, 1, order), torch.gather(tok.reshape(BSZ, -1), 1, order), order // K
    _, G, S = mode
    mb = beam // G
    counts = torch.zeros(BSZ, V, device=lp.device)
    outs = []
    for g in range(G):
        lp_g = lp3[:, g::G]
        if g > 0:
            lp_pen = torch.add(lp_g, counts.unsqueeze(1), alpha=-S)
        else:
            lp_pen = lp_g
        if s == 0:
            cand, plain_c = lp_pen[:, 0], lp_g[:, 0]
        else:
            cand, plain_c = (lp_pen + prev[:, g::G]).reshape(BSZ, -1), (lp_g + prev[:, g::G]).reshape(BSZ, -1)
        sv, order = torch.sort(cand, dim=1, descending=True, stable=True)
        if g > 0:
            plain = torch.sort(plain_c, dim=1, descending=True, stable=True)[1][:, :2 * mb]
            for b in range(BSZ):
                st["places"] += 1
                st["dead_places"] += int(st["dead"][b])
                st["changed"] += int(set(order[b, :2 * mb].tolist()) != set(plain[b].tolist()))
        _margin(st, sv, 2 * mb)
        order = order[:, :2 * mb]
        tok = order % V
        parent = (order // V) * G + g if s > 0 else torch.zeros_like(order)
        outs.append((torch.gather(cand, 1, order), tok, parent))
        counts.scatter_add_(1, tok, torch.ones_like(tok, dtype=counts.dtype))
    return tuple(torch.stack([o[i] for o in outs], dim=2).view(BSZ, -1) for i in range(3))


def search_step(st, logits, s, beam, mode=None, ngram=0, prefix=None, min_len=1, unk_penalty=0.0):
    """One step of the search at step s on state st (changed in place).  logits: list of [bbsz, V] (members), any float dtype."""
    bbsz, V = logits[0].shape
    K = 2 * beam
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
    forced = [False] * BSZ
    if prefix is not None and s < prefix.size(1) and s < MAX_LEN:
        for b in range(BSZ):
            t = int(prefix[b, s])
            rows = slice(b * beam, (b + 1) * beam)
            if t != PAD:
                forced[b] = True
                keep = lp[rows, t].clone()
                lp[rows] = -math.inf
                lp[rows, t] = keep
            if t == EOS:  # the sentence's first beam stands for all its beams
                st["ended_by_prefix"][b] = True
                lp[rows] = lp[b * beam].clone()
                tokens[rows] = tokens[b * beam].clone()
                scores[rows] = scores[b * beam].clone()
                anc[rows] = anc[b * beam].clone()
    elif s < min_len:
        lp[:, EOS] = -math.inf
    if ngram:
        tk_all = tokens.tolist()
        for h in range(bbsz):
            ban = banned_tokens(tk_all[h], s, ngram)
            if ban:
                lp[h, torch.tensor(sorted(set(ban)), device=dev)] = -math.inf
    if s < MAX_LEN:  # (the last step leaves eos alone; a forced row its one token: -inf candidates follow in token order on both sides)
        live = [b for b in range(BSZ) if not forced[b]]
        if live:
            fin = torch.isfinite(lp.view(BSZ, beam, V)[live]).sum(-1)
            st["min_finite"] = min(st["min_finite"], int(fin.min()))
    # places where no penalty can change anything: a forced step (one finite candidate per row) and the junk rows of a sentence that its
    # prefix has ended
    st["dead"] = [forced[b] or st["ended_by_prefix"][b] for b in range(BSZ)]
    c_score, c_tok, c_beam = select(st, lp, s, beam, mode)
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


_RUNS = {}


def run_restatement(dtype_name, V, members, variant, seed=None):
    """The whole search by the restatement alone, on the CPU, once per (case, variant): the final state with the gathered figures."""
    key = (dtype_name, V, members, variant)
    if seed is not None:
        key = key + (seed,)
    else:
        seed = SEEDS.get(key, 0)
    if key not in _RUNS:
        beam, mode, ngram, with_prefix = VARIANTS[variant]
        prefix = torch.tensor(PREFIX) if with_prefix else None
        st = new_state(beam)
        for s in range(MAX_LEN + 1):
            search_step(st, step_logits(dtype_name, V, members, s, beam, seed), s, beam, mode=mode, ngram=ngram, prefix=prefix)
        _RUNS[key] = st
    return _RUNS[key]
