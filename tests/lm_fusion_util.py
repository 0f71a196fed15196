"""Shared by tests/test_decode_lm_cpu.py, tests/test_decode_lm_gpu.py and tools/ref_harness/make_decode_lm_goldens.py: shallow fusion
with a target-side language model (--lm-path / --lm-weight, reference sequence_generator.py:318-324) restated in plain torch.

  * the stored inputs of the per-element kernel test and of the CPU measurement of its bound (both evaluate the SAME tensors), and the
    torch evaluation of  lp'[v] = fl(lp[v] + fl(w * (x_lm[v] - lse_lm)))  in a chosen dtype (lp: the model's log-probability, single
    or ensemble-combined, after the temperature; the LM is NOT tempered);
  * one fused search step on synthetic per-step logits (the peaked rows of decode_constraints_util) in fp64, with the n-gram ban and
    forced prefixes, and its selection gaps;
  * the whole search over any lp_fn, and a pre-norm Transformer LM forward on the CPU (the oracle's attention and LayerNorm), for the
    fixture decode_lm_tiny.npz."""
import math

import torch

from decode_constraints_util import BEAM, BSZ, EOS, MAX_LEN, PAD, PREFIX, UNK, banned_tokens, step_logits  # noqa: F401

W = 0.5          # lm_weight of the kernel and search tests
STEPS = 6        # steps the search tests take (of a MAX_LEN = 12 search: hypotheses finish from step 3 on)
ROWS, VOCAB = 160, 10000
KERNEL_CASES = [(N, T, dt) for N in (1, 2, 3, 8) for T in (1.0, 0.7) for dt in ("fp32", "bf16")]
CAP = 1e-4 / 13  # the ensemble kernel test's score bar: 1e-4 over the fixture's longest hypothesis
# (dtype name, vocabulary): NV = 1, 3, 5 vectors per thread in registers and the wide body, per storage type
SEARCH_CASES = [("bf16", 1003), ("bf16", 10000), ("bf16", 20000), ("bf16", 20488), ("fp32", 1003), ("fp32", 6000), ("fp32", 10000), ("fp32", 10244)]
SEARCH_SEED = 0  # every (case, N, variant) keeps all selection gaps above 1e-4 with it (test_decode_lm_cpu checks)


def tdtype(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def model_logits(N, dtype, rows=ROWS, V=VOCAB, seed=0):
    """[N, rows, V] model logits (randn x 2.0) in `dtype`: row 5 has -inf in member 1 only at every 7th token (N >= 2), row 9 in
    every member at every 11th."""
    g = torch.Generator().manual_seed(7000 + 1000 * N + seed + (1 if dtype == torch.bfloat16 else 0))
    x = (torch.randn(N, rows, V, generator=g) * 2.0).to(dtype)
    if N >= 2:
        x[1, 5, ::7] = -math.inf
    x[:, 9, ::11] = -math.inf
    return x


def lm_logits(dtype, rows=ROWS, V=VOCAB, seed=0):
    """[rows, V] LM logits (randn x 1.5) in `dtype`: row 7 has -inf at every 13th token."""
    g = torch.Generator().manual_seed(9000 + seed + (1 if dtype == torch.bfloat16 else 0))
    y = (torch.randn(rows, V, generator=g) * 1.5).to(dtype)
    y[7, ::13] = -math.inf
    return y


def fused_lprobs(x, y, w, T, dt):
    """lp' evaluated by torch in `dt` on the stored logits x [N, rows, V] and y [rows, V]."""
    lp = torch.log_softmax(x.to(dt) / T, dim=-1)
    lp = lp[0] if x.size(0) == 1 else torch.logsumexp(lp, dim=0) - math.log(x.size(0))
    return lp + torch.log_softmax(y.to(dt), dim=-1) * w


def fp32_torch_error(x, y, w, T):
    """(largest |fp32 torch - fp64 torch| over the finite elements, largest finite |lp'|); the -inf sets must coincide."""
    a, b = fused_lprobs(x, y, w, T, torch.float32), fused_lprobs(x, y, w, T, torch.float64)
    fin = torch.isfinite(b)
    assert torch.equal(fin, torch.isfinite(a)) and not torch.isnan(a).any() and not torch.isnan(b).any()
    return float((a.double() - b)[fin].abs().max()), float(b[fin].abs().max())


# ---- one fused search step on synthetic logits ------------------------------------------------------------------------------------
def search_logits(dtype_name, V, N, step, seed=SEARCH_SEED, sampling=False):
    """(model logits [N][BSZ * BEAM, V], LM logits [BSZ * BEAM, V]) of one step in the storage dtype: the model's rows are the peaked
    rows of decode_constraints_util.step_logits (sampling: of decode_sampling_util.step_logits, whose tail lies lower); the LM's are
    another draw of the same kind with the ladder reversed, halved in scale, so the LM reorders the model's favourites without
    flattening them."""
    from decode_constraints_util import HOT
    gen = step_logits
    if sampling:
        from decode_sampling_util import step_logits as gen
    model = gen(dtype_name, V, N, step + 100 * seed)
    lm = gen(dtype_name, V, 1, step + 100 * seed + 50)[0].float()
    lm[:, list(HOT)] = lm[:, list(reversed(HOT))]
    return model, (lm * 0.5).to(tdtype(dtype_name))


def new_state():
    bbsz, L1, LT = BSZ * BEAM, MAX_LEN + 1, MAX_LEN + 2
    tokens = torch.full((bbsz, LT), PAD, dtype=torch.long)
    tokens[:, 0] = EOS
    anc = torch.zeros(bbsz, L1, dtype=torch.int32)
    anc[:, 0] = torch.arange(bbsz, dtype=torch.int32)
    return dict(tokens=tokens, scores=torch.zeros(bbsz, L1, dtype=torch.float64), anc=anc,
                ignore=torch.zeros(BSZ, BEAM, dtype=torch.uint8), finished=torch.zeros(BSZ, dtype=torch.uint8),
                nfinal=torch.zeros(BSZ, dtype=torch.int32), fin_tokens=torch.zeros(BSZ, BEAM, L1, dtype=torch.long),
                fin_score=torch.zeros(BSZ, BEAM, dtype=torch.float64), fin_len=torch.zeros(BSZ, BEAM, dtype=torch.int32), min_gap=math.inf)


def masked(st, lp, s, ngram=0, prefix=None, min_len=1, unk_penalty=0.0):
    """The generator's masks, in its order, on lp' [bbsz, V] (changed in place and returned).  Where the prefix holds eos the sentence's
    first row is copied over its rows in st and in lp', as the reference does."""
    beam = BEAM
    st["copies"] = set()  # sentences whose rows are copies of the first at this step: their candidates tie exactly, by construction
    lp[lp != lp] = -math.inf
    lp[:, PAD] = -math.inf
    lp[:, UNK] -= unk_penalty
    if s >= MAX_LEN:
        lp[:, :EOS] = -math.inf
        lp[:, EOS + 1:] = -math.inf
    if prefix is not None and s < prefix.size(1) and s < MAX_LEN:
        for b in range(BSZ):
            t = int(prefix[b, s])
            rows = slice(b * beam, (b + 1) * beam)
            if t != PAD:
                keep = lp[rows, t].clone()
                lp[rows] = -math.inf
                lp[rows, t] = keep
            if t == EOS:
                st["copies"].add(b)
                lp[rows] = lp[b * beam].clone()
                for name in ("tokens", "scores", "anc"):
                    st[name][rows] = st[name][b * beam].clone()
    elif s < min_len:
        lp[:, EOS] = -math.inf
    if ngram:
        tk_all = st["tokens"].tolist()
        for h in range(lp.size(0)):
            ban = sorted(set(banned_tokens(tk_all[h], s, ngram)))
            if ban:
                lp[h, torch.tensor(ban)] = -math.inf
    return lp


def fused_step_lprobs(model, lm, w, T=1.0, dt=torch.float64):
    """lp' of one step from search_logits()' (model, lm)."""
    return fused_lprobs(torch.stack(model, 0), lm, w, T, dt)


def select_step(st, lp, s):
    """Top 2 * beam of the masked lp' + cumulative scores per sentence and the bookkeeping of the beam step (sequence_generator.py
    :340-499) on st, in fp64.  st["min_gap"] collects the smallest difference between neighbours among each sentence's first
    2 * beam + 1 candidates (finite ones): the margin the exact ids hang on (where the prefix holds eos the sentence's rows are copies of
    one row and their candidates tie exactly; those ties are decided by the flat index, not by rounding, and are left out)."""
    bbsz, V = lp.shape
    beam, K = BEAM, 2 * BEAM
    tokens, scores, anc = st["tokens"], st["scores"], st["anc"]
    cand = lp.view(BSZ, beam, V)[:, :1].reshape(BSZ, -1) if s == 0 else (lp + scores[:, s - 1:s]).view(BSZ, -1)
    val, order = torch.sort(cand, dim=1, descending=True, stable=True)
    for b in range(BSZ):
        if not bool(st["finished"][b]):
            top = val[b, :K + 1]
            top = top[torch.isfinite(top)]
            if b in st.get("copies", ()):  # (equal rows: the ties go to the smaller flat index on both sides)
                top = torch.unique(top).flip(0)
            if top.numel() > 1:
                st["min_gap"] = min(st["min_gap"], float((top[:-1] - top[1:]).min()))
    order, c_score = order[:, :K], val[:, :K]
    c_tok, c_beam = order % V, order // V
    new_tokens, new_scores, new_anc = tokens.clone(), scores.clone(), anc.clone()
    for b in range(BSZ):
        ign = st["ignore"][b].tolist()
        was_finished, nf = bool(st["finished"][b]), int(st["nfinal"][b])
        em, any_top_eos = [], False
        for k in range(K):
            e = int(c_tok[b, k]) == EOS and float(c_score[b, k]) != -math.inf and not (k < beam and ign[k])
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
        st["ignore"][b] = torch.tensor([1 if i >= len(live) else 0 for i in range(beam)], dtype=torch.uint8)
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


SEARCH_VARIANTS = {"plain": (0, False), "ngram2_prefix": (2, True)}  # (no_repeat_ngram_size, with the ragged prefix)
# every dispatch family x N = 1, 2 plain; the constrained variant at V = 1003 and 10 000
SEARCH_PARAMS = [(dt, V, N, "plain") for dt, V in SEARCH_CASES for N in (1, 2)] + \
                [(dt, V, N, "ngram2_prefix") for dt, V in SEARCH_CASES if V in (1003, 10000) for N in (1, 2)]


def run_restatement(dtype_name, V, N, variant="plain", w=W, seed=SEARCH_SEED, steps=STEPS):
    """`steps` steps of the fused search by the fp64 restatement alone: the states after every step and the final one."""
    ngram, with_prefix = SEARCH_VARIANTS[variant]
    prefix = torch.tensor(PREFIX) if with_prefix else None
    st, states = new_state(), []
    for s in range(steps):
        model, lm = search_logits(dtype_name, V, N, s, seed)
        lp = masked(st, fused_step_lprobs(model, lm, w), s, ngram=ngram, prefix=prefix)
        select_step(st, lp, s)
        states.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()})
    return st, states


# ---- the whole search over any lp_fn, and the LM on the CPU (for the fixture) ------------------------------------------------------------
def search(lp_fn, B, beam, max_len, len_penalty=1.0, unk_penalty=0.0, ngram=0, pad=PAD, eos=EOS, unk=UNK):
    """The reference's beam search (min_len 1, normalised scores) per sentence over lp_fn(sentence, tokens[beam, step + 1]) -> [beam, V]
    fp32 log-probabilities BEFORE the masks (with shallow fusion: lp').  Returns (hypotheses per sentence, best first: dict(tokens,
    score, positional_scores), the smallest top-2*beam boundary gap of any step)."""
    results, min_gap = [], math.inf
    for b in range(B):
        tokens = torch.full((beam, max_len + 2), pad, dtype=torch.long)
        tokens[:, 0] = eos
        scores = torch.zeros(beam, max_len + 1)
        fin = []
        for step in range(max_len + 1):
            lp = lp_fn(b, tokens[:, :step + 1]).clone()
            lp[lp != lp] = -math.inf
            lp[:, pad] = -math.inf
            lp[:, unk] -= unk_penalty
            if step >= max_len:
                lp[:, :eos] = -math.inf
                lp[:, eos + 1:] = -math.inf
            if step < 1:
                lp[:, eos] = -math.inf
            if ngram:
                for h, tk in enumerate(tokens.tolist()):
                    ban = sorted(set(banned_tokens(tk, step, ngram)))
                    if ban:
                        lp[h, torch.tensor(ban)] = -math.inf
            V = lp.size(-1)
            cand = lp[0:1] if step == 0 else lp + scores[:, step - 1].unsqueeze(-1)
            top_s, top_i = torch.topk(cand.reshape(-1), k=2 * beam + 1)
            if top_s[2 * beam] != -math.inf:
                min_gap = min(min_gap, float(top_s[2 * beam - 1] - top_s[2 * beam]))
            top_s, top_i = top_s[:2 * beam], top_i[:2 * beam]
            beams, idx = top_i // V, top_i.fmod(V)
            eos_mask = idx.eq(eos) & top_s.ne(-math.inf)
            for j in range(beam):
                if eos_mask[j] and len(fin) < beam:
                    bi = int(beams[j])
                    pos = torch.cat([scores[bi, :step], top_s[j:j + 1]])
                    pos[1:] = pos[1:] - pos[:-1].clone()
                    fin.append(dict(tokens=torch.cat([tokens[bi, 1:step + 1], torch.tensor([eos])]),
                                    score=float(top_s[j]) / ((step + 1) ** len_penalty), positional_scores=pos))
            if len(fin) >= beam or step >= max_len:
                break
            keep = [j for j in range(2 * beam) if not eos_mask[j]][:beam]
            kb = beams[keep]
            new_tokens, new_scores = tokens[kb].clone(), scores[kb].clone()
            new_tokens[:, step + 1] = idx[keep]
            new_scores[:, step] = top_s[keep]
            tokens, scores = new_tokens, new_scores
        fin.sort(key=lambda h: -h["score"])
        results.append(fin)
    return results, min_gap


def lm_forward(p, tokens, heads, layers, scale=True):
    """Logits [B, T, V] of a pre-norm Transformer LM (TransformerDecoder without encoder attention, ReLU, final LayerNorm; parameters
    under the reference's names `decoder.*`) on the CPU, through the oracle's attention and LayerNorm."""
    from oracle import chimera_oracle as O
    emb = p["decoder.embed_tokens.weight"]
    d = emb.size(1)
    x = (math.sqrt(d) if scale else 1.0) * torch.nn.functional.embedding(tokens, emb) + O.positional_embedding(tokens, d, PAD)
    x = x.transpose(0, 1)
    U = x.size(0)
    causal = torch.triu(torch.full((U, U), -math.inf), 1)
    for i in range(layers):
        pre = "decoder.layers.%d." % i
        h = O.layer_norm(x, p[pre + "self_attn_layer_norm.weight"], p[pre + "self_attn_layer_norm.bias"])
        x = x + O.mha(p, pre + "self_attn.", h, h, h, heads, None, causal)
        h = O.layer_norm(x, p[pre + "final_layer_norm.weight"], p[pre + "final_layer_norm.bias"])
        x = x + O.linear(torch.relu(O.linear(h, p[pre + "fc1.weight"], p[pre + "fc1.bias"])), p[pre + "fc2.weight"], p[pre + "fc2.bias"])
    x = O.layer_norm(x, p["decoder.layer_norm.weight"], p["decoder.layer_norm.bias"]).transpose(0, 1)
    return x.matmul(p.get("decoder.output_projection.weight", emb).t())
