"""Device-resident beam search over the incremental decoder — the MI355X-native form of the decode loop of
fairseq/sequence_generator.py:_generate (:179-541).

The reference runs, per generated token, ~70 module calls, a K/V-cache `index_select` per layer
(multihead_attention.py:419-437) and several host synchronisations (`.any()`, `masked_select`, Python lists of
finalized hypotheses).  At batch x beam = 160 rows the arithmetic of a step is a few microseconds per kernel, so the
loop is launch- and sync-bound.  Here one decode step is a FIXED sequence of C-ABI launches whose only step-dependent
input is a device-side counter:

    cst_dec_embed -> per layer [LN, packed QKV GEMM, cst_dec_self_attn (append-only caches + ancestry table), out-proj
    GEMM (+residual), LN, q GEMM, cst_attn_fwd over the per-SENTENCE encoder K/V (beam rows are the query "time" axis, so
    the encoder K/V are neither replicated nor reordered), out-proj GEMM (+residual), LN, fc1 GEMM (+bias+act), fc2 GEMM
    (+bias+residual)] -> LN -> vocabulary GEMM -> cst_beam_step (log-softmax, masks, top-2*beam, finalisation, next rows)

(decoder-only members — language models decoded from prompts — have no cross block: their layers are the LM member's of shallow fusion.)
The sequence is captured once per (batch, encoder length) in a HIP graph and replayed; the host reads one int32
(`num_remaining`) every `poll` steps.  Results are the reference's: same candidates, same finalisation order, same
scores (tests/test_decode_engine_gpu.py checks token ids bit-exactly against the reference's SequenceGenerator fixtures
and against the module-by-module mirror path).

Three records describe an engine: DecodeOptions (what to search for: the options part of the state key and of cst_beam_desc), Switches
(the CST_DEC_* environment, read once) and, per member and row count, StepPlan (which launches a layer is made of)."""
import ctypes
import dataclasses
import os
from typing import NamedTuple, Optional

import torch

from . import kernels as K
from . import lib as L
from .optim import PARAM_EPOCH


@dataclasses.dataclass(frozen=True)
class DecodeOptions:
    """The search a BeamDecodeEngine runs.  Every field is a parameter of cst_beam_step baked into the captured step graph (or sizes the
    state), so the record itself — frozen, hashable — is the options part of the state key, and fill() writes it into a cst_beam_desc."""
    beam: int
    max_len: int
    min_len: int = 1
    normalize_scores: bool = True
    len_penalty: float = 1.0
    unk_penalty: float = 0.0
    temperature: float = 1.0
    no_repeat_ngram_size: int = 0         # --no-repeat-ngram-size (0 = off: the row kernels without the constraint code)
    sampling: bool = False                # --sampling / --sampling-topk / --sampling-topp: one draw per row instead of the top 2 * beam
    topk: int = 0
    topp: float = 0.0
    diverse_groups: int = 0               # --diverse-beam-groups / --diverse-beam-strength (sequence_generator.DiverseBeamSearch)
    diverse_strength: float = 0.0
    sibling_rate: Optional[float] = None  # --diversity-rate (DiverseSiblingsSearch); None = off, 0 is a legal rate
    lm_weight: float = 0.0                # --lm-weight: the factor of the language model's log-softmax (shallow fusion)

    def __post_init__(self):
        opt = lambda f: lambda v: None if v is None else f(v)
        floor0 = lambda f: lambda v: max(f(v), f(0))
        norm = dict(beam=int, max_len=int, min_len=int, normalize_scores=bool, len_penalty=float, unk_penalty=float, temperature=float,
                    no_repeat_ngram_size=int, sampling=bool, topk=floor0(int), topp=floor0(float), diverse_groups=floor0(int),
                    diverse_strength=float, sibling_rate=opt(float), lm_weight=float)
        for name, f in norm.items():
            object.__setattr__(self, name, f(getattr(self, name)))
        assert self.no_repeat_ngram_size == 0 or self.no_repeat_ngram_size >= 2, "no_repeat_ngram_size is 0 (off) or at least 2"

    def fill(self, d, members):
        """Write the options into the cst_beam_desc `d` of a step over `members` models.  A strategy that is off leaves its fields at
        zero: the step then launches the instantiations without it.  cst_beam_step refuses bad values and combinations."""
        d.beam, d.max_len, d.min_len = self.beam, self.max_len, self.min_len
        d.unk_penalty, d.len_penalty, d.temperature = self.unk_penalty, self.len_penalty, self.temperature
        d.normalize_scores = int(self.normalize_scores)
        d.members = members if members > 1 else 0  # 0: the single-matrix kernels
        d.no_repeat_ngram = self.no_repeat_ngram_size
        if self.sampling:
            d.sampling, d.sample_topk, d.sample_topp = 1, self.topk, self.topp
        if self.diverse_groups > 0:
            d.diverse_groups, d.diverse_strength = self.diverse_groups, self.diverse_strength
        if self.sibling_rate is not None:
            d.diverse_siblings, d.sibling_rate = 1, self.sibling_rate


class Switches(NamedTuple):
    """The engine's CST_DEC_* environment switches, read once when an engine is built."""
    cross_kernel: str
    lanes: int
    no_ln_fuse: bool
    no_splitk: bool
    no_qcross: bool

    @classmethod
    def read(cls, cross_kernel=None, lanes=None):
        """Arguments that are not None win over the environment."""
        env = os.environ
        return cls(env.get("CST_DEC_CROSS_KERNEL", "auto") if cross_kernel is None else cross_kernel,
                   max(1, int(env.get("CST_DEC_LANES", "1") if lanes is None else lanes)),
                   bool(env.get("CST_DEC_NO_LN_FUSE")), bool(env.get("CST_DEC_NO_SPLITK")), bool(env.get("CST_DEC_NO_QCROSS")))


class StepPlan(NamedTuple):
    """Which launches one layer of a member is made of (BeamDecodeEngine._plan decides, everything else reads)."""
    cross: bool                # the layers have a cross-attention block (a language model's have none)
    fuse_ln: bool              # the layer's LayerNorms run inside the projections behind them (cst_dec_ln_linear)
    cross_mode: Optional[str]  # "flash" | "flash_hm" | "shared"; None without a cross block
    q_in_cross: bool           # the query projection runs inside the cross-attention launch (cst_dec_ln_q_cross_attn)
    split_fc2: bool            # fc2 as eight K slices + the reduce launch

    @property
    def head_major(self):
        """The encoder K/V are stored head-major [bsz, H, S, D]."""
        return self.cross_mode in ("shared", "flash_hm")

    @property
    def layer_nodes(self):
        """Launches per layer: (LayerNorm, qkv, self-attention, out, LayerNorm, fc1, fc2) + the cross block's (LayerNorm, q, cross
        attention, out); a folded LayerNorm and a query projection inside the attention launch are no launches, the split-K reduce is."""
        n = (5 if self.fuse_ln else 7) + self.split_fc2
        return n + ((3 if self.fuse_ln else 4) - self.q_in_cross if self.cross else 0)


class BeamDecodeEngine:
    def __init__(self, decoders, tgt_dict, options, lm_decoder=None, use_graph=True, poll=8, cross_kernel=None, lanes=None, lexical=None, attention=False):
        # `decoders`: the list of models of a checkpoint ensemble (--path a.pt:b.pt:c.pt; one model is a list of one).  A language model
        # (shallow fusion, --lm-path / --lm-weight, sequence_generator.py:318-324) is one more decoder of the step: a decoder WITHOUT
        # cross attention (lm_supported) whose log-softmax cst_beam_step_lm adds, x lm_weight, to the models' combined log-probabilities.
        # MEMBERS = the models in order, then the LM.  Every member keeps its own packed weights, activations, K/V caches, encoder K/V
        # and logits buffer; the beam state (tokens / scores / ancestry, step counter, finalized hypotheses) is shared — all members
        # follow the same hypotheses, so one ancestry table serves every member's append-only caches.  Three parallel lists in member
        # order: self.members (decoders), _pack() (weights), st["members"] (buffers).
        # INVARIANT: packed weights, states and member dicts hold no reference to the engine, to their state or to each other — no
        # cycles, so a dropped state is freed by reference counting at once and not by the cyclic collector, which could otherwise run
        # inside a later graph capture.
        # `lexical`: None | "ordered" | "unordered" — the representation of the lexical constraints a generate() call may bring
        # (sequence_generator.LexicallyConstrainedBeamSearch; cst_lex_init / cst_beam_step_lex).  A call without constraints runs the
        # engine as if it were None.
        # `attention` (--print-alignment): keep the last decoder layer's head-averaged cross attention of every step and return it with
        # the hypotheses.  Like `lexical` it is the engine's, not an option of cst_beam_desc: it sizes the state (the attention history
        # and the finalised hypotheses' ancestry rows), so an engine is built with it or without it.  Off: every launch, graph node,
        # buffer and result is what it is without the feature.
        self.opt = options
        self.attention = bool(attention)
        assert lexical in (None, "ordered", "unordered"), lexical
        assert lexical is None or not (options.sampling or options.diverse_groups > 0 or options.sibling_rate is not None), \
            "sampling, the diverse strategies and lexical constraints are mutually exclusive search strategies"
        self.lexical = lexical
        self.decs, self.lm = list(decoders), lm_decoder
        assert 1 <= len(self.decs) <= 8, "cst_beam_step combines at most 8 ensemble members"
        # DECODER-ONLY: every model is itself a language model (lm_supported: no cross block in any layer) — generation from LM prompts
        # (fairseq_interactive.py --task language_modeling).  Such members have no encoder K/V, no cross launches and no per-call
        # projection (_begin_member); the state key carries no source length.  The step is otherwise the same sequence: every member's
        # layers up to its logits, then cst_beam_step over them (an ensemble of LMs is averaged like any other).
        n_lm = sum(1 for d in self.decs if all(getattr(l, "encoder_attn", None) is None for l in d.layers))
        if n_lm not in (0, len(self.decs)):
            raise ValueError("an ensemble mixes %d decoder-only language models with %d encoder-decoder models: the members must be of "
                             "one kind" % (n_lm, len(self.decs) - n_lm))
        self.decoder_only = n_lm > 0
        assert not self.decoder_only or all(self.lm_supported(d) for d in self.decs), "a language model's decoder is outside lm_supported()"
        if self.decoder_only and lm_decoder is not None:
            raise ValueError("shallow fusion (lm_decoder) into a model that is itself a language model is not built: decode the two as an ensemble")
        if self.decoder_only and attention:
            raise ValueError("attention (--print-alignment) needs cross attention: a decoder-only language model has none")
        assert self.lm is None or self.lm_supported(self.lm), "the language model's decoder is outside lm_supported()"
        assert self.lm is None or self.lm.output_projection.weight.shape[0] == len(tgt_dict), "the LM's vocabulary must be the target dictionary"
        self.members = self.decs + ([self.lm] if self.lm is not None else [])
        self.pad, self.unk, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos()
        self.vocab = len(tgt_dict)
        self.use_graph, self.poll = use_graph, max(1, int(poll))
        # cross_kernel — cross attention per step: "flash" = cst_attn_fwd with batch = sentence and the beam rows as the query axis
        # (37 us per layer at 32 x beam 5 x 750 source positions, bf16); "flash_hm" = the same kernel over head-major K/V (contiguous
        # per-head streams: no faster, 0.811 vs 0.812 ms per step); "shared" = cst_dec_cross_attn (VALU kernel, one pass with online
        # softmax, K/V rows shared by the beam: ~59 us — the 5 queries' dot products per key cost more than the MFMA tile the
        # flash kernel spends on them; kept selectable, covered by the same tests)
        # "auto" (round 5): "shared" where cst_dec_cross_attn runs its matrix-core kernel (bf16, head dim 64, beam <= 32: the four waves
        # of a (sentence, head) workgroup split the keys, 21.5 us per layer against 26.4 for "flash" on s2t_transformer_l), else "flash"
        self.sw = Switches.read(cross_kernel, lanes)
        assert self.sw.cross_kernel in ("auto", "flash", "flash_hm", "shared")
        # lanes: the batch may be cut into groups of sentences, each with its own state, step graph and HIP stream, replayed side by
        # side (sentences never interact in beam search: same hypotheses, tests/test_decode_engine_gpu.py).  Measured on MI355X
        # (32 x beam 5, s2t_transformer_l): 1 lane 0.877 ms per step, 2 lanes 0.910, 3 lanes 1.60, 4 lanes 1.63 — the step graphs of
        # different streams do not overlap on this stack (a half-batch step costs 0.455 ms, two of them 0.91), so the default is 1.
        # (sampling: the index of a draw holds the sentence's position in the WHOLE batch)
        self.lanes = 1 if self.opt.sampling else self.sw.lanes
        self._packed = None
        self._state = {}
        self._cfg = None
        self._streams = []

    lm_weight = property(lambda self: self.opt.lm_weight)  # (read-only, next to .decs and .lm)

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _supported(decoder, cross):
        try:
            ok = (decoder.embed_positions is not None and decoder.layernorm_embedding is None and decoder.project_in_dim is None
                  and decoder.project_out_dim is None and decoder.adaptive_softmax is None and len(decoder.layers) > 0)
            if not cross:
                ok = ok and hasattr(decoder.embed_positions, "get_embedding")  # sinusoidal positions
            for l in decoder.layers:
                ok = ok and l.normalize_before and (l.encoder_attn is not None) == cross and l.self_attn.head_dim in (32, 64)
                ok = ok and l.self_attn.q_proj.bias is not None and (not cross or l.encoder_attn.head_dim == l.self_attn.head_dim)
            return bool(ok)
        except AttributeError:
            return False

    @staticmethod
    def supported(decoder):
        """The fused loop covers the configuration every Chimera / s2t_transformer arch uses: pre-norm layers, sinusoidal
        positions, encoder attention in every layer, no layernorm_embedding / project_in / adaptive softmax."""
        return BeamDecodeEngine._supported(decoder, True)

    @staticmethod
    def lm_supported(decoder):
        """supported() for a language model: the same decoder without encoder attention in any layer."""
        return BeamDecodeEngine._supported(decoder, False)

    @staticmethod
    def sampling_supported(vocab, dtype):
        """cst_beam_step samples in its register-resident row kernels: at most 5 * 512 16-byte vectors per row (20480 symbols in bf16,
        10240 in fp32).  Beyond that it returns CST_ERR_UNSUPPORTED, so the generator takes the host loop up front."""
        vec = 8 if dtype == torch.bfloat16 else 4
        return -(-(-(-int(vocab) // vec)) // 512) <= 5

    @staticmethod
    def lexical_supported(packed, beam):
        """cst_lex_init holds at most 32 constraint tokens per sentence and lists at most 16 next tokens per state; beyond that, or
        with packed rows wider than 32 one-token constraints need (65), cst_lex_init returns CST_ERR_UNSUPPORTED, so the generator takes the host loop up
        front.  packed: the int64 [bsz, W] tensor of lexical_constraints.pack_constraints."""
        from . import lexical_constraints as LC
        return beam <= 20 and int(packed.shape[1]) <= L.LEX_WIDTH_MAX and LC.device_limits_ok(packed)

    def invalidate(self):
        """Drop the packed / folded weight copies and the captured graphs (call after changing decoder weights by any other route)."""
        self._packed = None
        self._state.clear()

    def _plan(self, dec, dtype, rows=None):
        """The StepPlan of member `dec` at `rows` hypothesis rows — the ONLY place where these decisions are made.  rows None: what holds
        for any row count up to 1024 (the weights to pack; nodes_per_step's default): LayerNorms folded where they can be, no split."""
        bf16, C, l0 = dtype == torch.bfloat16, dec.embed_dim, dec.layers[0]
        D, cross = l0.self_attn.head_dim, l0.encoder_attn is not None
        matrix_core = bf16 and D == 64 and self.opt.beam <= 32  # cst_dec_cross_attn's matrix-core kernel
        fuse_ln = bf16 and C % 512 == 0 and (rows is None or rows <= 1024) and not self.sw.no_ln_fuse
        mode = None if not cross else self.sw.cross_kernel if self.sw.cross_kernel != "auto" else "shared" if matrix_core else "flash"
        # fc2 (K = 4096) at <= 256 rows: 48 workgroups would stream 170 KB of weights each through a 48 KB ring — 23.7 us; eight K
        # slices + the reduce launch: 15.3 us although it is a node more (tools/bench_dec_splitk.py; K = 1024 projections lose with any
        # split).  bf16 only: the fp32 parity configuration keeps the summation order of the module path it is compared with.
        split_fc2 = bf16 and rows is not None and rows <= 256 and l0.fc1.out_features >= 4096 and not self.sw.no_splitk
        return StepPlan(cross, fuse_ln, mode, fuse_ln and mode == "shared" and matrix_core and not self.sw.no_qcross, split_fc2)

    def nodes_per_step(self, dtype, rows=None):
        """Kernel launches (graph nodes) of one decode step: every member's sequence up to its vocabulary projection, then ONE pair of
        beam-search kernels over the members' logits.  With `attention` every MODEL member's last layer adds cst_attn_avg_probs,
        and the query projection it reads where the plan otherwise runs that inside the cross-attention launch."""
        n = sum(self._member_nodes(dec, dtype, rows) for dec in self.members) + 2
        if self.attention:
            n += sum(1 + self._plan(dec, dtype, rows).q_in_cross for dec in self.decs)
        return n

    def _member_nodes(self, dec, dtype, rows):
        """embed + the layers (StepPlan.layer_nodes) + final LayerNorm + vocabulary projection."""
        return 1 + self._plan(dec, dtype, rows).layer_nodes * len(dec.layers) + (1 if dec.layer_norm is not None else 0) + 1

    def _pack(self, dtype, device):
        """Per member: per layer the packed [3C, C] self-attention projection and the LayerNorm-folded weights the plan asks for, and the
        position table (weights are constants in eval mode).  Returns the list in member order."""
        # weights may have been updated since the last call (training between validations): re-pack and drop the graphs
        # (autograd versions catch load_state_dict / copy_; optim.PARAM_EPOCH catches the fused optimizer's raw-pointer updates)
        key = (dtype, device, PARAM_EPOCH[0], tuple((p.data_ptr(), p._version) for dec in self.members for p in dec.parameters()))
        if self._packed is None or self._packed[0] != key:
            self._state.clear()
            self._packed = (key, [self._pack_member(dec, dtype, device) for dec in self.members])
        return self._packed[1]

    def _pack_member(self, dec, dtype, device):
        layers = []
        plan = self._plan(dec, dtype)
        for l in dec.layers:
            sa, ca = l.self_attn, l.encoder_attn
            d = dict(
                wqkv=torch.cat((sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight), 0).detach().contiguous(),
                bqkv=torch.cat((sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias), 0).detach().contiguous())
            if plan.fuse_ln:  # LayerNorm folded into the projection that follows it (include/cst.h: cst_dec_ln_linear)
                d["ln_qkv"] = self._fold_ln(l.self_attn_layer_norm, d["wqkv"], d["bqkv"])
                d["ln_fc1"] = self._fold_ln(l.final_layer_norm, l.fc1.weight, l.fc1.bias)
                if plan.cross:
                    d["ln_q"] = self._fold_ln(l.encoder_attn_layer_norm, ca.q_proj.weight, ca.q_proj.bias)
                if plan.q_in_cross:
                    d["ln_q_frag"] = self.fragment_major(d["ln_q"][0], ca.num_heads)  # cst_dec_ln_q_cross_attn's weight layout
                    assert d["ln_q_frag"] is not None
            layers.append(d)
        pos = dec.embed_positions
        need = dec.padding_idx + 2 + self.opt.max_len + 1
        table = pos.get_embedding(need, pos.embedding_dim, pos.padding_idx).to(device=device, dtype=torch.float32).contiguous()
        # the module path adds positions converted to the storage dtype (models/transformer.py:756 on a .half()/bf16 model)
        if dtype != torch.float32:
            table = table.to(dtype).float()
        return dict(layers=layers, pos=table)

    @staticmethod
    def _fold_ln(ln, w, b):
        """(Wg, sg, sb) of cst_dec_ln_linear: gamma folded into the weight columns (one bf16 rounding), beta and the bias into sb."""
        wf = w.detach().float()
        wg = (wf * ln.weight.detach().float().unsqueeze(0)).to(w.dtype).contiguous()
        sg = wg.float().sum(dim=1).contiguous()
        sb = (wf * ln.bias.detach().float().unsqueeze(0)).sum(dim=1).contiguous()  # (a row-wise sum, not `wf @ beta`: no vendor BLAS in the package)
        if b is not None:
            sb = (sb + b.detach().float()).contiguous()
        return wg, sg, sb, float(ln.eps)

    @staticmethod
    def fragment_major(wg, H):
        """[H*64, K] -> the fragment-major packing of include/cst.h (cst_dec_ln_q_cross_attn): [H][2][K/16][2][32][8]."""
        N, K = wg.shape
        if N != H * 64 or K % 16:
            return None
        return wg.view(H, 2, 32, K // 16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous()

    # ------------------------------------------------------------------------------------------------------------
    def _alloc_member(self, dec, bsz, S, dtype, device, has_mask):
        """One member's own buffers and its plan: activations, logits, append-only self-attention caches and — with a cross block — the
        query, the per-sentence encoder K/V and their padding mask."""
        beam, L1 = self.opt.beam, self.opt.max_len + 1
        bbsz, C, nl = bsz * beam, dec.embed_dim, len(dec.layers)
        z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=device)
        plan = self._plan(dec, dtype, bbsz)
        m = dict(
            plan=plan, x=z(bbsz, C), x2=z(bbsz, C), h=z(bbsz, C), qkv=z(bbsz, 3 * C), attn=z(bbsz, C), f=z(bbsz, dec.layers[0].fc1.out_features),
            logits=z(bbsz, (self.vocab + 7) // 8 * 8), mean=z(bbsz, dt=torch.float32), rstd=z(bbsz, dt=torch.float32),
            kc=[z(bbsz, L1, C) for _ in range(nl)], vc=[z(bbsz, L1, C) for _ in range(nl)],
            gemm_ws=z(8 * bbsz * C * 4, dt=torch.uint8) if plan.split_fc2 else None)  # split-K partials of the fc2 projection (own buffer: captured)
        if plan.cross:
            m.update(q=z(bbsz, C), lse=z(bsz * 64 * beam, dt=torch.float32), kx=[z(bsz, S, C) for _ in range(nl)],
                     vx=[z(bsz, S, C) for _ in range(nl)], proj=z(bsz * S, C), kpm=z(bsz, S, dt=torch.uint8) if has_mask else None)
        return m

    def _alloc(self, lane, bsz, S, dtype, device, has_mask, prefix_len=0, lex=None):
        """S / has_mask: one value per model (models may differ in encoder output length).  prefix_len and the options are kernel
        parameters baked into the captured graph, so they are part of the state key; the prefix TOKENS and the sampling key live in
        buffers the state owns (st["prefix"], st["sample_key"]), which every call overwrites: a replayed graph reads the new call's."""
        # lex: None or (representation, width of the packed constraints) — the step then is cst_beam_step_lex over a workspace and a
        # constraint buffer of the lane's own (st["lex_packed"], refilled by every call like st["prefix"]).
        key = (lane, bsz, S, dtype, device, has_mask, prefix_len, self.opt, lex)
        st = self._state.get(key)
        if st is not None:
            return st
        beam, L1, LT = self.opt.beam, self.opt.max_len + 1, self.opt.max_len + 2
        bbsz = bsz * beam
        z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=device)
        st = dict(
            step=z(1, dt=torch.int32), num_remaining=z(1, dt=torch.int32),
            tokens=z(2, bbsz, LT, dt=torch.int64), scores=z(2, bbsz, L1, dt=torch.float32), anc=z(2, bbsz, L1, dt=torch.int32),
            ignore=z(bsz, beam, dt=torch.uint8), finished=z(bsz, dt=torch.uint8), nfinal=z(bsz, dt=torch.int32),
            fin_tokens=z(bsz, beam, L1, dt=torch.int64), fin_pos=z(bsz, beam, L1, dt=torch.float32),
            fin_score=z(bsz, beam, dt=torch.float32), fin_len=z(bsz, beam, dt=torch.int32), graph=None, lm_desc=None,
            beam_ws=torch.zeros(L.load().cst_beam_workspace(bsz, beam), dtype=torch.uint8, device=device),
            prefix=torch.full((bsz, prefix_len), self.pad, dtype=torch.int64, device=device) if prefix_len > 0 else None,
            sample_key=z(1, dt=torch.int32) if self.opt.sampling else None)  # (the 32 bits of the key; the kernel reads them unsigned)
        if self.attention:
            # attn_hist[row, s, :]: the head-averaged cross attention row `row` computed at step s (append-only like the K/V caches: a
            # hypothesis' column j is attn_hist[anc[j], j, :]); fin_anc: the ancestry row of every finalised hypothesis (cst_beam_desc)
            st.update(attn_hist=z(bbsz, L1, S[0], dt=torch.float32), fin_anc=z(bsz, beam, L1, dt=torch.int32))
        if self.decoder_only:  # (S and has_mask are None)
            ms = [self._alloc_member(dec, bsz, 0, dtype, device, False) for dec in self.decs]
        else:
            ms = [self._alloc_member(dec, bsz, s, dtype, device, hm) for dec, s, hm in zip(self.decs, S, has_mask)]
        if self.lm is not None:
            ms.append(self._alloc_member(self.lm, bsz, 0, dtype, device, False))
            f = L.LmFusionDesc()
            f.lm_logits, f.lm_weight, f.lprobs_out = ms[-1]["logits"].data_ptr(), self.opt.lm_weight, None
            st["lm_desc"] = f
        st["members"] = ms
        d = L.BeamDesc()
        self.opt.fill(d, len(self.decs))
        d.dtype = L.dtype_code(dtype)
        d.bsz, d.vocab = bsz, self.vocab
        d.pad, d.unk, d.eos = self.pad, self.unk, self.eos
        d.logits, d.ld_logits = ms[0]["logits"].data_ptr(), ms[0]["logits"].stride(0)
        for i, m in enumerate(ms[1:len(self.decs)]):
            d.logits_n[i] = m["logits"].data_ptr()
        d.step, d.tokens, d.scores, d.anc = (st[k].data_ptr() for k in ("step", "tokens", "scores", "anc"))
        d.cands_to_ignore, d.finished, d.nfinal = st["ignore"].data_ptr(), st["finished"].data_ptr(), st["nfinal"].data_ptr()
        d.num_remaining = st["num_remaining"].data_ptr()
        d.fin_tokens, d.fin_pos, d.fin_score, d.fin_len = (st[k].data_ptr() for k in ("fin_tokens", "fin_pos", "fin_score", "fin_len"))
        d.workspace = st["beam_ws"].data_ptr()
        if prefix_len > 0:
            d.prefix_tokens, d.prefix_len = st["prefix"].data_ptr(), prefix_len
        if self.opt.sampling:
            d.sample_key = st["sample_key"].data_ptr()
        if self.attention:
            d.fin_anc = st["fin_anc"].data_ptr()
        st["desc"] = d
        st["lex_desc"] = None
        if lex is not None:
            from .lexical_constraints import REPRESENTATIONS
            x = L.LexDesc()
            st["lex_packed"] = torch.zeros(bsz, lex[1], dtype=torch.int64, device=device)
            st["lex_ws"] = torch.zeros(L.load().cst_lex_workspace(bsz, beam, lex[1]), dtype=torch.uint8, device=device)
            x.representation, x.width = REPRESENTATIONS[lex[0]], lex[1]
            x.constraints, x.workspace = st["lex_packed"].data_ptr(), st["lex_ws"].data_ptr()
            st["lex_desc"] = x
        self._state[key] = st
        return st

    # ------------------------------------------------------------------------------------------------------------
    def _linear(self, x, w, b, out, act=L.ACT_NONE, resid=None, ws=None):
        """out = act(x w^T + b) + resid.  ws: the split-K scratch — given (by fc2 where the plan splits it), the GEMM is split 8 ways."""
        M, Kd = x.shape
        K.gemm(x, w, out, M, w.shape[0], Kd, a_kmajor=1, b_kmajor=1, lda=Kd, ldb=Kd, ldc=out.stride(0), bias=b, act=act,
               resid=resid, ld_resid=0 if resid is None else resid.stride(0), split_k=1 if ws is None else 8, ws=ws)

    def _ln_linear(self, x, folded, out, act=L.ACT_NONE):
        wg, sg, sb, eps = folded
        M, Kd = x.shape
        L.check(L.load().cst_dec_ln_linear(L.ptr(x), L.ptr(wg), L.ptr(sg), L.ptr(sb), eps, None, L.ptr(out), M, wg.shape[0], Kd,
                                           x.stride(0), 0, out.stride(0), act, None, 0, L.dtype_code(x.dtype), L.stream_ptr()),
                "cst_dec_ln_linear")

    def _ln(self, x, ln, out, m):
        L.check(L.load().cst_layernorm_fwd(L.ptr(x), None, L.ptr(ln.weight), L.ptr(ln.bias), L.ptr(out), None, L.ptr(m["mean"]),
                                           L.ptr(m["rstd"]), x.shape[0], x.shape[1], ln.eps, L.dtype_code(x.dtype), L.stream_ptr()),
                "cst_layernorm_fwd")

    def _step(self, st, pk, bsz):
        """One decode step: every launch reads the step counter from device memory.  The members' layer sequences follow one another
        on the one stream (a linear graph; step graphs on several streams do not overlap on this stack — see `lanes`), then ONE beam
        step reads all their logits."""
        for dec, m, mpk in zip(self.members, st["members"], pk):
            self._step_member(dec, st, m, mpk, bsz)
        if st["lex_desc"] is not None:
            f = None if self.lm is None else ctypes.byref(st["lm_desc"])
            L.check(L.load().cst_beam_step_lex(ctypes.byref(st["desc"]), f, ctypes.byref(st["lex_desc"]), L.stream_ptr()), "cst_beam_step_lex")
        elif self.lm is None:
            L.check(L.load().cst_beam_step(ctypes.byref(st["desc"]), L.stream_ptr()), "cst_beam_step")
        else:
            L.check(L.load().cst_beam_step_lm(ctypes.byref(st["desc"]), ctypes.byref(st["lm_desc"]), L.stream_ptr()), "cst_beam_step_lm")

    def _step_member(self, dec, st, m, pk, bsz):
        """One member's decoder up to its vocabulary projection -> m["logits"], following the shared st["tokens" / "step" / "anc"]."""
        lib = L.load()
        bbsz, C = m["x"].shape
        dt = L.dtype_code(m["x"].dtype)
        H = dec.layers[0].self_attn.num_heads
        D = C // H
        fused = m["plan"].fuse_ln
        L.check(lib.cst_dec_embed(L.ptr(st["tokens"]), L.ptr(st["step"]), L.ptr(dec.embed_tokens.weight), L.ptr(pk["pos"]),
                                  float(dec.embed_scale), dec.padding_idx, L.ptr(m["x"]), bbsz, C, self.opt.max_len,
                                  pk["pos"].shape[0], dt, L.stream_ptr()), "cst_dec_embed")
        x, x2 = m["x"], m["x2"]
        for li, layer in enumerate(dec.layers):
            sa, p = layer.self_attn, pk["layers"][li]
            if fused:
                self._ln_linear(x, p["ln_qkv"], m["qkv"])
            else:
                self._ln(x, layer.self_attn_layer_norm, m["h"], m)
                self._linear(m["h"], p["wqkv"], p["bqkv"], m["qkv"])
            L.check(lib.cst_dec_self_attn(L.ptr(m["qkv"]), L.ptr(m["kc"][li]), L.ptr(m["vc"][li]), L.ptr(st["anc"]),
                                          L.ptr(st["step"]), L.ptr(m["attn"]), bbsz, H, D, self.opt.max_len, float(sa.scaling), dt,
                                          L.stream_ptr()), "cst_dec_self_attn")
            self._linear(m["attn"], sa.out_proj.weight, sa.out_proj.bias, x2, resid=x)
            x, x2 = x2, x
            if m["plan"].cross:
                x, x2 = self._step_cross(layer, li, st, m, p, x, x2, bsz, attn=self.attention and li == len(dec.layers) - 1)
            act = L.ACT_GELU if layer.activation_fn == "gelu" else L.ACT_RELU
            if fused:
                self._ln_linear(x, p["ln_fc1"], m["f"], act=act)
            else:
                self._ln(x, layer.final_layer_norm, m["h"], m)
                self._linear(m["h"], layer.fc1.weight, layer.fc1.bias, m["f"], act=act)
            self._linear(m["f"], layer.fc2.weight, layer.fc2.bias, x2, resid=x, ws=m["gemm_ws"])
            x, x2 = x2, x
        if dec.layer_norm is not None:
            self._ln(x, dec.layer_norm, m["h"], m)
        self._linear(x if dec.layer_norm is None else m["h"], dec.output_projection.weight, None, m["logits"])
        # the x/x2 swaps of a step (3 per layer, 2 without a cross block) may leave the residual stream in x2: the NEXT step's embed
        # always writes m["x"], and every step performs the same swaps, so the captured sequence is step-invariant.

    def _attn_probs(self, ca, st, m, li, bsz):
        """`attention`, last layer of a model member: this step's head-averaged cross-attention probabilities of m["q"] over the
        sentence's encoder K (read in place in either layout) -> slot *step of st["attn_hist"]; an ensemble's members add theirs x 1/N
        one after the other (EnsembleModel.forward_decoder :829-868)."""
        hist, kx = st["attn_hist"], m["kx"][li]
        H, D, S = ca.num_heads, ca.head_dim, kx.shape[1]
        strides = (H * S * D, S * D, D) if m["plan"].head_major else (S * H * D, D, H * D)
        first = m is st["members"][0]
        L.check(L.load().cst_attn_avg_probs(L.ptr(m["q"]), m["q"].stride(0), L.ptr(kx), *strides, L.ptr(m["kpm"]), L.ptr(hist), hist.stride(0),
                                            L.ptr(st["step"]), self.opt.max_len, bsz, self.opt.beam, H, D, S, float(ca.scaling),
                                            1.0 / len(self.decs), 0 if first else 1, L.dtype_code(m["q"].dtype), L.stream_ptr()),
                "cst_attn_avg_probs")

    def _step_cross(self, layer, li, st, m, p, x, x2, bsz, attn=False):
        """The cross-attention block of one layer (query projection, attention over the sentence's encoder K/V, out-proj + residual);
        returns the swapped (x, x2).  attn: also record the attention probabilities (_attn_probs) — the launches that feed the residual
        stream stay what they are, so where the query projection runs inside the cross-attention launch the query is materialised for
        the probabilities by one more cst_dec_ln_linear (its folded weights are packed anyway)."""
        lib = L.load()
        bbsz, C = m["x"].shape
        dt = L.dtype_code(m["x"].dtype)
        ca, plan, beam = layer.encoder_attn, m["plan"], self.opt.beam
        H = layer.self_attn.num_heads
        D = C // H
        S = m["kx"][li].shape[1]
        # cross attention: one workgroup per (sentence, head); the sentence's K/V rows serve all of its beam rows
        if plan.q_in_cross:  # the query projection runs inside the cross-attention launch
            if attn:
                self._ln_linear(x, p["ln_q"], m["q"])
            _, sg, sb, eps = p["ln_q"]
            L.check(lib.cst_dec_ln_q_cross_attn(L.ptr(x), x.stride(0), L.ptr(p["ln_q_frag"]), L.ptr(sg), L.ptr(sb), eps, L.ptr(m["kx"][li]),
                                                L.ptr(m["vx"][li]), L.ptr(m["kpm"]), L.ptr(m["attn"]), L.ptr(st["step"]), self.opt.max_len,
                                                bsz, beam, H, D, S, float(ca.scaling), dt, L.stream_ptr()), "cst_dec_ln_q_cross_attn")
        else:
            if plan.fuse_ln:
                self._ln_linear(x, p["ln_q"], m["q"])
            else:
                self._ln(x, layer.encoder_attn_layer_norm, m["h"], m)
                self._linear(m["h"], ca.q_proj.weight, ca.q_proj.bias, m["q"])
            if plan.cross_mode == "shared":
                L.check(lib.cst_dec_cross_attn(L.ptr(m["q"]), L.ptr(m["kx"][li]), L.ptr(m["vx"][li]), L.ptr(m["kpm"]), L.ptr(m["attn"]),
                                               L.ptr(st["step"]), self.opt.max_len, bsz, beam, H, D, S, float(ca.scaling), dt,
                                               L.stream_ptr()), "cst_dec_cross_attn")
            else:  # the flash kernel with batch = sentence, query "time" axis = the beam rows (very long sources)
                q3, o3 = m["q"].view(bsz, beam, C), m["attn"].view(bsz, beam, C)
                d = K.attn_desc(q3, m["kx"][li], m["vx"][li], o3, m["lse"], H, D, m["kpm"], False, float(ca.scaling))
                if plan.cross_mode == "flash_hm":  # over head-major K/V: (b, h, t) strides = (H*S*D, S*D, D)
                    d.k_sb = d.v_sb = H * S * D
                    d.k_sh = d.v_sh = S * D
                    d.k_st = d.v_st = D
                K.attn_fwd_desc(d)
        if attn:
            self._attn_probs(ca, st, m, li, bsz)
        self._linear(m["attn"], ca.out_proj.weight, ca.out_proj.bias, x2, resid=x)
        return x2, x

    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, encoder_outs, bsz, prefix_tokens=None, sample_key=0, constraints=None):
        """encoder_outs: one EncoderOut per model, each with encoder_out [S, B, C] (T x B x C view) and encoder_padding_mask [B, S] or
        None (each model's own encoder; lengths S and widths may differ).  A decoder-only engine takes None: dtype and device are the
        first member's embedding table's.
        prefix_tokens: None or int64 [bsz, K] padded with pad, K <= max_len: the tokens forced at the first K steps (--prefix-size);
        it is copied into the engine's own buffer (the caller's tensor is never captured).
        sample_key: the 32-bit key of this call's draws (sampling only), written into the state's buffer before the first step: the
        captured step graph reads it there, so a replay draws with the key of the call that replays it.
        constraints: None or the packed lexical constraints int64 [bsz, W] (lexical_constraints.pack_constraints) of an engine built
        with lexical=...; each lane copies its sentences' rows into its own buffer and cst_lex_init rebuilds tables and root states.  A
        sentence whose constraints are not met within max_len finalises nothing: RuntimeError.
        Returns the reference's `finalized` structure (list over sentences of hypothesis dicts, best first)."""
        prefix_len = 0 if prefix_tokens is None else int(prefix_tokens.shape[1])
        assert prefix_tokens is None or (prefix_tokens.dim() == 2 and prefix_tokens.shape[0] == bsz and prefix_len <= self.opt.max_len)
        assert (encoder_outs is None) if self.decoder_only else (len(encoder_outs) == len(self.decs)), \
            "one encoder output per ensemble member; none for decoder-only members"
        lex = None
        if constraints is not None:
            assert self.lexical is not None, "constraints need an engine built with lexical=\"ordered\" | \"unordered\""
            assert prefix_len == 0, "lexical constraints cannot be combined with prefix_tokens"
            assert constraints.dim() == 2 and constraints.shape[0] == bsz and self.lexical_supported(constraints, self.opt.beam)
            lex = (self.lexical, int(constraints.shape[1]))
        if self.decoder_only:
            w = [d.embed_tokens.weight for d in self.decs]
            encs, masks, S, has_mask, dtype, device = [], [], None, None, w[0].dtype, w[0].device
            assert all(x.dtype == dtype and x.device == device for x in w), "ensemble members must share the storage dtype and the device"
        else:
            encs = [e.encoder_out for e in encoder_outs]
            assert all(e.shape[1] == bsz for e in encs)
            dtype, device = encs[0].dtype, encs[0].device
            assert all(e.dtype == dtype for e in encs), "ensemble members must share the storage dtype"
            masks = [e.encoder_padding_mask for e in encoder_outs]
            masks = [m if (m is not None and m.dim() == 2) else None for m in masks]
            S, has_mask = tuple(e.shape[0] for e in encs), tuple(m is not None for m in masks)
        if self.attention and len(set(S)) > 1:  # (the reference's avg_attn.add_ cannot add them either)
            raise ValueError("attention of an ensemble needs members of one encoder length, got %s" % (S,))
        pk = self._pack(dtype, device)
        lanes = min(self.lanes, bsz)
        bounds = [(bsz * i // lanes, bsz * (i + 1) // lanes) for i in range(lanes)]
        cfg = (tuple(b1 - b0 for b0, b1 in bounds), S, dtype, device, has_mask, prefix_len, lex)
        if cfg != self._cfg:
            self._state.clear()  # one resident configuration (the caches are the large buffers)
            self._cfg = cfg
        main = torch.cuda.current_stream()
        while lanes > 1 and len(self._streams) < lanes:
            self._streams.append(torch.cuda.Stream(device=device))
        encb = [e.transpose(0, 1) for e in encs]
        encb = [e if e.is_contiguous() else e.contiguous() for e in encb]
        total = self.opt.max_len + 1
        runs = []
        for i, (b0, b1) in enumerate(bounds):
            stream = main if lanes == 1 else self._streams[i]
            if stream is not main:
                stream.wait_stream(main)
            with torch.cuda.stream(stream):
                st = self._alloc(i, b1 - b0, S, dtype, device, has_mask, prefix_len, lex)
                if lex is not None:  # the lane's sentences' constraints, into the buffer cst_lex_init reads (in _begin)
                    st["lex_packed"].copy_(constraints[b0:b1].to(device=device, dtype=torch.int64))
                if prefix_len > 0:  # the lane's sentences' prefixes, into the buffer the (captured) beam step reads
                    st["prefix"].copy_(prefix_tokens[b0:b1].to(device=device, dtype=torch.int64))
                if self.opt.sampling:
                    k32 = int(sample_key) & 0xFFFFFFFF
                    st["sample_key"].fill_(k32 - (1 << 32) if k32 >= (1 << 31) else k32)
                done = self._begin(st, pk, [e[b0:b1] for e in encb], [m[b0:b1] if m is not None else None for m in masks], b1 - b0)
            runs.append(dict(stream=stream, st=st, bsz=b1 - b0, steps=done, remaining=b1 - b0))
        while any(r["steps"] < total and r["remaining"] > 0 for r in runs):
            for r in runs:
                r["n"] = min(self.poll, total - r["steps"]) if r["remaining"] > 0 else 0
            for j in range(self.poll):  # the lanes' steps alternate in launch order; each lane's own order is its stream's
                for r in runs:
                    if j < r["n"]:
                        with torch.cuda.stream(r["stream"]):
                            if self.use_graph:
                                r["st"]["graph"].replay()
                            else:
                                self._step(r["st"], pk, r["bsz"])
            for r in runs:
                if r["n"]:
                    r["steps"] += r["n"]
                    with torch.cuda.stream(r["stream"]):
                        r["remaining"] = int(r["st"]["num_remaining"].item())  # the only host sync of the loop (one per lane)
        # (with lexical constraints a sentence that could not meet them is still "remaining": _collect names it)
        assert lex is not None or all(r["remaining"] == 0 for r in runs), "beam search did not terminate within max_len + 1 steps"
        finalized = []
        for r in runs:
            with torch.cuda.stream(r["stream"]):
                finalized += self._collect(r["st"], r["bsz"], None if r["stream"] is main else main)
            if r["stream"] is not main:
                main.wait_stream(r["stream"])
        if lex is not None:
            unmet = [b for b, hyps in enumerate(finalized) if not hyps]
            if unmet:
                raise RuntimeError("lexical constraints not met within max_len: sentences %s" % unmet)
        return finalized

    def _begin_member(self, dec, m, encb, mask, bsz):
        """The static cross-attention K/V of one model, projected from ITS encoder's output."""
        S, Ce = encb.shape[1], encb.shape[2]
        flat = encb.reshape(bsz * S, Ce)
        for li, layer in enumerate(dec.layers):  # static cross-attention K/V, once per sentence (not per beam)
            ca = layer.encoder_attn
            if m["plan"].head_major:  # [bsz, H, S, D] (one transposing copy per call)
                for name, proj in (("kx", ca.k_proj), ("vx", ca.v_proj)):
                    self._linear(flat, proj.weight, proj.bias, m["proj"])
                    m[name][li].view(bsz, ca.num_heads, S, ca.head_dim).copy_(
                        m["proj"].view(bsz, S, ca.num_heads, ca.head_dim).transpose(1, 2))
            else:
                self._linear(flat, ca.k_proj.weight, ca.k_proj.bias, m["kx"][li].view(bsz * S, -1))
                self._linear(flat, ca.v_proj.weight, ca.v_proj.bias, m["vx"][li].view(bsz * S, -1))
        if mask is not None:
            m["kpm"].copy_(mask.to(torch.uint8))

    def _begin(self, st, pk, encb, mask, bsz):
        """Queues the per-call work of one lane on the current stream: every model's static cross-attention K/V of its sentences, the beam
        state, and — first call of a configuration — the eager step 0 and the capture of the step graph.  Returns the number of
        decode steps already taken (1 after that eager step, else 0)."""
        # (the LM, last of the members, has no encoder: zip stops before it; decoder-only members have none either: encb is empty)
        for dec, m, e, mk in zip(self.decs, st["members"], encb, mask):
            self._begin_member(dec, m, e, mk, bsz)
        L.check(L.load().cst_beam_init(ctypes.byref(st["desc"]), L.stream_ptr()), "cst_beam_init")
        if st["lex_desc"] is not None:  # tables and root states from the call's constraints (outside the captured step)
            L.check(L.load().cst_lex_init(ctypes.byref(st["desc"]), ctypes.byref(st["lex_desc"]), L.stream_ptr()), "cst_lex_init")
        if self.use_graph and st["graph"] is None:
            self._step(st, pk, bsz)  # eager warm-up step 0 (loads code objects, sizes the GEMM workspace)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step(st, pk, bsz)
            st["graph"] = g
            return 1
        return 0

    def _collect(self, st, bsz, consumer=None):
        # hypotheses are views of ONE device-side copy of the result buffers (the engine state is reused by the next call)
        d_tokens, d_pos, d_score = st["fin_tokens"].clone(), st["fin_pos"].clone(), st["fin_score"].clone()
        if consumer is not None:  # made on a lane's stream, read by the caller on its own
            for t in (d_tokens, d_pos, d_score):
                t.record_stream(consumer)
        d_attn = None
        if self.attention:
            # column j of hypothesis (b, r) is attn_hist[fin_anc[b, r, j], j, :]: ONE indexed gather over the lane's history (slots past a
            # hypothesis' length read row 0 of a zero-filled table and are cut off below), then source-major like the reference
            hist, fa = st["attn_hist"], st["fin_anc"].long()
            L1 = hist.shape[1]
            d_attn = hist[fa, torch.arange(L1, device=hist.device).view(1, 1, L1)].transpose(2, 3)  # [bsz, beam, S, L1]
            if consumer is not None:
                d_attn.record_stream(consumer)
        fin_score, fin_len, nfinal = d_score.cpu(), st["fin_len"].cpu(), st["nfinal"].cpu()
        finalized = []
        for b in range(bsz):
            hyps = []
            for r in range(int(nfinal[b])):
                n = int(fin_len[b, r])
                hyps.append({"tokens": d_tokens[b, r, :n], "score": d_score[b, r], "attention": None if d_attn is None else d_attn[b, r, :, :n],
                             "alignment": None, "positional_scores": d_pos[b, r, :n]})
            _, order = torch.sort(fin_score[b, :len(hyps)], descending=True)  # sequence_generator.py:529-540
            finalized.append([hyps[i] for i in order.tolist()])
        return finalized
