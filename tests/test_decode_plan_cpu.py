"""No-GPU checks of the decode engine's three records (decode_engine.py; building an engine touches no device):
  * StepPlan / nodes_per_step: the launches of a step, pinned to the documented per-layer counts — per layer (LayerNorm, qkv, self-attention,
    out, LayerNorm, q, cross-attention, out, LayerNorm, fc1, fc2) = 11, 7 without the cross block; the three (two) LayerNorms folded into
    their projections on the bf16 path with C % 512 == 0 at <= 1024 rows = 8 (5); the query projection inside the cross-attention launch
    (bf16, head dim 64, beam <= 32) = 7; + 1 where fc2 is split (bf16, <= 256 rows, ffn >= 4096); embed, final LayerNorm and vocabulary
    projection per member; the two beam-search kernels once;
  * Switches: each CST_DEC_NO_* switch moves the row it governs;
  * DecodeOptions: equal options hash equal, a difference in any one field does not (the state-key property), and fill() leaves the
    fields of a strategy that is off at zero."""
import dataclasses
from importlib import import_module
from types import SimpleNamespace as NS

import pytest
import torch

from conftest import load_pkg

F32, BF16 = torch.float32, torch.bfloat16
SWITCHES = ("CST_DEC_CROSS_KERNEL", "CST_DEC_LANES", "CST_DEC_NO_LN_FUSE", "CST_DEC_NO_SPLITK", "CST_DEC_NO_QCROSS")
V = 100


class _Dict:
    def pad(self): return 1
    def eos(self): return 2
    def unk(self): return 3
    def __len__(self): return V


def _dec(C, D, F, layers, cross=True):
    """A decoder as far as the engine's constructor and plan read it."""
    layer = NS(self_attn=NS(head_dim=D, q_proj=NS(bias=0.0)), encoder_attn=NS(head_dim=D) if cross else None, fc1=NS(out_features=F),
               normalize_before=True)
    return NS(embed_dim=C, layers=[layer] * layers, layer_norm=NS(), embed_positions=NS(get_embedding=None), layernorm_embedding=None,
              project_in_dim=None, project_out_dim=None, adaptive_softmax=None, output_projection=NS(weight=NS(shape=(V, C))))


@pytest.fixture
def E(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    load_pkg()
    return import_module("chimera-st_amd.decode_engine")


def _engine(E, decs, beam=4, lm=None, **opts):
    return E.BeamDecodeEngine(decs, _Dict(), E.DecodeOptions(beam=beam, max_len=20, **opts), lm_decoder=lm)


FP32_ROW = (256, 64, 1024, 2)
FUSED_ROW = (512, 64, 2048, 2)
BENCH_ROW = (1024, 64, 4096, 6)
SINGLE = [  # dtype, (C, D, F, layers), beam, rows, member nodes, total
    (F32, FP32_ROW, 4, 20, 1 + 11 * 2 + 2, 27),
    (BF16, FUSED_ROW, 4, 20, 1 + 7 * 2 + 2, 19),
    (BF16, (512, 32, 2048, 2), 4, 20, 1 + 8 * 2 + 2, 21),     # head dim 32: no query projection inside the cross-attention launch
    (BF16, (768, 64, 3072, 2), 4, 20, 25, 27),                # C % 512 != 0: nothing folded
    (BF16, BENCH_ROW, 5, 160, 1 + 8 * 6 + 2, 53),             # the benchmark's: 7 + the fc2 reduce
    (BF16, BENCH_ROW, 5, None, 1 + 7 * 6 + 2, 47),
    (BF16, BENCH_ROW, 5, 2000, 1 + 11 * 6 + 2, 71),           # > 1024 rows: unfused, unsplit
    (BF16, FUSED_ROW, 64, 20, 19, 21),                        # beam > 32: flash, no query projection inside it
]


@pytest.mark.parametrize("dtype,dims,beam,rows,member,total", SINGLE)
def test_nodes_of_one_member(E, dtype, dims, beam, rows, member, total):
    dec = _dec(*dims)
    eng = _engine(E, [dec], beam=beam)
    assert eng._member_nodes(dec, dtype, rows) == member
    assert eng.nodes_per_step(dtype, rows) == total
    plan = eng._plan(dec, dtype, rows)
    assert member == 1 + plan.layer_nodes * len(dec.layers) + 2


def test_nodes_of_ensembles_and_language_models(E):
    two = _engine(E, [_dec(*FP32_ROW), _dec(*FP32_ROW)])
    assert two.nodes_per_step(F32, 20) == 25 + 25 + 2 == 52
    lm = _dec(256, 64, 1024, 3, cross=False)
    eng = _engine(E, [_dec(*FP32_ROW)], lm=lm, lm_weight=0.5)
    assert eng.members == eng.decs + [lm] and eng._member_nodes(lm, F32, 20) == 1 + 7 * 3 + 2 == 24
    assert eng.nodes_per_step(F32, 20) == 25 + 24 + 2 == 51
    lm = _dec(512, 64, 2048, 3, cross=False)
    eng = _engine(E, [_dec(*FUSED_ROW)], lm=lm, lm_weight=0.5)
    assert eng._member_nodes(lm, BF16, 20) == 1 + 5 * 3 + 2 == 18
    assert eng.nodes_per_step(BF16, 20) == 17 + 18 + 2 == 37
    assert eng._plan(lm, BF16, 20) == (False, True, None, False, False)


def test_plan_records(E):
    eng = _engine(E, [_dec(*BENCH_ROW)], beam=5)
    dec = eng.decs[0]
    assert eng._plan(dec, BF16, 160) == E.StepPlan(cross=True, fuse_ln=True, cross_mode="shared", q_in_cross=True, split_fc2=True)
    assert eng._plan(dec, BF16, 160).head_major and eng._plan(dec, BF16, 1024).fuse_ln and not eng._plan(dec, BF16, 1025).fuse_ln
    assert eng._plan(dec, BF16, 256).split_fc2 and not eng._plan(dec, BF16, 257).split_fc2
    assert eng._plan(dec, F32, 160) == (True, False, "flash", False, False) and not eng._plan(dec, F32, 160).head_major
    for mode in ("flash", "flash_hm", "shared"):
        e = E.BeamDecodeEngine([dec], _Dict(), E.DecodeOptions(beam=5, max_len=20), cross_kernel=mode)
        for dt in (F32, BF16):
            p = e._plan(dec, dt, 160)
            assert p.cross_mode == mode and p.head_major == (mode != "flash") and p.q_in_cross == (dt == BF16 and mode == "shared")


@pytest.mark.parametrize("switch,dims,beam,rows,total", [
    ("CST_DEC_NO_LN_FUSE", FUSED_ROW, 4, 20, 27),   # 19 -> the unfused 1 + 11 * 2 + 2 + 2
    ("CST_DEC_NO_QCROSS", FUSED_ROW, 4, 20, 21),    # 19 -> two launches: 1 + 8 * 2 + 2 + 2
    ("CST_DEC_NO_SPLITK", BENCH_ROW, 5, 160, 47),   # 53 -> unsplit: 1 + 7 * 6 + 2 + 2
])
def test_each_switch_moves_its_row(E, monkeypatch, switch, dims, beam, rows, total):
    monkeypatch.setenv(switch, "1")
    assert _engine(E, [_dec(*dims)], beam=beam).nodes_per_step(BF16, rows) == total


def test_switches_are_read_when_the_engine_is_built(E, monkeypatch):
    monkeypatch.setenv("CST_DEC_LANES", "3")
    monkeypatch.setenv("CST_DEC_CROSS_KERNEL", "flash_hm")
    eng = _engine(E, [_dec(*FUSED_ROW)])
    assert eng.lanes == 3 and eng.sw == E.Switches("flash_hm", 3, False, False, False)
    assert _engine(E, [_dec(*FUSED_ROW)], sampling=True).lanes == 1  # the index of a draw holds the sentence's position in the whole batch
    monkeypatch.setenv("CST_DEC_LANES", "1")
    monkeypatch.setenv("CST_DEC_NO_LN_FUSE", "1")
    assert eng.sw.lanes == 3 and eng.nodes_per_step(BF16, 20) == 21  # not read again (flash_hm: the query projection is its own launch)
    built_with_args = E.BeamDecodeEngine([_dec(*FUSED_ROW)], _Dict(), E.DecodeOptions(beam=4, max_len=20), cross_kernel="shared", lanes=2)
    assert built_with_args.sw == E.Switches("shared", 2, True, False, False)


OTHER = dict(beam=5, max_len=21, min_len=2, normalize_scores=False, len_penalty=1.5, unk_penalty=0.5, temperature=0.7, no_repeat_ngram_size=3,
             sampling=True, topk=5, topp=0.9, diverse_groups=2, diverse_strength=0.5, sibling_rate=0.0, lm_weight=0.3)


def test_options_are_the_state_key(E):
    a, b = E.DecodeOptions(beam=4, max_len=20), E.DecodeOptions(beam=4.0, max_len="20", topk=-1, topp=-1.0, diverse_groups=-3)
    assert a == b and hash(a) == hash(b) and (b.beam, b.max_len, b.topk, b.topp, b.diverse_groups) == (4, 20, 0, 0.0, 0)
    assert type(b.beam) is int and type(b.max_len) is int
    assert sorted(OTHER) == sorted(f.name for f in dataclasses.fields(E.DecodeOptions))  # every field is varied below
    for name, value in OTHER.items():
        c = dataclasses.replace(a, **{name: value})
        assert c != a and hash(c) != hash(a) and len({a: 0, c: 1}) == 2, name
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.beam = 5
    with pytest.raises(AssertionError):
        E.DecodeOptions(beam=4, max_len=20, no_repeat_ngram_size=1)


def test_fill_leaves_strategies_that_are_off_at_zero(E):
    BeamDesc = import_module("chimera-st_amd.lib").BeamDesc
    d = BeamDesc()
    E.DecodeOptions(beam=4, max_len=20, min_len=3, len_penalty=1.5, topk=5, topp=0.5, diverse_strength=0.5).fill(d, 1)
    assert (d.beam, d.max_len, d.min_len, d.len_penalty, d.normalize_scores, d.members) == (4, 20, 3, 1.5, 1, 0)
    assert (d.sampling, d.sample_topk, d.sample_topp, d.diverse_groups, d.diverse_strength, d.diverse_siblings, d.sibling_rate) == (0,) * 7
    for n in (2, 3, 8):
        E.DecodeOptions(beam=4, max_len=20).fill(d, n)
        assert d.members == n
    d = BeamDesc()
    E.DecodeOptions(beam=4, max_len=20, sampling=True, topk=5, no_repeat_ngram_size=3).fill(d, 1)
    assert (d.sampling, d.sample_topk, d.no_repeat_ngram, d.diverse_groups, d.diverse_siblings) == (1, 5, 3, 0, 0)
    d = BeamDesc()
    E.DecodeOptions(beam=4, max_len=20, diverse_groups=2, diverse_strength=0.5).fill(d, 1)
    assert (d.sampling, d.diverse_groups, d.diverse_strength, d.diverse_siblings) == (0, 2, 0.5, 0)
    d = BeamDesc()
    E.DecodeOptions(beam=4, max_len=20, sibling_rate=0.0).fill(d, 1)  # rate 0 is on
    assert (d.sampling, d.diverse_groups, d.diverse_siblings, d.sibling_rate) == (0, 0, 1, 0.0)
