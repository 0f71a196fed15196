"""GPU tests of checkpoint-ensemble decoding (`--path a.pt:b.pt:c.pt`): the N-member form of cst_beam_step, the engine with one
decoder / K/V cache set / logits buffer per member and ONE shared beam state, the host loop's ensemble _forward_decoder, and the
CLI — against the fixture the REAL reference's EnsembleModel search produced (decode_ensemble_tiny.npz)."""
import ctypes
import json
import math
import os
import shutil
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, load_pkg
from ensemble_inputs import combine, fp32_torch_error, member_logits
from test_decode_engine_gpu import _beam_state, _build_s2t
from test_model_gpu import assert_close, build_from_golden

pytestmark = pytest.mark.gpu
SETTINGS = {"beam5": dict(beam_size=5), "recipe": dict(beam_size=10, len_penalty=1.5), "temp": dict(beam_size=5, temperature=0.7)}


def fixture_members(n, dtype=torch.float32):
    """The first n members of the fixture as models of this package: member 0 = decode_tiny.npz, members 1 and 2 = member 0 with
    the (float16-exact) tensors decode_ensemble_tiny.npz stores."""
    g, ens = load_golden("decode_tiny.npz"), load_golden("decode_ensemble_tiny.npz")
    models, task, args = [], None, None
    for k in range(n):
        gk = dict(g)
        pre = "member%d/param/" % k
        for name, v in ens.items():
            if name.startswith(pre):
                assert "param/" + name[len(pre):] in gk
                gk["param/" + name[len(pre):]] = v.astype(np.float32)
        model, task, args = build_from_golden(gk, "chimera", dtype)
        models.append(model.eval())
    return models, task, args, ens


def SG():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator").SequenceGenerator


def _sample(rec, tag):
    return {"net_input": {"src_tokens": torch.from_numpy(rec["in/%s/src_tokens" % tag]).cuda(),
                          "src_lengths": torch.from_numpy(rec["in/%s/src_lengths" % tag]).cuda()}}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", sorted(SETTINGS))
@pytest.mark.parametrize("N", [2, 3])
def test_ensemble_matches_reference_generator(N, name, fused):
    """Every finalized hypothesis of the reference's SequenceGenerator([m0, .., m_{N-1}]) in its order: token ids exact, scores to
    1e-4, positional scores to 1e-3 — from the device engine and from the host loop, fp32 storage, inputs "a" and "b"."""
    models, task, _, ens = fixture_members(N)
    rec = load_golden("decode_recipe_tiny.npz")
    gen = SG()(models, task.target_dictionary, max_len_a=0, max_len_b=int(ens["meta/max_len_b"]), min_len=1, fused=fused, **SETTINGS[name])
    for tag in ("a", "b"):
        hyps = gen.generate(models, _sample(rec, tag))
        assert (gen._engine is not None) == fused
        if fused:
            assert len(gen._engine.decs) == N
        for b in range(len(hyps)):
            n = int(ens["n%d/gen/%s/%s/b%d/n" % (N, name, tag, b)])
            assert len(hyps[b]) == n, (tag, b)
            for k in range(n):
                key = "n%d/gen/%s/%s/b%d/r%d/" % (N, name, tag, b, k)
                assert hyps[b][k]["tokens"].tolist() == ens[key + "tokens"].tolist(), key
                assert abs(float(hyps[b][k]["score"]) - float(ens[key + "score"])) < 1e-4, key
                assert_close(hyps[b][k]["positional_scores"], ens[key + "pos_scores"], 1e-3, key + "pos_scores")


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_ensemble_logprobs_kernel(N, dtype, T):
    """cst_beam_step with members = N: the combined log-probabilities lp[v] = log(sum_n exp(l_n[v]/T - lse_n)) - log N (lprobs_out of
    one step) against the fp64 torch evaluation of the same formula on the same stored logits — 160 rows, vocabulary 10 000 (1250
    16-byte vectors of bf16 over 512 threads: ragged per-thread tails), one row with -inf in a single member, one with -inf in all.

    Bound per element: 4 x the largest error of the FP32 TORCH evaluation of the formula against fp64 on these very inputs (same
    arithmetic, another summation order), never above 1e-4 / 13 = 7.69e-6 (the project's score bar over the fixture's longest
    hypothesis).  Measured on the CPU (tests/ensemble_inputs.py fp32_torch_error), fp32 torch vs fp64:
        fp32 logits  N=2: 3.44e-6 (T=1) 4.60e-6 (T=.7)   N=3: 3.89e-6 / 5.34e-6   N=8: 3.25e-6 / 4.56e-6
        bf16 logits  N=2: 2.58e-6 (T=1) 3.91e-6 (T=.7)   N=3: 2.83e-6 / 5.07e-6   N=8: 3.41e-6 / 4.90e-6
    so 4 x measured = 1.0e-5 .. 2.1e-5 and the bound in force is the cap, 7.69e-6, in every case (|lp| reaches 35: one fp32 ulp
    there is 3.8e-6)."""
    load_pkg()
    L = import_module("chimera-st_amd.lib")
    lib = L.load()
    rows, V = 160, 10000
    x = member_logits(N, dtype, rows, V)
    cpu_err = fp32_torch_error(x, T)
    bound = min(4.0 * cpu_err, 1e-4 / 13)
    ref = combine(x, T, torch.float64)
    Vp = (V + 7) // 8 * 8
    bufs = [torch.zeros(rows, Vp, dtype=dtype, device="cuda") for _ in range(N)]
    for n in range(N):
        bufs[n][:, :V] = x[n].cuda()
    st, d = _beam_state(L, rows, 1, V, 4, 1, dtype, bufs[0], temperature=T)
    out = torch.full((rows, Vp), 7.0, dtype=torch.float32, device="cuda")
    d.members = N
    for n in range(1, N):
        d.logits_n[n - 1] = bufs[n].data_ptr()
    d.lprobs_out = out.data_ptr()
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
    got = out[:, :V].cpu().double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), "the -inf sets differ (or a NaN appeared)"
    assert not torch.isnan(got).any()
    assert bool((got[~fin] == -math.inf).all()) and int((~fin[9]).sum()) == len(range(0, V, 11)) and bool(fin[5].all())
    err = float((got - ref)[fin].abs().max())
    print("N=%d %s T=%g: kernel max |err| %.3e, fp32 torch %.3e, bound %.3e" % (N, dtype, T, err, cpu_err, bound))
    assert err <= bound, (err, bound, cpu_err)
    # the search consumed these values: the step's winner of every row (beam 1, eos barred by min_len, pad barred) and its score
    masked = ref.clone()
    masked[:, 1] = -math.inf
    masked[:, 2] = -math.inf
    best = masked.argmax(dim=1)
    assert st["tokens"][1, :, 1].cpu().tolist() == best.tolist()
    assert float((st["scores"][1, :, 0].cpu().double() - masked.max(dim=1).values).abs().max()) <= bound


def test_more_than_eight_members_are_rejected():
    load_pkg()
    L = import_module("chimera-st_amd.lib")
    buf = torch.zeros(4, 64, dtype=torch.float32, device="cuda")
    st, d = _beam_state(L, 4, 1, 61, 4, 1, torch.float32, buf)
    d.members = 9
    assert L.load().cst_beam_step(ctypes.byref(d), L.stream_ptr()) == -1
    assert b"ensemble members" in L.load().cst_last_error()
    d.members = 2  # member 1's matrix is missing
    assert L.load().cst_beam_step(ctypes.byref(d), L.stream_ptr()) == -1
    assert b"member 1" in L.load().cst_last_error()


@pytest.mark.parametrize("N", [2, 3])
def test_copies_of_one_model_decode_like_the_single_model(N):
    """The average of N equal distributions is the distribution: token ids identical to the single-model engine, scores within 1e-4
    (fp32, the ragged s2t_transformer batch of test_engine_equals_mirror_loop_ragged_batch); the engine really runs N members."""
    model, task = _build_s2t(torch.float32, tied=False)
    g = torch.Generator().manual_seed(11)
    src = torch.randn(5, 97, 80, generator=g).cuda()
    lens = torch.tensor([97, 80, 64, 33, 20]).cuda()
    sample = {"net_input": {"src_tokens": src, "src_lengths": lens}}
    one = SG()([model], task.target_dictionary, beam_size=4, max_len_a=0, max_len_b=24)
    many = SG()([model] * N, task.target_dictionary, beam_size=4, max_len_a=0, max_len_b=24)
    h1, hn = one.generate([model], sample), many.generate([model] * N, sample)
    assert len(one._engine.decs) == 1 and len(many._engine.decs) == N
    assert many._engine.nodes_per_step(torch.float32, 20) == N * (one._engine.nodes_per_step(torch.float32, 20) - 2) + 2
    for b in range(5):
        assert len(h1[b]) == len(hn[b]) == 4
        for r in range(4):
            assert h1[b][r]["tokens"].tolist() == hn[b][r]["tokens"].tolist(), (b, r)
            assert abs(float(h1[b][r]["score"]) - float(hn[b][r]["score"])) < 1e-4


@pytest.mark.parametrize("N", [2, 3])
def test_copies_bf16_large_dims(N):
    """s2t_transformer_l decoder dimensions in bf16 (the standard of test_engine_bf16_large_dims_runs_and_agrees_on_first_tokens): the
    N-copy ensemble terminates, scores are finite and ordered, first tokens agree with the single-model engine in >= 6 of 8."""
    model, task = _build_s2t(torch.bfloat16, d=1024, heads=16, layers=2, V=10000)
    g = torch.Generator().manual_seed(5)
    src = torch.randn(8, 120, 80, generator=g).cuda().to(torch.bfloat16)
    lens = torch.tensor([120, 120, 100, 90, 77, 60, 41, 30]).cuda()
    sample = {"net_input": {"src_tokens": src, "src_lengths": lens}}
    h1 = SG()([model], task.target_dictionary, beam_size=5, max_len_a=0, max_len_b=20).generate([model], sample)
    hn = SG()([model] * N, task.target_dictionary, beam_size=5, max_len_a=0, max_len_b=20).generate([model] * N, sample)
    agree = 0
    for b in range(8):
        sc = [float(h["score"]) for h in hn[b]]
        assert len(sc) == 5 and all(math.isfinite(s) for s in sc) and sc == sorted(sc, reverse=True)
        agree += int(h1[b][0]["tokens"][0]) == int(hn[b][0]["tokens"][0])
    assert agree >= 6


class _ShortEncoder(torch.nn.Module):
    """A member whose encoder output is shorter than its partner's: the wrapped encoder's output without its last `cut` positions."""

    def __init__(self, enc, cut):
        super().__init__()
        self.enc, self.cut = enc, cut

    def forward_torchscript(self, net_input):
        return self._cut(self.enc.forward_torchscript(net_input))

    def _cut(self, out):
        pm = out.encoder_padding_mask
        return out._replace(encoder_out=out.encoder_out[:-self.cut].contiguous(),
                            encoder_padding_mask=pm[:, :-self.cut].contiguous() if pm is not None else None)

    def reorder_encoder_out(self, out, new_order):
        return self.enc.reorder_encoder_out(out, new_order)


def test_engine_equals_host_loop_members_of_different_depth_and_source_length():
    """Two fp32 members that differ in decoder depth (2 and 3 layers) and in encoder output length: the device engine (per-member
    caches and encoder K/V, one ancestry table) and the host loop (per-member incremental state) give the same hypotheses."""
    m0, task = _build_s2t(torch.float32, layers=2, seed=3, tied=False)
    m1, _ = _build_s2t(torch.float32, layers=3, seed=4, tied=False)
    m1.encoder = _ShortEncoder(m1.encoder, 5)
    models = [m0, m1]
    g = torch.Generator().manual_seed(13)
    src = torch.randn(4, 97, 80, generator=g).cuda()
    lens = torch.tensor([97, 97, 90, 85]).cuda()
    sample = {"net_input": {"src_tokens": src, "src_lengths": lens}}
    fused = SG()(models, task.target_dictionary, beam_size=4, max_len_a=0, max_len_b=20)
    host = SG()(models, task.target_dictionary, beam_size=4, max_len_a=0, max_len_b=20, fused=False)
    h1, h2 = fused.generate(models, sample), host.generate(models, sample)
    eng = fused._engine
    assert eng is not None and host._engine is None and [len(d.layers) for d in eng.decs] == [2, 3]
    st = next(iter(eng._state.values()))
    ms = st["members"]
    assert len(ms) == 2 and ms[0]["kx"][0].shape[1] == ms[1]["kx"][0].shape[1] + 5
    seen = set()
    for b in range(4):
        assert len(h1[b]) == len(h2[b]) == 4
        for r in range(4):
            assert h1[b][r]["tokens"].tolist() == h2[b][r]["tokens"].tolist(), (b, r)
            assert abs(float(h1[b][r]["score"]) - float(h2[b][r]["score"])) < 1e-4
            seen.update(h1[b][r]["tokens"].tolist())
    assert len(seen) > 8, "degenerate test: the hypotheses repeat a handful of tokens"


def test_two_calls_replay_one_graph():
    models, task, _, ens = fixture_members(2)
    rec = load_golden("decode_recipe_tiny.npz")
    gen = SG()(models, task.target_dictionary, beam_size=5, max_len_a=0, max_len_b=12)
    flat = lambda hyps: [[(h["tokens"].tolist(), float(h["score"]), h["positional_scores"].tolist()) for h in hb] for hb in hyps]
    first = flat(gen.generate(models, _sample(rec, "b")))
    graphs = [st["graph"] for st in gen._engine._state.values()]
    assert len(graphs) == 1 and graphs[0] is not None
    second = flat(gen.generate(models, _sample(rec, "b")))
    assert second == first
    assert [st["graph"] for st in gen._engine._state.values()] == graphs  # the same captured graph object: nothing was re-captured


def test_cli_path_list_decodes_the_ensemble(tmp_path, capsys):
    """fairseq_generate.py --path a.pt:b.pt on tests/golden/data_tiny (its dictionary padded to the fixture models' 60 symbols):
    the H- lines are those of SequenceGenerator([m0, m1]) called directly, the summary says "models": 2, and --path a.pt alone gives
    the single-model generator's hypotheses."""
    cli = import_module("chimera-st_amd.cli")
    cu = import_module("chimera-st_amd.checkpoint_utils")
    models, task, args, _ = fixture_members(2)
    data = os.path.join(GOLDEN, "data_tiny")
    root = tmp_path / "data"
    root.mkdir()
    for f in os.listdir(data):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(data, f), root / f)
    (root / "config_wave.yaml").write_text((root / "config_wave.yaml").read_text().replace("AUDIO_ROOT", data))
    lines = (root / "dict.txt").read_text().splitlines()
    V = models[0].decoder.embed_tokens.num_embeddings
    lines += ["filler%d 1" % i for i in range(V - 4 - len(lines))]
    (root / "dict.txt").write_text("\n".join(lines) + "\n")
    paths = []
    for k, m in enumerate(models):
        a = Namespace(**vars(args))
        a.arch, a.task, a.no_save_optimizer_state = "s2t_transformer_w2v2_interlingua_base", "triplet", True
        a.data, a.config_yaml = str(root), "config_wave.yaml"
        paths.append(str(tmp_path / ("m%d.pt" % k)))
        cu.save_state(paths[-1], a, m.state_dict(), None, None, 0)
    common = [str(root), "--task", "triplet", "--config-yaml", "config_wave.yaml", "--gen-subset", "dev_st", "--max-tokens", "12000",
              "--beam", "5", "--max-len-b", "12", "--max-source-positions", "2000000"]

    def run(path):
        capsys.readouterr()
        summary = cli.generate_main(common + ["--path", path])
        out = capsys.readouterr().out.splitlines()
        return summary, {int(l.split("\t")[0][2:]): l.split("\t")[1:] for l in out if l.startswith("H-")}

    def direct(ms):
        loaded, _, t = cu.load_model_ensemble_and_task(paths[:len(ms)], arg_overrides={"data": str(root), "config_yaml": "config_wave.yaml",
                                                                                      "max_source_positions": 2000000})
        loaded = [m.to("cuda").eval() for m in loaded]
        ds = t.load_dataset("dev_st")
        itr = t.get_batch_iterator(ds, max_tokens=12000, max_positions=(2000000, 1024), ignore_invalid_inputs=True)
        gen = SG()(loaded, t.target_dictionary, beam_size=5, max_len_a=0, max_len_b=12)
        res = {}
        for s in itr.next_epoch_itr(shuffle=False):
            ni = s["net_input"]
            hyps = gen.generate(loaded, {"net_input": {"src_tokens": ni["src_tokens"].cuda(), "src_lengths": ni["src_lengths"].cuda()}})
            for i, sid in enumerate(s["id"].tolist()):
                res[sid] = ["%.6f" % (float(hyps[i][0]["score"]) / math.log(2)), t.target_dictionary.string(hyps[i][0]["tokens"].cpu())]
        return res

    s2, h2 = run(paths[0] + ":" + paths[1])
    assert s2["models"] == 2 and s2["sentences"] == len(h2) > 0
    assert h2 == direct(models)
    s1, h1 = run(paths[0])
    assert s1["models"] == 1 and h1 == direct(models[:1])
    assert h1 != h2, "the second file of --path changed nothing"
