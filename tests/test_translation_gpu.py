"""The `translation` task on a real MI355X: cst_collate_pairs against the host collater (bit-equal, every word written), the two
routes of batch assembly end to end through train_main (bit-identical updates, BLEU statistics and checkpoints), text decoding and
--eval-bleu validation against the reference fixture (tests/golden/translation_tiny.npz), and the drivers."""
import ast
import contextlib
import io
import json
import os
import shutil
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, load_pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.join(GOLDEN, "translation_tiny")
PAD, EOS = 1, 2
SENTINEL = -7777
GEN = dict(beam=5, max_len_a=1.2, max_len_b=10)  # the script's --eval-bleu-args


def mods():
    load_pkg()
    return (import_module("chimera-st_amd.language_pair_dataset"), import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.tasks"),
            import_module("chimera-st_amd.cli"))


# ---- cst_collate_pairs against the host collater --------------------------------------------------------------------------------
# sentence lengths (tokens incl. eos): odd ones first, so that the uint16 sentences behind them start on odd element offsets; 1, 7 and 65
# (one row crosses a wave), 130 (a row wider than two waves), and the corpus's last sentence
SRC_LENS = [1, 7, 65, 3, 130, 2, 9, 1, 64, 5, 33, 12]
TGT_LENS = [3, 1, 7, 130, 65, 1, 4, 2, 129, 8, 6, 11]


def corpus(dtype, seed=3):
    r = np.random.RandomState(seed)
    hi = 250 if dtype == np.uint8 else 60000
    mk = lambda lens: [np.concatenate([r.randint(4, hi, size=n - 1), [EOS]]).astype(dtype) for n in lens]
    return mk(SRC_LENS), mk(TGT_LENS)


def resident(P, src, tgt, lps, lpt):
    off = lambda s: np.concatenate([[0], np.cumsum([len(x) for x in s])]).astype(np.int64)
    return P.ResidentPairs(np.concatenate(src), off(src), np.concatenate(tgt), off(tgt), PAD, EOS, lps, lpt)


def host_batch(P, src, tgt, idx, lps, lpt, mult):
    samples = [{"id": i, "source": torch.from_numpy(src[i].astype(np.int64)), "target": torch.from_numpy(tgt[i].astype(np.int64))} for i in idx]
    return P.collate(samples, PAD, EOS, lps, lpt, True, mult)


def check_against_host(rp, host):
    """The four outputs of one launch into a sentinel-filled buffer, bit for bit the host collater's; no word left unwritten."""
    ids = host["id"]
    B, S, T = ids.numel(), host["net_input"]["src_tokens"].size(1), host["target"].size(1)
    out = torch.full((B * S + 2 * B * T + B,), SENTINEL, dtype=torch.int64, device="cuda")
    st, sl, prev, target = rp.collate(ids, S, T, out=out)
    torch.cuda.synchronize()
    assert int((out == SENTINEL).sum()) == 0
    assert st.dtype == sl.dtype == prev.dtype == target.dtype == torch.int64
    assert torch.equal(st.cpu(), host["net_input"]["src_tokens"]) and torch.equal(sl.cpu(), host["net_input"]["src_lengths"])
    assert torch.equal(prev.cpu(), host["net_input"]["prev_output_tokens"]) and torch.equal(target.cpu(), host["target"])


BATCHES = {
    "one_token": [0],                          # B = 1, a sentence that is eos alone
    "cross_wave": [0, 1, 2],                   # lengths {1, 7, 65}
    "wide_rows": [4, 8, 2, 3, 10, 11, 6, 9, 1, 5, 7, 0, 4, 8, 2, 3],  # T = 130, 16 rows: several blocks; indices repeat
    "last_and_repeat": [11, 11, 5, 11],        # the corpus's last sentence, a repeated index
    "odd_offsets": [1, 3, 5, 6, 9],            # sentences behind odd-length ones
}


@pytest.mark.parametrize("name", sorted(BATCHES))
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("lps,lpt", [(True, False), (False, False), (True, True), (False, True)])
def test_collate_pairs_equals_the_host_collater(name, dtype, lps, lpt):
    P, _, _, _ = mods()
    src, tgt = corpus(dtype)
    if dtype == np.uint16 and name == "odd_offsets":
        offs = np.cumsum([0] + SRC_LENS)
        assert any(offs[i] % 2 for i in BATCHES[name])
    rp = resident(P, src, tgt, lps, lpt)
    for mult in (1, 8):  # --required-seq-len-multiple
        check_against_host(rp, host_batch(P, src, tgt, BATCHES[name], lps, lpt, mult))


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_collate_pairs_other_stream_types(dtype):
    P, _, _, _ = mods()
    src, tgt = corpus(dtype)
    rp = resident(P, src, tgt, True, False)
    check_against_host(rp, host_batch(P, src, tgt, BATCHES["wide_rows"], True, False, 1))
    # a narrower source stream beside a wider target stream is widened once, at construction
    src16, _ = corpus(np.uint8)
    _, tgt32 = corpus(np.int32)
    check_against_host(resident(P, src16, tgt32, True, False), host_batch(P, src16, tgt32, [2, 0, 7], True, False, 1))


def test_collate_pairs_is_reproducible_and_guards_its_arguments():
    P, K, _, _ = mods()
    src, tgt = corpus(np.uint16)
    rp = resident(P, src, tgt, True, False)
    idx = torch.tensor(BATCHES["wide_rows"])
    a = torch.cat([t.reshape(-1) for t in rp.collate(idx, 130, 130)])
    b = torch.cat([t.reshape(-1) for t in rp.collate(idx, 130, 130)])
    assert torch.equal(a, b)
    # an index outside the corpus yields a pad row of length 0 and reads nothing
    st, sl, prev, target = rp.collate(torch.tensor([1, len(src), -1]), 7, 3)
    assert sl.tolist() == [7, 0, 0] and bool((st[1:] == PAD).all()) and bool((prev[1:] == PAD).all()) and bool((target[1:] == PAD).all())
    s, so, t, to = rp._dev
    dev_idx = idx.cuda()
    with pytest.raises(ValueError, match="out must be"):
        K.collate_pairs(s, t, rp.tok_dtype, so, to, dev_idx, 130, 130, PAD, EOS, True, False, out=torch.empty(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="bad token dtype"):
        K.collate_pairs(s, t, 9, so, to, dev_idx, 130, 130, PAD, EOS, True, False)
    with pytest.raises(RuntimeError, match="bad shape"):
        K.collate_pairs(s, t, rp.tok_dtype, so, to, dev_idx, 0, 130, PAD, EOS, True, False)
    with pytest.raises(ValueError, match="rise from 0"):
        P.ResidentPairs(np.concatenate(src), np.array([0, 5, 3]), np.concatenate(tgt), np.array([0, 5, 3]), PAD, EOS)


def translation_task(**over):
    _, _, tasks, _ = mods()
    a = Namespace(data=ROOT, source_lang=None, target_lang=None, left_pad_source="True", left_pad_target="False", max_source_positions=20,
                  max_target_positions=20, required_seq_len_multiple=1, dataset_impl=None, eval_bleu=False)
    for k, v in over.items():
        setattr(a, k, v)
    return tasks.TranslationTask.setup_task(a)


@pytest.mark.parametrize("split", ["train", "valid32"])
def test_resident_batches_equal_the_reference_fixture(split, monkeypatch):
    """The task's own route on the fixture corpus (uint16 and int32 streams): every batch of an epoch, assembled on the device from the
    collater's record, against the batches the reference collated."""
    monkeypatch.delenv("CST_PAIR_COLLATE", raising=False)
    P, _, _, _ = mods()
    g = load_golden("translation_tiny.npz")
    t = translation_task()
    ds = t.load_dataset(split)
    assert ds.resident is not None and ds.resident.tok_dtype == (1 if split == "train" else 2)
    it = t.get_batch_iterator(ds, max_tokens=40, max_positions=(20, 20), ignore_invalid_inputs=True, seed=1)
    records = list(it.next_epoch_itr(shuffle=(split == "train")))
    assert len(records) == int(g[split + "/collated/n"])
    for j, rec in enumerate(records):
        assert P.is_pair_record(rec) and rec["target"] is None
        s = ds.resident.materialize(rec)
        key = "%s/collated/%d" % (split, j)
        assert s["id"].tolist() == g[key + "/id"].tolist() and s["ntokens"] == int(g[key + "/ntokens"])
        for k in ("src_tokens", "src_lengths", "prev_output_tokens"):
            np.testing.assert_array_equal(s["net_input"][k].cpu().numpy(), g[key + "/" + k], err_msg=key + k)
        np.testing.assert_array_equal(s["target"].cpu().numpy(), g[key + "/target"])
    # the budget decides the default route; CST_PAIR_COLLATE=host forces the host one
    monkeypatch.setenv("CST_RESIDENT_CORPUS_MB", "0.0001")
    assert t.load_dataset(split).resident is None
    monkeypatch.setenv("CST_RESIDENT_CORPUS_MB", "64")
    assert t.load_dataset(split).resident is not None
    monkeypatch.setenv("CST_PAIR_COLLATE", "host")
    assert t.load_dataset(split).resident is None


# ---- the two routes end to end ---------------------------------------------------------------------------------------------------
def tiny_flags(save, train_subset="train"):
    return [ROOT, "--task", "translation", "--train-subset", train_subset, "--valid-subset", "valid", "--save-dir", save, "--max-tokens", "40",
            "--max-source-positions", "20", "--max-target-positions", "20", "--skip-invalid-size-inputs-valid-test",
            "--criterion", "label_smoothed_cross_entropy", "--label-smoothing", "0.1",
            "--eval-bleu-args", json.dumps(dict(GEN)), "--eval-bleu", "--eval-bleu-detok", "moses", "--eval-bleu-remove-bpe",
            "--eval-bleu-print-samples", "--best-checkpoint-metric", "bleu", "--maximize-best-checkpoint-metric",
            "--arch", "s2t_transformer_w2v2_interlingua_base", "--share-decoder-input-output-embed",
            "--w2v2-model-path", "synthetic:golden_tiny", "--encoder-layers", "2", "--encoder-embed-dim", "64",
            "--encoder-ffn-embed-dim", "128", "--encoder-attention-heads", "2", "--decoder-attention-heads", "2", "--decoder-layers", "2",
            "--conv-channels", "64", "--interlingua-length", "8", "--interlingua-layers", "2", "--dropout", "0.1",
            "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--clip-norm", "0.0", "--lr", "2e-3", "--lr-scheduler", "inverse_sqrt",
            "--weight-decay", "0.0001", "--warmup-updates", "2", "--fp16", "--update-freq", "1", "--num-workers", "1",
            "--ddp-backend", "no_c10d", "--seed", "1", "--log-interval", "1"]


def run_mt(save, route, extra, validate=None):
    """train_main on the fixture corpus -> (trainer, its JSON events, what every validation returned)."""
    _, _, _, cli = mods()
    w2t = import_module("chimera-st_amd.w2v2_transformer")
    w2t.SYNTHETIC_W2V["golden_tiny"] = Namespace(**ast.literal_eval(str(load_golden("chimera_tiny.npz")["meta/w2v_args"])))
    stats, orig, prev = [], cli.validate, os.environ.get("CST_PAIR_COLLATE")

    def recording(*a, **k):
        stats.append(validate(len(stats)) if validate is not None else orig(*a, **k))
        return stats[-1]

    cli.validate = recording
    if route is not None:
        os.environ["CST_PAIR_COLLATE"] = route
    else:
        os.environ.pop("CST_PAIR_COLLATE", None)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            tr = cli.train_main(tiny_flags(save) + extra)
    finally:
        cli.validate = orig
        os.environ.pop("CST_PAIR_COLLATE", None)
        if prev is not None:
            os.environ["CST_PAIR_COLLATE"] = prev
    return tr, [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")], stats


@pytest.fixture(scope="module")
def mt_run(tmp_path_factory):
    """Two updates and one validation with --eval-bleu on the resident route (the default); the checkpoints serve the driver tests."""
    save = str(tmp_path_factory.mktemp("mt_resident"))
    tr, ev, stats = run_mt(save, None, ["--max-update", "2"])
    return dict(save=save, trainer=tr, events=ev, stats=stats)


def test_the_two_routes_train_and_validate_bit_identically(mt_run, tmp_path):
    tr_r, ev_r, st_r = mt_run["trainer"], mt_run["events"], mt_run["stats"]
    assert tr_r.task.datasets["train"].resident is not None and tr_r.task.datasets["valid"].resident is not None
    save = str(tmp_path / "mt_host")
    tr_h, ev_h, st_h = run_mt(save, "host", ["--max-update", "2"])
    assert tr_h.task.datasets["train"].resident is None and tr_h.task.datasets["valid"].resident is None
    inner = lambda ev: [(e["num_updates"], e["loss"], e["gnorm"], e["ntokens"]) for e in ev if e["event"] == "train_inner"]
    assert len(inner(ev_r)) == 2 and inner(ev_r) == inner(ev_h)  # losses and gradient norms, bit for bit
    assert len(st_r) == len(st_h) == 1 and st_r[0] == st_h[0]
    bleu_keys = {"_bleu_sys_len", "_bleu_ref_len"} | {"_bleu_%s_%d" % (k, i) for k in ("counts", "totals") for i in range(4)}
    assert bleu_keys <= set(st_r[0]) and "bleu" in st_r[0] and st_r[0]["_bleu_ref_len"] > 0 and st_r[0]["_bleu_sys_len"] > 0
    valid = [e for e in ev_r if e["event"] == "valid"]
    assert len(valid) == 1 and valid[0]["bleu"] == st_r[0]["bleu"] and not any(k.startswith("_") for k in valid[0])
    a = torch.load(os.path.join(mt_run["save"], "checkpoint_last.pt"), weights_only=False)
    b = torch.load(os.path.join(save, "checkpoint_last.pt"), weights_only=False)
    assert list(a["model"]) == list(b["model"])
    # (`_float_tensor` of the sinusoidal tables is the reference's one-element placeholder buffer: never written, never read)
    differ = [k for k in a["model"] if not k.endswith("._float_tensor") and not torch.equal(a["model"][k], b["model"][k])]
    assert not differ, differ[:8]
    assert {n for n, _ in tr_r.get_model().named_parameters()} <= set(a["model"])
    assert a["args"].task == "translation" and os.path.exists(os.path.join(mt_run["save"], "checkpoint_best.pt"))
    assert torch.equal(tr_r.buffers.flat_param, tr_h.buffers.flat_param)


# ---- text decoding against the reference ---------------------------------------------------------------------------------------
def golden_model():
    from test_model_gpu import build_from_golden
    return build_from_golden(load_golden("chimera_tiny.npz"), "chimera", torch.float32)


def valid_batches(g):
    for j in range(int(g["valid/collated/n"])):
        key = "valid/collated/%d" % j
        yield j, {"net_input": {k: torch.from_numpy(g[key + "/" + k]).cuda() for k in ("src_tokens", "src_lengths", "prev_output_tokens")},
                  "target": torch.from_numpy(g[key + "/target"]).cuda(), "ntokens": int(g[key + "/ntokens"]),
                  "nsentences": int(g[key + "/nsentences"])}


@pytest.mark.parametrize("fused", [True, False])
def test_text_decoding_reproduces_the_reference_hypotheses(fused):
    """The engine (fused) and the host loop on the fixture's TEXT batches: token ids exact, scores within the 1e-4 of
    decode_recipe_tiny.npz's comparison of the same kind."""
    mods()
    SG = import_module("chimera-st_amd.sequence_generator")
    g = load_golden("translation_tiny.npz")
    assert ast.literal_eval(str(g["gen/settings"])) == dict(beam_size=5, max_len_a=1.2, max_len_b=10)
    model, task, _ = golden_model()
    gen = SG.SequenceGenerator([model], task.target_dictionary, beam_size=5, max_len_a=1.2, max_len_b=10, fused=fused)
    assert gen.fused == fused
    n = 0
    for j, sample in valid_batches(g):
        hyps = gen.generate([model], sample)
        assert len(hyps) == sample["nsentences"]
        for b, h in enumerate(hyps):
            assert len(h) == int(g["gen/%d/b%d/n" % (j, b)])
            for r, hyp in enumerate(h):
                key = "gen/%d/b%d/r%d/" % (j, b, r)
                assert hyp["tokens"].tolist() == g[key + "tokens"].tolist(), key
                assert abs(float(hyp["score"]) - float(g[key + "score"])) < 1e-4, key
                assert float((hyp["positional_scores"].cpu() - torch.from_numpy(g[key + "pos_scores"])).abs().max()) < 1e-4, key
                n += 1
    assert n == 8 * 5


def test_eval_bleu_statistics_equal_the_host_loop():
    """valid_step's statistics (hypotheses from the device engine) against the same count made here from the host loop's hypotheses."""
    _, _, tasks, _ = mods()
    SG = import_module("chimera-st_amd.sequence_generator")
    Bm = import_module("chimera-st_amd.bleu")
    crit = import_module("chimera-st_amd.criterions").LabelSmoothedCrossEntropyCriterion
    g = load_golden("translation_tiny.npz")
    model, _, _ = golden_model()
    t = translation_task(eval_bleu=True, eval_bleu_remove_bpe=None, eval_bleu_detok="space", eval_bleu_print_samples=False)
    t.tokenizer, t.bpe = Bm.build_detokenizer("space", None), None
    t.sequence_generator = t.build_generator([model], Namespace(**GEN))
    assert t.sequence_generator.fused and (t.sequence_generator.beam_size, t.sequence_generator.max_len_a, t.sequence_generator.max_len_b) == (5, 1.2, 10)
    host = SG.SequenceGenerator([model], t.target_dictionary, beam_size=5, max_len_a=1.2, max_len_b=10, fused=False)
    c = crit(t, False, 0.1)
    total = {}
    for j, sample in valid_batches(g):
        _, _, log = t.valid_step(sample, model, c)
        hyps, refs = t.bleu_strings([h[0]["tokens"].tolist() for h in host.generate([model], sample)], sample["target"].cpu())
        want = Bm.corpus_stats(hyps, refs)
        assert {k: log[k] for k in want} == want and want["_bleu_ref_len"] == int((sample["target"] != PAD).sum()) - sample["nsentences"]
        assert "loss" in log and "ntokens" in log
        for k in want:
            total[k] = total.get(k, 0) + log[k]
    assert total["_bleu_sys_len"] > 0 and 0.0 <= t.derived_metrics(total)["bleu"] <= 100.0


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
def test_generate_decodes_the_test_split_from_the_binarised_data(mt_run, capsys):
    """generate-wmt17.sh's command line.  fairseq-generate prints the groups as the batches come (by length, as the reference); per
    sentence id there is exactly one S-/T-/H-/D-/P- group, in that order, and S- / T- are the corpus's own sentences."""
    _, _, _, cli = mods()
    capsys.readouterr()
    summary = cli.generate_main([ROOT, "--path", os.path.join(mt_run["save"], "checkpoint_best.pt"), "--max-tokens", "400", "--beam", "5", "--remove-bpe"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l[:2] in ("S-", "T-", "H-", "D-", "P-")]
    assert summary["sentences"] == 6 and summary["subset"] == "test"
    groups = {}
    for l in lines:
        sid = int(l[2:].split("\t")[0])
        groups.setdefault(sid, []).append(l)
    assert sorted(groups) == list(range(6))
    for sid in sorted(groups):  # in id order: the corpus text beside it
        assert [l[0] for l in groups[sid]] == ["S", "T", "H", "D", "P"]
    unk = lambda s: " ".join(w if w.startswith("w") else "<unk>" for w in s.split())
    for lang, tag in (("en", 0), ("de", 1)):
        with open(os.path.join(ROOT, "corpus", "test.%s.txt" % lang), encoding="utf-8") as f:
            for sid, text in enumerate(f.read().split("\n")[:6]):
                assert groups[sid][tag].split("\t", 1)[1] == unk(text), (lang, sid)


def test_best_checkpoint_follows_bleu_upwards_only(tmp_path):
    """--best-checkpoint-metric bleu --maximize-best-checkpoint-metric over two epochs with stubbed validation results."""
    for name, scores, best_epoch in (("worse", [10.0, 5.0], 1), ("better", [5.0, 10.0], 2)):
        save = str(tmp_path / name)
        _, _, cli = mods()[1:]
        w2t = import_module("chimera-st_amd.w2v2_transformer")
        w2t.SYNTHETIC_W2V["golden_tiny"] = Namespace(**ast.literal_eval(str(load_golden("chimera_tiny.npz")["meta/w2v_args"])))
        calls, orig = [], cli.validate
        cli.validate = lambda *a, **k: (calls.append(1), {"loss": 1.0, "bleu": scores[len(calls) - 1]})[1]
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                cli.train_main(tiny_flags(save, train_subset="valid") + ["--max-epoch", "2"])  # (the 8-pair split: two batches an epoch)
        finally:
            cli.validate = orig
        assert len(calls) == 2
        best = torch.load(os.path.join(save, "checkpoint_best.pt"), weights_only=False)
        last = torch.load(os.path.join(save, "checkpoint_last.pt"), weights_only=False)
        # (a checkpoint written after epoch e resumes at epoch e + 1)
        assert best["extra_state"]["train_iterator"]["epoch"] == best_epoch + 1 and best["extra_state"]["best"] == 10.0
        assert last["extra_state"]["train_iterator"]["epoch"] == 3 and last["extra_state"]["best"] == 10.0


def test_the_st_stage_starts_from_the_mt_checkpoint(mt_run, tmp_path, capsys):
    """train-en2any-ST.sh:19 copies the MT stage's checkpoint_best.pt to checkpoint_last.pt and trains `triplet` with --reset-optimizer."""
    from test_cli_gpu import DATA, _tiny_cli_flags
    _, _, _, cli = mods()
    root = tmp_path / "data"
    root.mkdir()
    for f in os.listdir(DATA):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(DATA, f), root / f)
    (root / "config_wave.yaml").write_text((root / "config_wave.yaml").read_text().replace("AUDIO_ROOT", DATA))
    shutil.copy(os.path.join(ROOT, "dict.en.txt"), root / "dict.txt")  # the joint dictionary of both stages
    save = tmp_path / "st"
    save.mkdir()
    shutil.copy(os.path.join(mt_run["save"], "checkpoint_best.pt"), save / "checkpoint_last.pt")
    mt = torch.load(save / "checkpoint_last.pt", weights_only=False)
    capsys.readouterr()
    tr = cli.train_main(_tiny_cli_flags(root, str(save), "synthetic:golden_tiny") + ["--reset-optimizer", "--lr", "0.0", "--max-update", "1",
                                                                                    "--disable-validation", "--no-save"])
    ev = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    loaded = [e for e in ev if e["event"] == "loaded_checkpoint"]
    assert loaded and loaded[0]["num_updates"] == 0 and tr.num_updates == 1  # the optimizer starts over
    sd = tr.get_model().state_dict()  # (learning rate 0: the parameters are still the MT stage's)
    assert set(sd) == set(mt["model"])
    for k, v in mt["model"].items():
        a, b = sd[k].float().cpu(), v.float().to(sd[k].dtype).float()
        # (`_float_tensor` of the sinusoidal tables is the reference's one-element placeholder buffer, never written: where the
        #  allocator hands out a NaN, the loaded NaN is the same value and still not `equal`)
        assert torch.equal(a, b) or (k.endswith("._float_tensor") and torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)), k
