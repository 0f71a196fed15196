"""Training and evaluating the fusion LM on a real MI355X: the `language_modeling` task, the `cross_entropy` criterion and
`transformer_lm` against what the reference computed on the fixture (tests/golden/lm_tiny.npz: tools/ref_harness/make_lm_goldens.py);
the device and host batch routes through the Trainer; fairseq_train.py -> fairseq_eval_lm.py -> fairseq_generate.py --lm-path."""
import ast
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
from parity_util import assert_grads_close_fp32, max_abs_rel

pytestmark = pytest.mark.gpu

ROOT = os.path.join(GOLDEN, "lm_tiny")
PAD = 1


@pytest.fixture(scope="module")
def g():
    return load_golden("lm_tiny.npz")


def lm_task(mode="none", tokens_per_sample=16, **over):
    load_pkg()
    tasks = import_module("chimera-st_amd.tasks")
    a = Namespace(data=ROOT, sample_break_mode=mode, tokens_per_sample=tokens_per_sample, max_target_positions=None, dataset_impl=None)
    for k, v in over.items():
        setattr(a, k, v)
    return tasks.LanguageModelingTask.setup_task(a)


def fixture_model(g, task, dtype=torch.float32):
    import_module("chimera-st_amd.transformer_lm")
    args = Namespace(**ast.literal_eval(str(g["meta/lm_args"])))
    model = task.build_model(args)
    sd = {k[len("lm/param/"):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith("lm/param/")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    assert sorted(model.state_dict().keys()) == [str(k) for k in g["meta/lm_keys"]]  # the reference's state-dict keys
    return model.to("cuda", dtype), args


def fixture_batch(g, key):
    return {"id": torch.from_numpy(g[key + "/id"]), "nsentences": int(g[key + "/nsentences"]), "ntokens": int(g[key + "/ntokens"]),
            "net_input": {"src_tokens": torch.from_numpy(g[key + "/src_tokens"]).cuda(), "src_lengths": torch.from_numpy(g[key + "/src_lengths"]).cuda()},
            "target": torch.from_numpy(g[key + "/target"]).cuda()}


@pytest.mark.parametrize("tag", ["full", "padded"])
def test_cross_entropy_update_matches_the_reference(g, tag):
    """fp32: loss within 1e-4 relative; logits and every gradient within 1e-3 * max(1, |ref|max); a ReLU tie (a pre-activation the
    reference found within 1e-4 of zero) is excused by assert_grads_close_fp32 within its caps only."""
    task = lm_task()
    model, _ = fixture_model(g, task)
    crit = import_module("chimera-st_amd.criterions").CrossEntropyCriterion(task, False).cuda()
    key = str(g["crit/%s/batch" % tag])
    sample = fixture_batch(g, key)
    assert bool((sample["target"] == PAD).any()) == (tag == "padded")
    model.train()
    loss, sample_size, log = crit(model, sample)
    loss.backward()
    ref_loss = float(g["crit/%s/loss" % tag])
    print("loss %.6f reference %.6f" % (float(loss.detach()), ref_loss))
    assert sample_size == int(g["crit/%s/sample_size" % tag]) == sample["ntokens"]
    assert sorted(log) == ["loss", "nsentences", "ntokens", "sample_size"]
    assert log["ntokens"] == int(g["crit/%s/log_ntokens" % tag]) and log["nsentences"] == int(g["crit/%s/log_nsentences" % tag])
    assert abs(float(loss.detach()) - ref_loss) <= 1e-4 * abs(ref_loss), (float(loss.detach()), ref_loss)
    with torch.no_grad():
        logits = model(**sample["net_input"])[0]
    e = max_abs_rel(logits, g["crit/%s/logits" % tag])
    print("logits max-abs-rel %.3e" % e)
    assert e <= 1e-3
    pre = "crit/%s/grad/" % tag
    ref = {k[len(pre):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre)}
    got = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(got) == sorted(ref) and all(v is not None for v in got.values())
    taps = {k[len("crit/%s/relu_min_abs/" % tag):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("crit/%s/relu_min_abs/" % tag)}
    assert sorted(taps) == ["decoder.layers.0.fc1", "decoder.layers.1.fc1"]
    n, worst, excused = assert_grads_close_fp32(got, ref, taps)
    print("gradients compared %d, worst %s %.3e, tie rows excused %d" % (n, worst[0], worst[1], excused))
    assert n == len(ref)


def _targs():
    return Namespace(bf16=False, lr=[1e-3], adam_betas="(0.9, 0.98)", adam_eps=1e-8, weight_decay=0.0, clip_norm=0.0,
                     warmup_updates=1, warmup_init_lr=1e-3, seed=1, bucket_cap_mb=0.05)


def _three_updates(g, route, monkeypatch):
    monkeypatch.setenv("CST_BLOCK_COLLATE", route)
    monkeypatch.setenv("CST_RESIDENT_CORPUS_MB", "64")
    task = lm_task("eos")
    ds = task.load_dataset("train")
    assert (ds.resident is not None) == (route == "device")
    model, _ = fixture_model(g, task)
    crit = import_module("chimera-st_amd.criterions").CrossEntropyCriterion(task, False)
    tr = import_module("chimera-st_amd.trainer").Trainer(_targs(), task, model, crit, device="cuda")
    itr = task.get_batch_iterator(ds, max_tokens=48, max_positions=task.max_positions(), ignore_invalid_inputs=True, seed=1)
    M = import_module("chimera-st_amd.monolingual_dataset")
    outs, ids = [], []
    for i, sample in enumerate(itr.next_epoch_itr(shuffle=True)):
        if i == 3:
            break
        assert M.is_block_record(sample) == (route == "device")
        ids.append(sample["id"].tolist())
        outs.append(tr.train_step([sample]))
    torch.cuda.synchronize()
    return tr.buffers.flat_param.detach().clone(), outs, ids


def test_device_and_host_batches_give_the_same_three_updates(g, monkeypatch):
    pd, od, idd = _three_updates(g, "device", monkeypatch)
    ph, oh, idh = _three_updates(g, "host", monkeypatch)
    assert idd == idh and len(od) == 3
    assert [o["loss"] for o in od] == [o["loss"] for o in oh] and [o["ntokens"] for o in od] == [o["ntokens"] for o in oh]
    assert torch.equal(pd, ph)  # the batches are identical and the update is bit-reproducible


def _events(text):
    return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


def test_train_eval_lm_and_fuse_from_the_command_line(g, tmp_path, capsys):
    """fairseq_train.py (bf16, three epochs) -> fairseq_eval_lm.py on the checkpoint -> fairseq_generate.py --lm-path with it."""
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    cu = import_module("chimera-st_amd.checkpoint_utils")
    save = str(tmp_path / "ckpt")
    flags = [ROOT, "--task", "language_modeling", "--arch", "transformer_lm", "--criterion", "cross_entropy", "--share-decoder-input-output-embed",
             "--decoder-layers", "2", "--decoder-embed-dim", "64", "--decoder-ffn-embed-dim", "128", "--decoder-attention-heads", "2",
             "--dropout", "0.0", "--sample-break-mode", "none", "--tokens-per-sample", "16", "--max-tokens", "48", "--save-dir", save,
             "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--lr", "5e-3", "--lr-scheduler", "inverse_sqrt", "--warmup-updates", "2",
             "--clip-norm", "0.0", "--fp16", "--seed", "1", "--log-interval", "1", "--no-epoch-checkpoints", "--max-epoch", "3"]
    tr = cli.train_main(flags)
    ev = _events(capsys.readouterr().out)
    assert ev[0]["event"] == "start" and ev[0]["task"] == "language_modeling" and ev[0]["criterion"] == "cross_entropy" and ev[0]["dtype"] == "torch.bfloat16"
    train = [e for e in ev if e["event"] == "train"]
    valid = [e for e in ev if e["event"] == "valid"]
    print("train losses", [e["loss"] for e in train], "valid", [(e["loss"], e["ppl"]) for e in valid])
    assert len(train) == 3 and len(valid) == 3 and train[-1]["loss"] < train[0]["loss"]
    assert all("loss" in e and "ppl" in e and e["ppl"] == round(2 ** e["loss"], 2) for e in valid) and all("ppl" in e for e in train)
    last = os.path.join(save, "checkpoint_last.pt")
    d = tr.task.target_dictionary
    lm = cu.load_language_model(last, d)  # strict, the reference's keys
    assert sorted(lm.state_dict().keys()) == [str(k) for k in g["meta/lm_keys"]]
    assert lm.decoder.output_projection.weight is lm.decoder.embed_tokens.weight
    # eval-lm on the trained checkpoint at the training run's settings: its loss IS the training CLI's valid loss
    s = cli.eval_lm_main([ROOT, "--path", last, "--gen-subset", "valid", "--max-tokens", "48", "--fp16"])
    out = capsys.readouterr().out
    assert "Loss (base 2): %.4f, Perplexity: %.2f" % (s["loss"], s["ppl"]) in out and "Evaluated %d tokens in" % s["tokens"] in out
    print("eval-lm loss %.6f, training valid loss %.6f" % (s["loss"], valid[-1]["loss"]))
    assert s["count"] == s["tokens"] == int(g["eval_lm/valid/none/count"])
    assert abs(s["loss"] - valid[-1]["loss"]) <= 1e-4 * abs(valid[-1]["loss"])
    # fairseq_generate.py --lm-path accepts the checkpoint on the existing decode fixture
    from test_ensemble_gpu import fixture_members
    models, task, args, _ = fixture_members(1)
    data = os.path.join(GOLDEN, "data_tiny")
    root = tmp_path / "data"
    root.mkdir()
    for f in os.listdir(data):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(data, f), root / f)
    (root / "config_wave.yaml").write_text((root / "config_wave.yaml").read_text().replace("AUDIO_ROOT", data))
    lines = (root / "dict.txt").read_text().splitlines()
    V = models[0].decoder.embed_tokens.num_embeddings
    assert V == len(d)
    lines += ["filler%d 1" % i for i in range(V - 4 - len(lines))]
    (root / "dict.txt").write_text("\n".join(lines) + "\n")
    a = Namespace(**vars(args))
    a.arch, a.task, a.no_save_optimizer_state = "s2t_transformer_w2v2_interlingua_base", "triplet", True
    a.data, a.config_yaml = str(root), "config_wave.yaml"
    m_path = str(tmp_path / "m.pt")
    cu.save_state(m_path, a, models[0].state_dict(), None, None, 0)
    summary = cli.generate_main([str(root), "--task", "triplet", "--config-yaml", "config_wave.yaml", "--gen-subset", "dev_st", "--max-tokens", "12000",
                                 "--beam", "5", "--max-len-b", "12", "--max-source-positions", "2000000", "--path", m_path,
                                 "--lm-path", last, "--lm-weight", "0.3"])
    out = capsys.readouterr().out.splitlines()
    assert summary["lm_path"] == last and summary["sentences"] == sum(l.startswith("H-") for l in out) > 0


@pytest.mark.parametrize("mode", ["none", "eos"])
def test_eval_lm_matches_the_reference_on_the_fixture_model(g, mode, tmp_path, capsys):
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    cu = import_module("chimera-st_amd.checkpoint_utils")
    task = lm_task(mode)
    model, args = fixture_model(g, task)
    a = Namespace(**vars(args))
    a.task, a.data, a.sample_break_mode, a.no_save_optimizer_state = "language_modeling", ROOT, "complete", True  # (the run's mode: overridden below)
    a.tokens_per_sample = 16
    path = str(tmp_path / "lm.pt")
    cu.save_state(path, a, model.state_dict(), None, None, 0)
    s = cli.eval_lm_main([ROOT, "--path", path, "--gen-subset", "valid", "--max-tokens", "48", "--sample-break-mode", mode, "--softmax-batch", "1024"])
    capsys.readouterr()
    k = "eval_lm/valid/%s" % mode
    print("eval-lm %s: count %d loss %.6f; reference count %d loss %.6f" % (mode, s["count"], s["loss"], int(g[k + "/count"]), float(g[k + "/loss"])))
    assert s["count"] == int(g[k + "/count"]) and s["sample_break_mode"] == mode
    assert abs(s["loss"] - float(g[k + "/loss"])) <= 1e-4 * abs(float(g[k + "/loss"]))
    assert abs(s["ppl"] - 2 ** s["loss"]) < 1e-9 and math.isfinite(s["score_sum"])
