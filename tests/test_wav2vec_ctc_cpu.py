"""No-GPU checks of CTC fine-tuning against tests/golden/ctc_tiny.npz (recorded from the real reference): the fine-tuning masks for a
numpy seed, the model's state-dict keys and strict loading, post_process, the masking's gradient rule, the labelled audio dataset's
sample layout, and the audio_pretraining task's refusal without --labels."""
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import wav2vec_ctc_util as U
from conftest import load_pkg


@pytest.fixture(scope="module")
def g():
    return U.fixture()


@pytest.mark.parametrize("case", ["pad_3x50", "nopad_3x50", "pad_2x137", "nopad_2x137"])
def test_mask_indices_equal_the_reference(g, case):
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    ref_t, ref_c = g["mask/%s/time" % case], g["mask/%s/channel" % case]
    lens = g["mask/%s/lengths" % case].tolist() if "mask/%s/lengths" % case in g else None
    np.random.seed(int(g["meta/seed"]))
    t = W.compute_mask_indices(ref_t.shape, lens, 0.5, 10, "static", 0, min_masks=2, no_overlap=False, min_space=1)
    c = W.compute_mask_indices(ref_c.shape, None, 0.25, 8, "static", 0, no_overlap=False, min_space=1)
    assert np.array_equal(t, ref_t) and np.array_equal(c, ref_c)
    if lens is not None:
        assert not any(t[b, n:].any() for b, n in enumerate(lens))


def test_other_mask_selections_run_and_respect_lengths():
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    np.random.seed(1)
    for kind, other in (("uniform", 2), ("normal", 2.0), ("poisson", 0)):
        m = W.compute_mask_indices((3, 80), [80, 50, 61], 0.4, 6, kind, other, min_masks=2)
        assert m.shape == (3, 80) and m.any() and not m[1, 50:].any() and len(set(m.sum(1).tolist())) == 1
    m = W.compute_mask_indices((2, 90), None, 0.5, 10, "static", 0, no_overlap=True, min_space=1)
    for row in m:  # spans do not touch: every run of masked frames is exactly one span long
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate(([0], row.astype(int), [0])))))[::2]
        assert (runs == 10).all()


def test_state_dict_keys_and_strict_load(g):
    model, _, args = U.build_model(g)
    keys = str(g["meta/keys"]).split("\n")
    assert list(model.state_dict().keys()) == keys
    assert not any(k.split(".")[2] in ("quantizer", "project_q", "final_proj", "target_glu") for k in keys)
    # a reference-shaped state dict loads strictly; ours has its shapes
    import argparse
    torch.serialization.add_safe_globals([argparse.Namespace])
    ck = torch.load(U.W2V, map_location="cpu")
    sd = {"w2v_encoder.w2v_model." + k: v for k, v in ck["model"].items() if "w2v_encoder.w2v_model." + k in keys}
    sd.update({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    assert set(sd) == set(keys)
    model.load_state_dict(sd, strict=True)
    assert all(tuple(model.state_dict()[k].shape) == tuple(sd[k].shape) for k in keys)
    # a checkpoint of this model rebuilds without the pre-trained file: args.w2v_args carries the configuration
    A = import_module("chimera-st_amd.wav2vec2_asr")
    again = A.Wav2VecCtc.build_model(Namespace(w2v_path=None, w2v_args=args.w2v_args, normalize=False), U.SimpleNamespace(target_dictionary=U.letter_dictionary(g)))
    again.load_state_dict(model.state_dict(), strict=True)
    assert model.get_normalized_probs({"encoder_out": torch.zeros(2, 1, 32)}, log_probs=True).exp().sum(-1).allclose(torch.ones(2, 1))


def test_post_process_equals_the_reference(g):
    load_pkg()
    C = import_module("chimera-st_amd.criterions")
    for sym in ("letter", "sentencepiece", "none", "@@ "):
        for s, want in zip(g["post/%s/in" % sym].tolist(), g["post/%s/out" % sym].tolist()):
            assert C.post_process(s, sym) == want


def test_masking_gradient_rule(g):
    """mask_emb receives the sum of the incoming gradient over the masked frames, channel-masked columns excluded; masked positions pass
    nothing back; unmasked ones pass the gradient through."""
    model, _, _ = U.build_model(g)
    w = model.w2v_encoder.w2v_model
    B, T, C = 2, 9, w.mask_emb.numel()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(B, T, C, generator=gen, requires_grad=True)
    tm = torch.rand(B, T, generator=gen) < 0.4
    cm = torch.rand(B, C, generator=gen) < 0.3
    go = torch.randn(B, T, C, generator=gen)
    y = w.apply_mask(x, tm, cm)
    y.backward(go)
    live = (~cm).unsqueeze(1).float()
    assert torch.equal(y, torch.where(cm.unsqueeze(1), torch.zeros(()), torch.where(tm.unsqueeze(-1), w.mask_emb.detach(), x.detach())))
    assert torch.allclose(w.mask_emb.grad, (go * live * tm.unsqueeze(-1).float()).sum((0, 1)), atol=1e-6)
    assert torch.equal(x.grad, go * live * (~tm).unsqueeze(-1).float())


def test_dataset_sample_layout_and_task(g, tmp_path):
    load_pkg()
    T = import_module("chimera-st_amd.tasks")
    rows = U.write_manifest(str(tmp_path), g)
    args = Namespace(data=str(tmp_path), labels="ltr", sample_rate=16000, normalize=True, max_sample_size=None, min_sample_size=None,
                     enable_padding=False, criterion="ctc", seed=1)
    task = T.AudioPretrainingTask.setup_task(args)
    d = task.target_dictionary
    assert len(d) == 32 and d.bos() == 0
    ds = task.load_dataset("train")
    assert len(ds) == 6
    batch = ds.collater([ds[i] for i in (0, 3, 4)])
    assert set(batch) == {"id", "net_input", "target", "target_lengths", "ntokens"} and set(batch["net_input"]) == {"source", "padding_mask"}
    assert batch["id"].tolist() == [0, 3, 4]
    S = max(rows["train"][i][1] for i in (0, 3, 4))
    assert batch["net_input"]["source"].shape == (3, S) and batch["net_input"]["source"].dtype == torch.float32
    for j, i in enumerate((0, 3, 4)):
        rel, ns, label, pcm = rows["train"][i]
        wav = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
        want = torch.nn.functional.layer_norm(wav, wav.shape)  # per-utterance normalisation, before the padding
        assert torch.allclose(batch["net_input"]["source"][j, :ns], want, atol=1e-6)
        assert not batch["net_input"]["source"][j, ns:].any()
        assert batch["net_input"]["padding_mask"][j].tolist() == [False] * ns + [True] * (S - ns)
        ids = [d.index(c) for c in label.split()]  # no eos appended, no new symbols
        assert batch["target"][j, :len(ids)].tolist() == ids and (batch["target"][j, len(ids):] == d.pad()).all()
        assert int(batch["target_lengths"][j]) == len(ids)
    assert batch["ntokens"] == int(batch["target_lengths"].sum()) and batch["target"].dtype == torch.int64
    # batches by size, sharded like the other datasets
    itr = task.get_batch_iterator(ds, max_tokens=9000, seed=1, num_shards=2, shard_id=1, max_positions=task.max_positions())
    seen = [i for b in itr.frozen_batches for i in b]
    assert sorted(seen) == list(range(6)) and all(sum(rows["train"][i][1] for i in b) <= 9000 * 2 for b in itr.frozen_batches)
    assert len(list(itr.next_epoch_itr(shuffle=False))) == len(itr)
    # cropping to max_sample_size
    args.max_sample_size = 2000
    short = T.AudioPretrainingTask.setup_task(args).load_dataset("valid")
    assert short.collater([short[0], short[1]])["net_input"]["source"].shape == (2, 2000)
    with pytest.raises(NotImplementedError, match="wav2vec2 pre-training is not built"):
        T.AudioPretrainingTask.setup_task(Namespace(data=str(tmp_path), labels=None))
    (tmp_path / "flac.tsv").write_text("%s\naudio/x.flac\t3000\n" % tmp_path)
    (tmp_path / "flac.ltr").write_text("A |\n")
    (tmp_path / "audio" / "x.flac").write_bytes(b"fLaC")
    with pytest.raises(Exception, match="(?i)flac"):
        task.load_dataset("flac")[0]


def test_oracle_restatement_equals_the_reference(g):
    """The oracle composition the bf16 parity test rounds (wav2vec_ctc_util.ctc_oracle) reproduces the fixture in plain fp32, within the 1e-3 of
    the model-parity tests (two fp32 evaluations of layer 0's GroupNorm backward already differ by 2e-4 in its weight gradient)."""
    from parity_util import max_abs_rel, run_oracle
    out, grads = run_oracle(U.ctc_oracle, U.full_state_dict(g), U.fixture_sample(g), U.oracle_cfg(g))
    live = ~torch.from_numpy(g["out/frame_padding_mask"]).t()
    assert torch.equal(out["padding_mask"], torch.from_numpy(g["out/frame_padding_mask"]))
    assert max_abs_rel(out["logits"].detach()[live], torch.from_numpy(g["out/logits"])[live]) < 1e-3
    assert max_abs_rel(out["nll"].detach(), torch.from_numpy(g["out/nll"])) < 1e-3
    assert abs(float(out["loss"]) - float(g["out/loss"])) < 1e-3 * abs(float(g["out/loss"]))
    for k, v in grads.items():
        ref = torch.from_numpy(g["grad/" + k])
        assert max_abs_rel(v if v is not None else torch.zeros_like(ref), ref) < 1e-3, k  # (mask_emb: unused, no gradient)


def test_readme_command_line_builds(g, tmp_path):
    """The flags the README gives — no --feature-grad-mult, no mask options — parse and build: every override that reaches the wav2vec2
    arguments has the architecture's default, none is None."""
    load_pkg()
    import_module("chimera-st_amd.cli")
    R = import_module("chimera-st_amd.registry")
    U.write_manifest(str(tmp_path), g, splits=(("train", 1),))
    args = R.parse_args_and_arch([str(tmp_path), "--task", "audio_pretraining", "--labels", "ltr", "--criterion", "ctc", "--arch", "wav2vec_ctc",
                                  "--w2v-path", U.W2V])
    assert args.feature_grad_mult == 0 and args.layerdrop == 0.0 and args.freeze_finetune_updates == 0 and args.post_process == "letter"
    task = R.setup_task(args)
    model = task.build_model(args)
    w = model.w2v_encoder.w2v_model
    assert w.feature_grad_mult == 0 and w.mask_prob == 0.5 and w.mask_channel_prob == 0.5 and w.encoder.layerdrop == 0.0
    assert not [k for k, v in vars(args.w2v_args).items() if v is None and k in ("dropout", "feature_grad_mult", "encoder_layerdrop", "mask_prob")]
    assert R.build_criterion(args, task).zero_infinity is False
    A = import_module("chimera-st_amd.wav2vec2_asr")
    ns = Namespace(feature_grad_mult=None, mask_prob=0.3)
    A.base_architecture(ns)
    assert ns.feature_grad_mult == 0 and ns.mask_prob == 0.3
