"""CTC fine-tuning on a real MI355X: the tiny wav2vec_ctc model against tests/golden/ctc_tiny.npz (the real reference on the CPU in
fp32: logits, losses, every parameter gradient, the eval-mode error counts), the freeze / masking behaviour, the command-line run
(audio_pretraining --labels ltr, criterion ctc, arch wav2vec_ctc) and an ST encoder built from the checkpoint it leaves."""
import json
import os
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import wav2vec_ctc_util as U
from conftest import load_pkg
from parity_util import max_abs_rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return U.fixture()


def criterion(task, **kw):
    return import_module("chimera-st_amd.criterions").CtcCriterion(task, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_model_parity_with_the_reference(g, dtype):
    """fp32 storage: logits, per-utterance nll, loss and every gradient within the 1e-3 of the model-parity tests
    (parity_util.max_abs_rel).  bf16 storage: by emulated storage rounding, the bounds of test_model_gpu.py — the oracle restatement
    (wav2vec_ctc_util.ctc_oracle, pinned to the fixture on the CPU) is re-run with every stored tensor rounded to bf16, and its distance
    to the fp32 fixture is the yardstick: logits within 2x + 1e-3, loss within 3x + 5e-4 relative, all gradients together within 1.5x
    their relative L2 error + 1e-3, every tensor with >= 1 % of the norm within 2x its own + 1e-2.  The eval counts exactly (fp32)."""
    from parity_util import run_oracle
    from test_model_gpu import assert_grads_close_bf16, emulated_tol
    CF = import_module("chimera-st_amd.functional")
    model, task, _ = U.build_model(g)
    model = model.to("cuda", dtype).train()
    sample = U.to_cuda(U.fixture_sample(g))
    crit = criterion(task)
    loss, sample_size, log = crit(model, sample)
    loss.backward()
    with torch.no_grad():
        net = model(**sample["net_input"])
        in_len = (~net["padding_mask"]).long().sum(-1)
        t = sample["target"]
        _, nll = CF.ctc_loss(net["encoder_out"], t, sample["target_lengths"], in_len, 0)
    assert net["encoder_out"].shape == g["out/logits"].shape and net["encoder_out"].dtype == dtype
    assert torch.equal(net["padding_mask"].cpu(), torch.from_numpy(g["out/frame_padding_mask"]))
    live = ~torch.from_numpy(g["out/frame_padding_mask"]).t()  # [T, B]: the frames behind an utterance's end are read by nobody
    ref_logits, ref_loss = torch.from_numpy(g["out/logits"])[live], float(g["out/loss"])
    tol_logits = tol_nll = tol_loss = 1e-3
    if dtype == torch.bfloat16:
        emu, egrads = run_oracle(U.ctc_oracle, U.full_state_dict(g), U.fixture_sample(g), U.oracle_cfg(g), storage=torch.bfloat16)
        tol_logits = emulated_tol(emu["logits"].detach()[live], ref_logits)
        tol_nll = emulated_tol(emu["nll"].detach(), torch.from_numpy(g["out/nll"]))
        tol_loss = 3 * abs(float(emu["loss"].detach()) - ref_loss) / abs(ref_loss) + 5e-4
    e = max_abs_rel(net["encoder_out"].float().cpu()[live], ref_logits)
    en = max_abs_rel(nll.cpu(), torch.from_numpy(g["out/nll"]))
    el = abs(float(loss.detach()) - ref_loss) / abs(ref_loss)
    print("PARITY wav2vec_ctc %s logits %.2e (tol %.2e) nll %.2e (tol %.2e) loss %.2e (tol %.2e)" % (dtype, e, tol_logits, en, tol_nll, el, tol_loss))
    assert e <= tol_logits and en <= tol_nll and el <= tol_loss and sample_size == int(g["in/target_lengths"].sum())
    if dtype == torch.bfloat16:
        assert_grads_close_bf16(model, g, egrads)  # (a parameter without a gradient — mask_emb — counts as zeros on both sides)
        return
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        got = p.grad.float().cpu() if p.grad is not None else torch.zeros(p.shape)
        err = max_abs_rel(got, torch.from_numpy(g["grad/" + k]))
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert err < 1e-3, (k, err)
    print("PARITY wav2vec_ctc worst gradient %s %.2e" % worst)
    model.eval()
    with torch.no_grad():
        _, _, elog = crit(model, sample)
    for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total"):
        assert int(elog[k]) == int(g["eval/" + k]), k


def test_freeze_finetune_updates(g):
    """With freeze_finetune_updates = 1 the first update runs the wav2vec2 stack without a graph: none of its parameters receives a
    gradient (the optimizer leaves them bit-equal), the projection does; from the second update on both do."""
    model, task, _ = U.build_model(g, freeze_finetune_updates=1)
    model = model.cuda().train()
    sample = U.to_cuda(U.fixture_sample(g))
    crit = criterion(task)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    for step, frozen in ((0, True), (1, False)):
        model.set_num_updates(step)
        opt.zero_grad(set_to_none=True)
        loss, _, _ = crit(model, sample)
        loss.backward()
        opt.step()
        after = model.state_dict()
        w2v_changed = [k for k in before if k.startswith("w2v_encoder.w2v_model.") and not torch.equal(before[k], after[k])]
        proj_changed = [k for k in before if k.startswith("w2v_encoder.proj.") and not torch.equal(before[k], after[k])]
        assert len(proj_changed) == 2
        if frozen:
            assert not w2v_changed
        else:
            assert len(w2v_changed) > 20 and "w2v_encoder.w2v_model.feature_extractor.conv_layers.0.0.weight" in w2v_changed
        before = {k: v.clone() for k, v in after.items()}


def test_apply_mask_is_seeded_and_trains_mask_emb(g):
    """Two runs of two UPDATES (forward, backward, optimizer step) with --apply-mask and a numpy seed are bit-equal; the masks differ
    from update to update; mask_emb's gradient inside the real model is the sum of the gradient arriving at the masked features over the
    masked frames, channel-masked columns excluded (a torch composition on the tensors the model itself masked)."""
    results = []
    for _ in range(2):
        model, task, _ = U.build_model(g, apply_mask=True, mask_prob=0.5, mask_length=4, mask_channel_prob=0.25, mask_channel_length=4)
        model = model.cuda().train()
        sample = U.to_cuda(U.fixture_sample(g))
        crit = criterion(task)
        w = model.w2v_encoder.w2v_model
        seen, inner = [], w.apply_mask

        def tapped(x, tmask, cmask):
            y = inner(x, tmask, cmask)
            y.retain_grad()
            seen.append((y, tmask, cmask))
            return y
        w.apply_mask = tapped
        opt = torch.optim.SGD(model.parameters(), lr=1e-4)
        np.random.seed(11)
        run = []
        for step in range(2):
            model.set_num_updates(step)
            opt.zero_grad(set_to_none=True)
            loss, _, _ = crit(model, sample)
            loss.backward()
            y, tm, cm = seen[-1]
            want = (y.grad.float() * tm.unsqueeze(-1) * (~cm).unsqueeze(1)).sum((0, 1))
            got = w.mask_emb.grad.float()
            # one fp32 sum over at most B * T = 297 masked frames on either side, in different orders: 2 x 297 u of the sum of magnitudes
            slack = 2 * 297 * 2.0 ** -24 * (y.grad.float().abs() * tm.unsqueeze(-1)).sum((0, 1))
            assert bool(((got - want).abs() <= slack + 1e-30).all()) and bool(got.ne(0).any())
            assert bool(got[cm.all(0)].eq(0).all())  # a column masked in every utterance receives nothing
            run.append((loss.detach().clone(), tm.clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
            opt.step()
        run.append({k: v.clone() for k, v in model.state_dict().items()})
        results.append(run)
    for (la, ta, ga), (lb, tb, gb) in zip(results[0][:2], results[1][:2]):
        assert torch.equal(la, lb) and torch.equal(ta, tb) and ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert all(torch.equal(results[0][2][k], results[1][2][k]) for k in results[0][2])  # the weights after two updates
    assert not torch.equal(results[0][0][1], results[0][1][1])  # the second update draws other masks
    model.eval()  # no masking in evaluation: equal to the same weights without the option
    plain, _, _ = U.build_model(g)
    plain.load_state_dict(model.state_dict())
    with torch.no_grad():
        a = model(**sample["net_input"])["encoder_out"]
        b = plain.cuda().eval()(**sample["net_input"])["encoder_out"]
    assert torch.equal(a, b)


def test_cli_finetune_then_st_encoder_from_the_checkpoint(g, tmp_path, capsys):
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    root = tmp_path / "data"
    root.mkdir()
    U.write_manifest(str(root), g)
    save = str(tmp_path / "ckpt")
    tr = cli.train_main([str(root), "--task", "audio_pretraining", "--labels", "ltr", "--criterion", "ctc", "--arch", "wav2vec_ctc",
                         "--w2v-path", U.W2V, "--zero-infinity", "--apply-mask", "--mask-prob", "0.3", "--mask-length", "4",
                         "--mask-channel-prob", "0.1", "--mask-channel-length", "4", "--feature-grad-mult", "0.1",
                         "--freeze-finetune-updates", "1", "--max-tokens", "9000", "--max-update", "2", "--max-epoch", "2",
                         "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--lr", "1e-4", "--lr-scheduler", "inverse_sqrt",
                         "--warmup-updates", "2", "--save-dir", save, "--seed", "1", "--log-interval", "1", "--num-workers", "1",
                         "--best-checkpoint-metric", "wer"])
    ev = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert ev[0]["event"] == "start" and ev[0]["criterion"] == "ctc" and ev[0]["train_examples"] == 6
    assert tr.num_updates == 2
    valid = [e for e in ev if e["event"] == "valid"]
    assert valid and all(k in valid[-1] for k in ("uer", "wer", "raw_wer", "c_total", "w_total")) and valid[-1]["c_total"] > 0
    path = os.path.join(save, "checkpoint_last.pt")
    assert os.path.exists(path)
    state = torch.load(path, weights_only=False)
    assert all(k.startswith(("w2v_encoder.w2v_model.", "w2v_encoder.proj.")) for k in state["model"])
    # an ST encoder from that checkpoint (--use-asr-finetune-w2v): exactly its wav2vec2 weights; the heads it lacks are inert
    W = import_module("chimera-st_amd.w2v2_transformer")
    args = Namespace(w2v2_model_path=path, use_asr_finetune_w2v=True, encoder_embed_dim=64, encoder_ffn_embed_dim=128, encoder_layers=1,
                     encoder_attention_heads=2, conv_channels=64, dropout=0.0, max_source_positions=100000)
    W.s2t_transformer_w2v2asr_s(args)
    torch.manual_seed(3)
    enc = W.S2T_W2V2_TransformerEncoder(args).cuda().eval()
    got = enc.wav2vec_model.state_dict()
    prefix = "w2v_encoder.w2v_model."
    given = {k[len(prefix):]: v for k, v in state["model"].items() if k.startswith(prefix)}
    assert set(given) < set(got) and all(torch.equal(got[k].cpu(), v) for k, v in given.items())
    assert all(k.startswith(("quantizer.", "project_q.", "final_proj.")) for k in set(got) - set(given))
    # the same encoder given those weights by hand
    hand_args = Namespace(**{**vars(args), "use_asr_finetune_w2v": False})
    W.SYNTHETIC_W2V["ctc_tiny_w2v"] = state["args"].w2v_args
    hand_args.w2v2_model_path = "synthetic:ctc_tiny_w2v"
    hand = W.S2T_W2V2_TransformerEncoder(hand_args).cuda().eval()
    sd = enc.state_dict()
    hand.load_state_dict(sd, strict=True)
    src = torch.from_numpy(g["in/source"]).cuda()
    lens = (~torch.from_numpy(g["in/padding_mask"])).sum(1).cuda()
    with torch.no_grad():
        a, b = enc(src, lens), hand(src, lens)
    assert torch.equal(a.encoder_out, b.encoder_out) and bool(torch.isfinite(a.encoder_out).all())
