"""wav2vec2 pre-training end to end on a real MI355X: Wav2Vec2Model.forward(features_only=False) under criterion `wav2vec` against
tests/golden/w2v_pretrain_tiny.npz — the REAL reference's numbers (tools/ref_harness/make_w2v_pretrain_goldens.py) with its masks, negative
indices and Gumbel noise replayed: logits, loss terms, logging output and every gradient within the project's 1e-3 in fp32 storage; eval
mode; cross-sample negatives; the temperature; the checkpoint layout; and the command line: two updates of pre-training on a generated
manifest, bit-equal from run to run, whose checkpoint then feeds a CTC update through --w2v-path."""
import argparse
import json
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import wav2vec_ctc_util as U
from conftest import load_golden, load_pkg
from parity_util import max_abs_rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return load_golden("w2v_pretrain_tiny.npz")


def checkpoint():
    torch.serialization.add_safe_globals([argparse.Namespace])
    return torch.load(U.W2V, map_location="cpu")


def build(g, cross=0, dtype=torch.float32):
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    ck = checkpoint()
    args = ck["args"]
    args.mask_prob, args.mask_length = float(g["meta/mask_prob"]), int(g["meta/mask_length"])
    args.num_negatives, args.cross_sample_negatives, args.criterion = int(g["meta/num_negatives"]), cross, "wav2vec"
    model = W.Wav2Vec2Model.build_model(args)
    model.load_state_dict(ck["model"], strict=True)
    return model.to("cuda", dtype)


def criterion():
    C = import_module("chimera-st_amd.criterions")
    return C.Wav2vecCriterion(SimpleNamespace(), True, "[0.1, 10]", '["prob_perplexity","code_perplexity","temp"]')


def sample_of(g, case):
    ni = {"source": torch.from_numpy(g["in/source"]).cuda(), "padding_mask": None, "mask_indices": g[case + "/mask"],
          "neg_idxs": torch.from_numpy(g[case + "/neg_idx"])}
    if case + "/noise" in g:
        ni["noise"] = torch.from_numpy(g[case + "/noise"]).cuda()
    return {"id": torch.arange(3), "net_input": ni}


def check_case(g, case, model, train):
    model.train(train)
    model.zero_grad()
    crit = criterion()
    sample = sample_of(g, case)
    loss, sample_size, log = crit(model, sample)
    B, M, K1 = g[case + "/logits"].shape
    assert sample_size == int(g[case + "/sample_size"]) == B * M
    with torch.no_grad():
        logits = model.get_logits(model(**sample["net_input"])).cpu().view(B, M, K1)
    ref = torch.from_numpy(g[case + "/logits"])
    inf = torch.isinf(ref)
    assert bool(inf.any()) and torch.equal(torch.isinf(logits), inf), "the -inf logits (a negative with its positive's codes) differ"
    e = max_abs_rel(logits[~inf], ref[~inf])
    host = {k: float(v) for k, v in log.items()}  # (the test's read; the trainer makes one for all of them)
    errs = {k: abs(host[k] - float(g[case + "/" + k])) / max(abs(float(g[case + "/" + k])), 1e-6)
            for k in ("loss", "loss_0", "loss_1", "loss_2", "prob_perplexity", "code_perplexity", "temp")}
    print("PARITY w2v_pretrain %-5s logits %.2e  %s" % (case, e, "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert e < 1e-3 and all(v < 1e-3 for v in errs.values()), errs
    assert (int(host["correct"]), int(host["count"])) == (int(g[case + "/correct"]), int(g[case + "/count"]))
    assert set(log) == set(crit.logging_keys()) and crit.single_pass and not crit.logging_outputs_can_be_summed()
    return loss


def test_train_parity_with_the_reference(g):
    model = build(g)
    loss = check_case(g, "train", model, True)
    loss.backward()
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        got = p.grad.float().cpu() if p.grad is not None else torch.zeros(p.shape)
        err = max_abs_rel(got, torch.from_numpy(g["grad/" + k]))
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert err < 1e-3, (k, err)
    print("PARITY w2v_pretrain worst gradient %s %.2e" % worst)
    for k in ("mask_emb", "final_proj.weight", "project_q.weight", "quantizer.vars", "quantizer.weight_proj.weight"):
        assert float(np.abs(g["grad/" + k]).max()) > 0 and dict(model.named_parameters())[k].grad is not None, k


def test_eval_and_cross_sample_parity_with_the_reference(g):
    with torch.no_grad():
        check_case(g, "eval", build(g), False)
    check_case(g, "cross", build(g, cross=int(g["meta/cross_sample_negatives"])), True)


def replay(g, case, **extra):
    return dict(source=torch.from_numpy(g["in/source"]), mask=g[case + "/mask"], neg_idx=g[case + "/neg_idx"], noise=g.get(case + "/noise"),
                training=case != "eval", **extra)


@pytest.mark.parametrize("case", ["train", "eval"])
def test_bf16_parity_within_the_storage_rounding_bound(g, case):
    """The model in bf16 storage against the yardstick of test_wav2vec_ctc_gpu.py: the oracle-trunk composition
    (w2v_pretrain_util.pretrain_oracle, pinned to the real reference's fixture on the CPU) is re-run through parity_util.run_oracle with
    every stored tensor rounded to bf16, and its distance to the fp32 evaluation is the measure — logits, the loss terms loss_0..2 and
    prob_perplexity within 2x + 1e-3 (in units of max(1, |ref|)), the loss within 3x + 5e-4 relative, all gradients together within 1.5x their relative L2 error + 1e-3, every tensor with >= 1 % of the norm
    within 2x its own + 1e-2.
    The quantizer's hard choices are discrete: the fixture's closest top-2 margin is 2e-3 on logits of magnitude 20, where one bf16
    ulp is 0.125, so a bf16 run may decide a near-tie the other way.  The model's own choices are therefore replayed in BOTH oracle
    runs (the fp32 one is the reference then), and a choice may differ from the fp32 argmax only where that argmax's margin is within
    2x + 1e-3 of what storage rounding does to that row's decision values in the emulation."""
    import w2v_pretrain_util as PU
    from parity_util import grad_errors, run_oracle
    train = case == "train"
    model = build(g, dtype=torch.bfloat16).train(train)
    crit, sample = criterion(), sample_of(g, case)
    with torch.enable_grad() if train else torch.no_grad():
        net = model(**sample["net_input"])
        loss, sample_size, log = crit(model, sample)
    if train:
        loss.backward()
    assert net["x"].dtype == torch.bfloat16 and net["y"].dtype == torch.bfloat16
    B, M, K1 = g[case + "/logits"].shape
    choices = net["quantizer_targets"].reshape(B * M, -1).cpu()
    with torch.no_grad():
        logits = model.get_logits(net).cpu().view(B, M, K1)
    sd, a = PU.params(False)
    free, _ = run_oracle(PU.pretrain_oracle_fn, sd, replay(g, case), a)
    free16, _ = run_oracle(PU.pretrain_oracle_fn, sd, replay(g, case), a, storage=torch.bfloat16)
    ref, rgrads = run_oracle(PU.pretrain_oracle_fn, sd, replay(g, case, choices=choices), a)
    emu, egrads = run_oracle(PU.pretrain_oracle_fn, sd, replay(g, case, choices=choices), a, storage=torch.bfloat16)
    # choices: different from the fp32 argmax only at near-ties
    flipped = (choices != free["choices"]).nonzero().tolist()
    top2 = free["vq_scores"].topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    moved = (free16["vq_scores"] - free["vq_scores"]).abs().amax(-1)
    for n, grp in flipped:
        assert float(margin[n, grp]) <= 2 * 2 * float(moved[n, grp]) + 1e-3, (n, grp, float(margin[n, grp]), float(moved[n, grp]))
    assert len(flipped) <= 0.1 * choices.numel()
    # outputs
    inf = torch.isinf(ref["logits"])
    assert torch.equal(torch.isinf(logits), inf) and torch.equal(torch.isinf(emu["logits"]), inf)
    tol = 2 * max_abs_rel(emu["logits"].detach()[~inf], ref["logits"].detach()[~inf]) + 1e-3
    e = max_abs_rel(logits[~inf], ref["logits"].detach()[~inf])
    host = {k: float(v) for k, v in log.items()}
    worst = {}
    for k in ("loss", "loss_0", "loss_1", "loss_2", "prob_perplexity"):
        r = float(ref[k].detach())
        scale = max(1.0, abs(r))
        if k == "loss":  # the criterion's loss: 3x + 5e-4 relative, as test_wav2vec_ctc_gpu.py holds its loss
            worst[k] = (abs(host[k] - r) / abs(r), 3 * abs(float(emu[k].detach()) - r) / abs(r) + 5e-4)
        else:            # its terms and the perplexity: the output measure, 2x + 1e-3 of max(1, |ref|), as that test holds its nll terms
            worst[k] = (abs(host[k] - r) / scale, 2 * abs(float(emu[k].detach()) - r) / scale + 1e-3)
    print("PARITY w2v_pretrain bf16 %-5s flipped choices %d of %d  logits %.2e (tol %.2e)  %s" % (
        case, len(flipped), choices.numel(), e, tol, "  ".join("%s %.2e (tol %.2e)" % ((k,) + v) for k, v in worst.items())))
    assert e <= tol and all(v[0] <= v[1] for v in worst.values()), worst
    assert sample_size == B * M and int(host["count"]) == B * M
    if not train:
        return
    g_emu, per_emu = grad_errors(egrads, rgrads)
    g_hip, per_hip = grad_errors({n: p.grad for n, p in model.named_parameters()}, rgrads)
    print("PARITY w2v_pretrain bf16 gradient rel-L2: hip %.3e, storage rounding alone %.3e" % (g_hip, g_emu))
    assert set(rgrads) == {n for n, _ in model.named_parameters()}
    assert g_hip <= 1.5 * g_emu + 1e-3
    for name, (err, share) in per_hip.items():
        if share >= 1e-2:
            assert err <= 2 * per_emu[name][0] + 1e-2, (name, err, per_emu[name][0])


def test_eval_mode_backward_through_the_quantizer_module(g):
    """In eval the hard choice is the raw logits' argmax: q passes the dense gradient to vars (the reference's hard_x * vars) and
    nothing to the logits; a gradient of prob_perplexity there is refused by name."""
    model = build(g).eval()
    qz = model.quantizer
    x = torch.randn(3, 7, qz.input_dim, device="cuda", requires_grad=True)
    res = qz(x, produce_targets=True)
    dq = torch.randn_like(res["x"])
    (res["x"] * dq).sum().backward()
    G, V = qz.groups, qz.num_vars
    d = qz.vars.shape[-1]
    want = torch.zeros(G * V, d, dtype=torch.float64)
    rows = (res["targets"].reshape(-1, G).cpu() + torch.arange(G)[None, :] * V).reshape(-1)
    want.index_add_(0, rows, dq.reshape(-1, d).double().cpu())
    assert float((qz.vars.grad[0].double().cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert float(x.grad.abs().max()) == 0.0 and float(qz.weight_proj.weight.grad.abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match="prob_perplexity in eval"):
        qz(x)["prob_perplexity"].backward()


def test_own_draws_are_seeded_and_the_temperature_follows_the_updates(g):
    """Without replayed draws: masks from numpy's generator, negatives and noise from the counter hash — one seed, one result."""
    model = build(g).train()
    rng = import_module("chimera-st_amd.rng")
    src = {"source": torch.from_numpy(g["in/source"]).cuda()}
    outs = []
    for _ in range(2):
        np.random.seed(4)
        rng.reseed(4)
        loss, _, log = criterion()(model, {"id": torch.arange(3), "net_input": src})
        outs.append((loss.detach().clone(), log["correct"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and bool(torch.isfinite(outs[0][0]))
    model.set_num_updates(200000)
    assert model.quantizer.curr_temp == max(2.0 * 0.999995 ** 200000, 0.5)
    net = model(**src)
    assert net["temp"] == model.quantizer.curr_temp and net["x"].shape == net["y"].shape and net["neg_idx"].shape[1] == int(g["meta/num_negatives"])


def test_state_dict_layout_is_the_reference_files(g):
    model = build(g)
    ck = checkpoint()
    assert list(model.state_dict().keys()) == list(ck["model"].keys()) == str(g["meta/keys"]).split("\n")
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), ck["model"][k]), k


def pretrain(cli, root, save):
    return cli.train_main([str(root), "--task", "audio_pretraining", "--criterion", "wav2vec", "--arch", "wav2vec2", "--infonce",
                           "--loss-weights", "[0.1, 10]", "--log-keys", '["prob_perplexity","code_perplexity","temp"]', "--quantize-targets",
                           "--final-dim", "16", "--latent-vars", "8", "--latent-groups", "2", "--latent-temp", "(2,0.5,0.999995)",
                           "--mask-prob", "0.3", "--mask-length", "3", "--num-negatives", "5", "--feature-grad-mult", "0.1",
                           "--encoder-layerdrop", "0.05", "--dropout-input", "0.1", "--dropout-features", "0.1",
                           "--conv-feature-layers", "[(32, 10, 5)] + [(32, 3, 2)] * 2 + [(32, 2, 2)]", "--encoder-layers", "2",
                           "--encoder-embed-dim", "64", "--encoder-ffn-embed-dim", "128", "--encoder-attention-heads", "2", "--conv-pos", "16",
                           "--conv-pos-groups", "4", "--max-sample-size", "4000", "--min-sample-size", "2000", "--max-tokens", "9000",
                           "--max-update", "2", "--max-epoch", "2", "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--lr", "1e-4",
                           "--lr-scheduler", "inverse_sqrt", "--warmup-updates", "2", "--save-dir", save, "--seed", "1", "--log-interval", "1",
                           "--num-workers", "1", "--disable-validation"])


def test_cli_pretrain_twice_bit_equal_then_ctc_from_the_checkpoint(tmp_path, capsys):
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    gc = U.fixture()
    root = tmp_path / "data"
    root.mkdir()
    U.write_manifest(str(root), gc)
    states = []
    for run in ("a", "b"):
        tr = pretrain(cli, root, str(tmp_path / run))
        assert tr.num_updates == 2
        states.append(torch.load(os.path.join(str(tmp_path / run), "checkpoint_last.pt"), weights_only=False)["model"])
    ev = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert ev[0]["event"] == "start" and ev[0]["criterion"] == "wav2vec" and ev[0]["train_examples"] == 6
    steps = [e for e in ev if e["event"] == "train_inner"]
    assert len(steps) == 4 and all(np.isfinite(e["loss"]) and e["ntokens"] > 0 for e in steps)
    assert steps[:2] == steps[2:], "the two runs' logs differ"
    assert list(states[0]) == list(states[1]) and all(torch.equal(states[0][k], states[1][k]) for k in states[0]), "two runs differ"
    assert "quantizer.vars" in states[0] and "final_proj.weight" in states[0]
    path = os.path.join(str(tmp_path / "a"), "checkpoint_last.pt")
    tr = cli.train_main([str(root), "--task", "audio_pretraining", "--labels", "ltr", "--criterion", "ctc", "--arch", "wav2vec_ctc",
                         "--w2v-path", path, "--zero-infinity", "--freeze-finetune-updates", "5", "--max-tokens", "9000", "--max-update", "1",
                         "--max-epoch", "1",
                         "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--lr", "1e-4", "--lr-scheduler", "inverse_sqrt",
                         "--warmup-updates", "2", "--save-dir", str(tmp_path / "ctc"), "--seed", "1", "--log-interval", "1", "--num-workers", "1",
                         "--disable-validation"])
    assert tr.num_updates == 1
    w = tr.get_model().w2v_encoder.w2v_model
    assert w.quantizer is None and w.final_proj is None  # the CTC model drops the pre-training heads
    # the trunk is frozen during this update (--freeze-finetune-updates): every tensor of it is still the pre-trained checkpoint's
    trunk = w.state_dict()
    assert len(trunk) > 20 and set(trunk) <= set(states[0])
    for k, v in trunk.items():
        assert torch.equal(v.cpu(), states[0][k].cpu().to(v.dtype)), k
