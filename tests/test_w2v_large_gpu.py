"""Large-style wav2vec2 checkpoints (extractor_mode=layer_norm, conv_bias, layer_norm_first) on a real MI355X: the two new kernel pairs
against the restatement in w2v_large_ref.py, the models against the fixtures the reference produced (w2v_large_*tiny*), the packed
route against the padded one, the real large layout against the restatement, and training + decoding through the command line.

Tolerances are the suite's own: kernels — the bounds test_kernels_gpu.py uses for conv0_gn_gelu / layernorm (`check`); models — fp32
storage within 1e-3 * max(1, |ref|max) for outputs and gradients and 1e-4 relative for loss terms, bf16 by the emulated-storage rule
stated at the top of test_model_gpu.py (the emulation is the oracle run over the restatement, w2v_large_ref.patched_oracle)."""
import ast
import os
import shutil
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden_cfg, golden_sample, load_golden, load_pkg
from test_kernels_gpu import DT, check, rnd
from test_model_gpu import assert_close, assert_grads_close_bf16, build_from_golden, emulated_tol, to_cuda

import w2v_large_ref as R

pytestmark = pytest.mark.gpu
CKPT = os.path.join(GOLDEN, "w2v_large_tiny.pt")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return import_module("chimera-st_amd.kernels")


def _ln_gelu_ref(u, g, b):
    return F.gelu(F.layer_norm(u, (u.shape[-1],), g, b, 1e-5))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,S,C", [(2, 4000, 32), (3, 16000, 512)])
def test_conv0_ln_gelu(K, dt, B, S, C):
    kk, st = 10, 5
    wav = (0.1 * torch.randn(B, S, generator=torch.Generator().manual_seed(40))).cuda()
    w = rnd(C, kk, dt=dt, seed=41, scale=0.5)
    bias = rnd(C, dt=dt, seed=43, scale=0.1)
    g, b = (1 + 0.1 * torch.randn(C)).to(dt).cuda(), (0.1 * torch.randn(C)).to(dt).cuda()
    wr, bir, gr, br = (t.float().requires_grad_(True) for t in (w, bias, g, b))
    u = F.conv1d(wav[:, None], wr[:, None], bir, stride=st).transpose(1, 2)
    ref = _ln_gelu_ref(u, gr, br)
    y, mean, rstd = K.conv0_ln_fwd(wav, w, bias, g, b, kk, st)
    check(y, ref, dt, "conv0_ln fwd")
    check(mean, u.mean(-1), torch.float32, "conv0_ln mean")
    dy = rnd(B, ref.shape[1], C, dt=dt, seed=42)
    ref.backward(dy.float())
    dw, dbi, dg, db = K.conv0_ln_bwd(dy, wav, w, bias, g, b, mean, rstd, kk, st)
    check(dw, wr.grad, dt, "conv0_ln dW", scale=float(wr.grad.abs().max()))
    check(dbi, bir.grad, dt, "conv0_ln dbias", scale=float(bir.grad.abs().max()))
    check(dg, gr.grad, dt, "conv0_ln dgamma")
    check(db, br.grad, dt, "conv0_ln dbeta")
    # run to run: the same bits
    y2, mean2, rstd2 = K.conv0_ln_fwd(wav, w, bias, g, b, kk, st)
    again = K.conv0_ln_bwd(dy, wav, w, bias, g, b, mean, rstd, kk, st)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    assert all(torch.equal(a, c) for a, c in zip((dw, dbi, dg, db), again))


@pytest.mark.parametrize("dt", DT)
def test_conv0_ln_gelu_frame_limits_are_exact(K, dt):
    """Forward: identical bits below the limit, untouched memory at and above it.  Backward with a dy that is zero from the limit on:
    the bits of the call that reads every frame."""
    kk, st, B, S, C = 10, 5, 3, 16000, 512
    wav = (0.1 * torch.randn(B, S, generator=torch.Generator().manual_seed(40))).cuda()  # ragged: zero behind each utterance's end
    lens = [16000, 9000, 2003]
    for i, n in enumerate(lens):
        wav[i, n:] = 0
    w, bias = rnd(C, kk, dt=dt, seed=41, scale=0.5), rnd(C, dt=dt, seed=43, scale=0.1)
    g, b = (1 + 0.1 * torch.randn(C)).to(dt).cuda(), (0.1 * torch.randn(C)).to(dt).cuda()
    y, mean, rstd = K.conv0_ln_fwd(wav, w, bias, g, b, kk, st)
    Lo = y.shape[1]
    lim = torch.tensor([Lo + 5, 1799, 0], dtype=torch.int32, device="cuda")
    lib = import_module("chimera-st_amd.lib")
    yl = torch.full_like(y, 7.0)
    ml, rl = torch.full_like(mean, -3.0), torch.full_like(rstd, -3.0)
    lib.check(lib.load().cst_conv0_ln_gelu_fwd(lib.ptr(wav), lib.ptr(w), lib.ptr(bias), lib.ptr(g), lib.ptr(b), lib.ptr(yl), lib.ptr(ml),
                                               lib.ptr(rl), lib.ptr(lim), B, S, C, kk, st, 1e-5, lib.dtype_code(dt), lib.stream_ptr()), "fwd")
    for i, n in enumerate([Lo, 1799, 0]):
        assert torch.equal(yl[i, :n], y[i, :n]) and torch.equal(ml[i, :n], mean[i, :n]) and torch.equal(rl[i, :n], rstd[i, :n])
        assert bool((yl[i, n:] == 7.0).all()) and bool((ml[i, n:] == -3.0).all())
    dy = rnd(B, Lo, C, dt=dt, seed=42)
    for i, n in enumerate([Lo, 1799, 0]):
        dy[i, n:] = 0
    full = K.conv0_ln_bwd(dy, wav, w, bias, g, b, mean, rstd, kk, st)
    limited = K.conv0_ln_bwd(dy, wav, w, bias, g, b, ml, rl, kk, st, frame_limit=lim)  # (the limited call's own statistics: poison behind the limit)
    for a, c, n in zip(full, limited, ("dW", "dbias", "dgamma", "dbeta")):
        assert torch.equal(a, c), n


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,L,C", [(3, 50, 64), (4, 700, 512), (2, 33, 1024)])
def test_ln_gelu(K, dt, B, L, C):
    u = rnd(B, L, C, dt=dt, seed=20)
    g, b = (1 + 0.1 * torch.randn(C)).to(dt).cuda(), (0.1 * torch.randn(C)).to(dt).cuda()
    ur, gr, br = (t.float().requires_grad_(True) for t in (u, g, b))
    ref = _ln_gelu_ref(ur, gr, br)
    y, mean, rstd = K.ln_gelu_fwd(u, g, b)
    check(y, ref, dt, "ln_gelu fwd")
    dy = rnd(B, L, C, dt=dt, seed=22)
    ref.backward(dy.float())
    du, dg, db, dc = K.ln_gelu_bwd(dy, u, g, b, mean, rstd, want_colsum=True)
    check(du, ur.grad, dt, "ln_gelu du")
    check(dg, gr.grad, dt, "ln_gelu dgamma")
    check(db, br.grad, dt, "ln_gelu dbeta")
    check(dc, ur.grad.sum((0, 1)), dt, "ln_gelu colsum(du)", scale=float(ur.grad.abs().max()) * (B * L) ** 0.5)
    # row limits: rows below the limit keep their bits, rows from it on are zeros; gradients of a dy that is zero there keep theirs
    lim = torch.tensor([L, L // 3, 0, L - 1][:B], dtype=torch.int32, device="cuda")
    yl, _, _ = K.ln_gelu_fwd(u, g, b, row_limit=lim)
    dyl = dy.clone()
    for i in range(B):
        n = int(lim[i])
        assert torch.equal(yl[i, :n], y[i, :n]) and bool((yl[i, n:] == 0).all())
        dyl[i, n:] = 0
    f = K.ln_gelu_bwd(dyl, u, g, b, mean, rstd, want_colsum=True)
    l = K.ln_gelu_bwd(dyl, u, g, b, mean, rstd, row_limit=lim, want_colsum=True, padded=True)
    assert l[0].stride(0) == (L + 2) * C
    for a, c, n in zip(f, l, ("du", "dgamma", "dbeta", "colsum")):
        assert torch.equal(a, c), n
    again = K.ln_gelu_bwd(dyl, u, g, b, mean, rstd, row_limit=lim, want_colsum=True)
    assert all(torch.equal(a, c) for a, c in zip(l, again))


# ------------------------------------------------------------------------------------------------ models vs the reference's fixtures
def _fixture(arch):
    g = load_golden("w2v_large_%s_tiny.npz" % arch)
    g.update(load_golden("w2v_large_%s_tiny_grads.npz" % arch))
    return g


def _emulated_bf16(g, arch):
    from parity_util import run_oracle
    sd = {k[len("param/"):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("param/")}
    with R.patched_oracle() as O:
        return run_oracle(O.triplet_criterion if arch == "chimera" else O.lsce_criterion, sd, golden_sample(g), golden_cfg(g), storage=torch.bfloat16)


def test_wav2vec2_stage_activations_match_the_reference():
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    CF = import_module("chimera-st_amd.functional")
    g = load_golden("w2v_large_tiny.npz")
    ck = torch.load(CKPT, map_location="cpu", weights_only=False)
    model = W.Wav2Vec2Model.build_model(ck["args"])
    model.load_state_dict(ck["model"], strict=True)
    model = model.cuda().eval()
    wav, lens = torch.from_numpy(g["in/src_tokens"]).cuda(), torch.from_numpy(g["in/src_lengths"]).cuda()
    pm = torch.arange(wav.size(1), device="cuda").view(1, -1) >= lens.view(-1, 1)
    fe = model.feature_extractor
    l0 = fe.conv_layers[0]
    with torch.no_grad():
        c0 = CF.conv0_ln_gelu(wav, getattr(l0, "0").weight, getattr(l0, "0").bias, getattr(getattr(l0, "2"), "1").weight,
                              getattr(getattr(l0, "2"), "1").bias, fe.conv_spec[0][2])
        cnn = fe(wav)
        x, fpm = model.extract_features(wav, pm)
        os.environ["CST_NO_PACK"] = "1"
        try:
            x_padded, _ = model.extract_features(wav, pm)
        finally:
            del os.environ["CST_NO_PACK"]
    assert_close(c0.transpose(1, 2), g["act/conv0"], 1e-3, "conv layer 0")
    assert_close(cnn.transpose(1, 2), g["act/cnn"], 1e-3, "CNN output")
    assert np.array_equal(fpm.cpu().numpy(), g["out/padding_mask"])
    assert_close(x, g["act/out"], 1e-3, "wav2vec2 output (behind the trailing LayerNorm)")
    assert_close(x, g["act/final_ln"], 1e-3, "trailing LayerNorm")
    assert torch.equal(x, x_padded), "packed-row route differs from the padded one"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("arch", ["s2t", "chimera"])
def test_models_match_the_reference_fixtures(arch, dtype):
    g = _fixture(arch)
    model, task, args = build_from_golden(g, arch, dtype)
    assert model.encoder.wav2vec_model.feature_extractor.mode == "layer_norm"
    crit_mod = import_module("chimera-st_amd.criterions")
    sample = to_cuda(golden_sample(g))
    model.train()
    if arch == "chimera":
        crit = crit_mod.TripletSTMTContrastiveCriterion(task, False, 0.1, [1.0, 1.0, 1.0], 0.1)
        outs = ("memory_audio", "st_logits", "memory_text", "mt_logits")
        terms = ("loss", "nll_loss", "st_loss", "st_nll_loss", "mt_loss", "mt_nll_loss", "contrastive_loss")
    else:
        crit = crit_mod.LabelSmoothedCrossEntropyCriterion(task, False, 0.1)
        outs = ("logits",)
        terms = ("loss", "nll_loss")
    if dtype == torch.bfloat16:
        emu, egrads = _emulated_bf16(g, arch)
        tols = {k: emulated_tol(emu[k], g["out/" + k]) for k in outs}
        emu_gap = max(abs(float(emu[k]) - float(g["loss/" + k])) / abs(float(g["loss/" + k])) for k in terms)
    else:
        tols = {k: 1e-3 for k in outs}
    if arch == "chimera":
        (st_logits, _), mem_a = model.forward_with_internal(**sample["net_input"])
        (mt_logits, _), mem_t = model.forward_with_internal(src_tokens=sample["src_text"], src_lengths=sample["src_text_lengths"],
                                                            prev_output_tokens=sample["net_input"]["prev_output_tokens"])
        got = dict(memory_audio=mem_a, st_logits=st_logits, memory_text=mem_t, mt_logits=mt_logits)
    else:
        got = dict(logits=model(**sample["net_input"])[0])
    for k in outs:
        print(k, "tol %.3e" % tols[k])
        assert_close(got[k], g["out/" + k], tols[k], k)
    model.zero_grad()
    loss, sample_size, log = crit(model, sample)
    loss.backward()
    for k in terms:
        ref = float(g["loss/" + k])
        ltol = 1e-4 if dtype == torch.float32 else 3 * emu_gap + 5e-4
        print(k, float(log[k]), ref)
        assert abs(float(log[k]) - ref) <= ltol * abs(ref), "%s: %.6f vs %.6f" % (k, float(log[k]), ref)
    assert sample_size == int(g["loss/sample_size"])
    if dtype == torch.bfloat16:
        assert_grads_close_bf16(model, g, egrads)
        return
    for name, p in model.named_parameters():
        ref = g["grad/" + name]
        if p.grad is None:
            assert not np.abs(ref).any(), name
            continue
        assert_close(p.grad, ref, 1e-3, "grad " + name)


@pytest.mark.parametrize("beam", [1, 5])
def test_decoding_matches_the_reference_generator(beam):
    g = _fixture("chimera")
    model, task, args = build_from_golden(g, "chimera", torch.float32)
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    gen = SG([model.eval()], task.target_dictionary, beam_size=beam, max_len_a=0, max_len_b=12, min_len=1)
    hyps = gen.generate([model], to_cuda(golden_sample(g)))
    for b in range(len(hyps)):
        for r in range(min(beam, 3)):
            key = "gen/beam%d/b%d/r%d/" % (beam, b, r)
            assert hyps[b][r]["tokens"].tolist() == g[key + "tokens"].tolist(), key
            assert abs(float(hyps[b][r]["score"]) - float(g[key + "score"])) < 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("arch", ["s2t", "chimera"])
def test_packed_route_is_bit_identical_to_the_padded_one(arch, dtype):
    """As test_padding_free_wav2vec2_stack_is_bit_identical does for post-norm stacks: same forward bits; gradients to summation rounding."""
    Kn = import_module("chimera-st_amd.kernels")
    g = _fixture(arch)
    model, task, args = build_from_golden(g, arch, dtype)
    tasks = import_module("chimera-st_amd.tasks")
    sample = to_cuda(tasks.synthetic_sample(task.target_dictionary, 4, [9000, 5200, 2600, 1300], [9, 3, 12, 5], [4, 7, 2, 11], seed=7))
    crit_mod = import_module("chimera-st_amd.criterions")
    crit = (crit_mod.TripletSTMTContrastiveCriterion(task, False, 0.1, [1.0, 1.0, 1.0], 0.1) if arch == "chimera"
            else crit_mod.LabelSmoothedCrossEntropyCriterion(task, False, 0.1))
    model.train()

    def run():
        model.zero_grad()
        Kn.STATS.clear()
        enc = model.encoder(sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"])
        loss, _, _ = crit(model, sample)
        loss.backward()
        eo = enc.encoder_out.detach().clone()
        if arch == "s2t":
            eo = eo.masked_fill(enc.encoder_padding_mask.t().unsqueeze(-1), 0)
        return eo, loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, dict(Kn.STATS)

    out_p, loss_p, grads_p, stats_p = run()
    os.environ["CST_NO_PACK"] = "1"
    try:
        out_d, loss_d, grads_d, stats_d = run()
    finally:
        del os.environ["CST_NO_PACK"]
    assert stats_p.get("attn_packed", 0) > 0 and stats_d.get("attn_packed", 0) == 0, (stats_p, stats_d)
    assert torch.equal(out_p, out_d) and torch.equal(loss_p, loss_d)
    tol = 2e-5 if dtype == torch.float32 else 1.2e-2
    for n in grads_p:
        a, b = grads_p[n].float(), grads_d[n].float()
        scale = float(b.abs().max())
        if n.endswith(".bias") and n[:-5] + ".weight" in grads_d:
            scale = max(scale, float(grads_d[n[:-5] + ".weight"].float().abs().max()))
        assert float((a - b).abs().max()) / max(scale, 1e-30) <= tol, n


# ------------------------------------------------------------------------------------------------ the real large layout
def test_full_width_layout_against_the_restatement():
    """7 x 512 layer-norm CNN with biases, 24 x 1024 x 16 heads, FFN 4096, positional conv 1024 channels in 16 groups (k = 128), random
    weights, three utterances of 1.0 / 0.7 / 0.3 s (short audio, full layout: the fp64 and fp32 restatements on the CPU and the GPU run
    take about 5 s together).  fp32 storage: features within 2 x d + 1e-3 and gradients within 2 x d_g + 1e-3 of the fp64 restatement, in
    units of max(1, |ref|max), d / d_g being the distance of the restatement ITSELF run in fp32 from its fp64 run on the same input.
    Measured: features 2.7e-6 (d = 6.8e-7), worst gradient 4.1e-6 (d_g = 2.7e-6)."""
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    torch.manual_seed(5)
    args = W.wav2vec_small_args(
        extractor_mode="layer_norm", conv_bias=True, layer_norm_first=True, encoder_layers=24, encoder_embed_dim=1024,
        encoder_ffn_embed_dim=4096, encoder_attention_heads=16, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
        encoder_layerdrop=0.0, dropout_input=0.0, feature_grad_mult=1.0, final_dim=768, quantize_targets=False)
    model = W.Wav2Vec2Model.build_model(args)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias") or "layer_norm" in n or n.endswith("2.1.weight"):
                p.add_(0.05 * torch.randn_like(p))
    S = [16000, 11200, 4800]
    wav = torch.zeros(3, S[0])
    for i, n in enumerate(S):
        wav[i, :n] = 0.5 * torch.randn(n)
    lens = torch.tensor(S)
    pm = torch.arange(S[0]).view(1, -1) >= lens.view(-1, 1)
    cfg = dict(conv_layers=eval(args.conv_feature_layers), conv_pos=128, conv_pos_groups=16, w2v_layers=24, w2v_heads=16, feature_grad_mult=1.0)
    names = ["feature_extractor.conv_layers.0.0.weight", "feature_extractor.conv_layers.0.0.bias", "feature_extractor.conv_layers.0.2.1.weight",
             "feature_extractor.conv_layers.3.0.weight", "feature_extractor.conv_layers.6.0.bias", "feature_extractor.conv_layers.6.2.1.bias",
             "post_extract_proj.weight", "encoder.pos_conv.0.weight_v", "encoder.layers.0.self_attn.q_proj.weight",
             "encoder.layers.23.fc2.weight", "encoder.layer_norm.weight"]
    torch.manual_seed(6)
    cot = torch.randn(3, 49, 1024)

    def restated(dt):
        p = {k: v.detach().to(dt).requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
        x, fpm, _ = R.extract_features(p, "", wav.to(dt), pm, cfg)
        x = x.masked_fill(fpm.unsqueeze(-1), 0.0)
        (x * cot.to(dt)).sum().backward()
        return x.detach(), {n: p[n].grad for n in names}, fpm

    x64, g64, fpm = restated(torch.float64)
    x32, g32, _ = restated(torch.float32)
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / max(1.0, float(b.abs().max()))
    d_out = rel(x32, x64)
    d_g = max(rel(g32[n], g64[n]) for n in names)
    model = model.cuda().train()
    x, fpm_gpu = model.extract_features(wav.cuda(), pm.cuda())
    assert torch.equal(fpm_gpu.cpu(), fpm)
    x = x.masked_fill(fpm_gpu.unsqueeze(-1), 0.0)
    (x * cot.cuda()).sum().backward()
    e_out = rel(x.detach().cpu(), x64)
    grads = dict(model.named_parameters())
    e_g = {n: rel(grads[n].grad.cpu(), g64[n]) for n in names}
    print("full width: features err %.3e (fp32 restatement %.3e); gradients worst err %.3e (fp32 restatement %.3e)" % (e_out, d_out, max(e_g.values()), d_g))
    assert torch.isfinite(x).all()
    assert e_out <= 2 * d_out + 1e-3
    for n in names:
        assert e_g[n] <= 2 * d_g + 1e-3, (n, e_g[n], d_g)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("arch", ["s2t_transformer_w2v2", "s2t_transformer_w2v2_interlingua_base"])
def test_train_and_generate_through_the_command_line(arch, tmp_path, capsys):
    import json
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    DATA = os.path.join(GOLDEN, "data_tiny")
    root = tmp_path / "data"
    root.mkdir()
    for f in os.listdir(DATA):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(DATA, f), root / f)
    (root / "config_wave.yaml").write_text((root / "config_wave.yaml").read_text().replace("AUDIO_ROOT", DATA))
    save = str(tmp_path / "ckpt")
    chimera = arch.endswith("interlingua_base")
    flags = [str(root), "--task", "triplet", "--train-subset", "train_st", "--valid-subset", "dev_st", "--config-yaml", "config_wave.yaml",
             "--max-tokens", "12000", "--max-source-positions", "2000000", "--save-dir", save, "--normalize",
             "--criterion", "triplet_st_mt_contrastive" if chimera else "label_smoothed_cross_entropy", "--label-smoothing", "0.1",
             "--arch", arch, "--share-decoder-input-output-embed", "--w2v2-model-path", CKPT, "--encoder-layers", "2",
             "--encoder-embed-dim", "64", "--encoder-ffn-embed-dim", "128", "--encoder-attention-heads", "2", "--decoder-attention-heads", "2",
             "--decoder-layers", "2", "--conv-channels", "64", "--dropout", "0.1", "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)",
             "--clip-norm", "0.0", "--lr", "2e-3", "--lr-scheduler", "inverse_sqrt", "--weight-decay", "0.0001", "--warmup-updates", "2",
             "--fp16", "--update-freq", "1", "--num-workers", "1", "--ddp-backend", "no_c10d", "--seed", "1", "--log-interval", "1",
             "--max-update", "2"]
    if chimera:
        flags += ["--interlingua-length", "8", "--interlingua-layers", "2", "--best-checkpoint-metric", "st_loss"]
    tr = cli.train_main(flags)
    ev = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    losses = [e["loss"] for e in ev if e.get("event") in ("train", "train_inner") and "loss" in e]
    assert tr.num_updates == 2 and losses and all(np.isfinite(l) for l in losses), ev
    last = os.path.join(save, "checkpoint_last.pt")
    state = torch.load(last, weights_only=False)
    assert any(k.startswith("encoder.wav2vec_model.feature_extractor.conv_layers.3.2.1.") for k in state["model"])
    summary = cli.generate_main([str(root), "--task", "triplet", "--config-yaml", "config_wave.yaml", "--path", last, "--gen-subset", "dev_st",
                                 "--max-tokens", "12000", "--beam", "3", "--max-len-b", "10", "--max-source-positions", "2000000", "--fp16",
                                 "--normalize"])
    assert summary["sentences"] == 4
