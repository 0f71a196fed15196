#!/usr/bin/env python3
"""tests/golden/interactive_tiny.npz — typed input (fairseq-interactive) as the REAL reference handles it, imported through ref_import.py:
audio paths, sentences and language-model prompts -> tokens and lengths -> the inference dataset's batches -> hypotheses -> printed lines.

Build container only (CPU):   python tools/ref_harness/make_interactive_goldens.py
Holds data only — inputs, batches and recorded results, never reference source, and no parameters another fixture already holds.

  lm/   the LM of decode_lm_tiny.npz on prompts (words of its dictionary) through the reference's LanguageModelingTask:
        build_dataset_for_inference -> get_batch_iterator -> inference_step -> SequenceGenerator.  Buffers "ragged" (prompts of 1, 2
        and 4 tokens, one batch) and "one" (a single prompt of 3).  Settings (meta/lm_settings): beam5, beam1, lenpen_ngram (beam 5,
        len_penalty 1.5, no_repeat_ngram_size 2) and boundary (beam 5, max_len_b 4: the longest prompt is exactly max_len long).
        lm/prompts/<buffer>, lm/<buffer>/tokens/<i>, lm/<buffer>/lengths, lm/<buffer>/batch<j>/{id, src_tokens, src_lengths, target},
        lm/<setting>/<buffer>/batch<j>/b<i>/n and .../r<k>/{tokens, score, pos_scores};  lm/unprompted/r0/tokens (beam5, no prompt)
  st/   ref_checkpoint_tiny.pt on data_tiny/talk_a.wav and talk_b.wav (st/lines: a, b, a) through the reference's TripletTask and its
        fairseq_cli.interactive.buffered_read / make_batches at buffer sizes 1 and 3, --max-tokens st/max_tokens (cuts the buffer of 3
        into two batches), beam 5.  st/buf<N>/buffer<k>/batch<j>/{id, src_tokens, src_lengths}, hypotheses as above, st/buf<N>/stdout (the lines)
  mt/   the chimera_tiny.npz model (the one translation_tiny.npz carries) fed the lines of translation_tiny/corpus/test.en.txt through
        the reference's TranslationTask: "plain" (buffer 3, --max-tokens 20), "plain_buf1" (the same lines one by one: this model's
        output for a sentence depends on the padding beside it) and "constrained" (--constraints, one line with phrases after tabs).
        mt/<case>/{lines, buffer_size}, batches, hypotheses, mt/<case>/stdout
meta/printed_by says where the lines come from: the reference's main() needs hydra/omegaconf configuration objects the stubs do not
provide, so the lines are printed by a restatement in this harness over the reference's own Dictionary.string /
utils.post_process_prediction and its format strings' semantics (`{}` of the fp32 score tensor / ln 2, `{:.4f}` positional scores).

Before anything is written the script asserts that the fixture cannot hide a failure:
  * at every step the last kept and the first dropped candidate of the top-2*beam are more than 1e-4 apart and finalized scores within a
    sentence differ by more than 1e-3 (LM settings; recomputed with a plain-torch search that reproduces the reference's hypotheses);
  * in the ragged LM batch one sentence generates freely while another is still forced (prompt lengths 1 and 4);
  * the prompted hypotheses differ from unprompted decoding;
  * at least one continuation differs between beam 1 and beam 5;
  * in at least one buffer (st and mt) the iterator's batch order differs from input order.
If a seed fails a condition, change the seed (the prompts), not the condition."""
import ast
import contextlib
import io
import math
import os
import sys
import tempfile
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402
from decode_constraints_util import banned_tokens  # noqa: E402

GOLDEN = os.path.abspath(MG.OUT)
LM_SETTINGS = {
    "beam5": dict(beam_size=5, max_len_b=12),
    "beam1": dict(beam_size=1, max_len_b=12),
    "lenpen_ngram": dict(beam_size=5, max_len_b=12, len_penalty=1.5, no_repeat_ngram_size=2),
    "boundary": dict(beam_size=5, max_len_b=4),
}
LM_SEED = 1  # the prompts' seed; found by trying 0, 1, .. in turn against the conditions (python make_interactive_goldens.py --search)


def lm_buffers(seed):
    """Prompts over the words of the tiny dictionary: a buffer of three (1, 2 and 4 tokens) and a buffer of one (3 tokens)."""
    r = np.random.RandomState(1000 + seed)
    line = lambda n: " ".join("w%d" % i for i in r.randint(0, MG.VOCAB - 4, size=n))
    return {"ragged": [line(1), line(2), line(4)], "one": [line(3)]}


ST_LINES = ["talk_a.wav", "talk_b.wav", "talk_a.wav"]
ST_BEAM, ST_MAX_LEN_B = 5, 12
MT_BEAM, MT_MAX_LEN_A, MT_MAX_LEN_B = 5, 1.2, 10
MT_MAX_TOKENS = 20


def put_hyps(out, key, hyps):
    for b, h in enumerate(hyps):
        out["%s/b%d/n" % (key, b)] = np.int64(len(h))
        for r, hyp in enumerate(h):
            k = "%s/b%d/r%d/" % (key, b, r)
            out[k + "tokens"] = hyp["tokens"].numpy().astype(np.int64)
            out[k + "score"] = np.float32(float(hyp["score"]))
            out[k + "pos_scores"] = hyp["positional_scores"].numpy().astype(np.float32)


def prompt_search(lp_fn, prompt, width, beam, max_len, len_penalty=1.0, ngram=0, pad=1, eos=2, unk=3):
    """The reference's beam search of ONE sentence with a forced prompt (lm_fusion_util.search plus _prefix_tokens): width = the batch's
    prefix width (the min_len mask applies only past it).  -> (hypotheses best first, the smallest top-2*beam boundary gap)."""
    V = None
    tokens = torch.full((beam, max_len + 2), pad, dtype=torch.long)
    tokens[:, 0] = eos
    scores = torch.zeros(beam, max_len + 1)
    fin, min_gap = [], math.inf
    for step in range(max_len + 1):
        lp = lp_fn(tokens[:, :step + 1]).clone()
        V = lp.size(-1)
        lp[lp != lp] = -math.inf
        lp[:, pad] = -math.inf
        if step >= max_len:
            lp[:, :eos] = -math.inf
            lp[:, eos + 1:] = -math.inf
        if step < width and step < max_len:
            if step < len(prompt):
                keep = lp[:, prompt[step]].clone()
                lp[:] = -math.inf
                lp[:, prompt[step]] = keep
        elif step < 1:
            lp[:, eos] = -math.inf
        if ngram:
            for h, tk in enumerate(tokens.tolist()):
                ban = sorted(set(banned_tokens(tk, step, ngram)))
                if ban:
                    lp[h, torch.tensor(ban)] = -math.inf
        cand = lp[0:1] if step == 0 else lp + scores[:, step - 1].unsqueeze(-1)
        K = min(2 * beam, cand.numel() - 1)
        top_s, top_i = torch.topk(cand.reshape(-1), k=K + 1)
        if top_s[K] != -math.inf:
            min_gap = min(min_gap, float(top_s[K - 1] - top_s[K]))
        top_s, top_i = top_s[:K], top_i[:K]
        beams, idx = top_i // V, top_i.fmod(V)
        eos_mask = idx.eq(eos) & top_s.ne(-math.inf)
        for j in range(beam):
            if eos_mask[j] and len(fin) < beam:
                bi = int(beams[j])
                fin.append(dict(tokens=torch.cat([tokens[bi, 1:step + 1], torch.tensor([eos])]), score=float(top_s[j]) / ((step + 1) ** len_penalty)))
        if len(fin) >= beam or step >= max_len:
            break
        keep = [j for j in range(K) if not eos_mask[j]][:beam]
        kb = beams[keep]
        new_tokens, new_scores = tokens[kb].clone(), scores[kb].clone()
        new_tokens[:, step + 1] = idx[keep]
        new_scores[:, step] = top_s[keep]
        tokens, scores = new_tokens, new_scores
    fin.sort(key=lambda h: -h["score"])
    return fin, min_gap


def record_lm(out, seed=LM_SEED):
    LM_BUFFERS = lm_buffers(seed)
    out["meta/lm_seed"] = np.int64(seed)
    from fairseq.models.transformer_lm import TransformerLanguageModel
    from fairseq.sequence_generator import SequenceGenerator
    from fairseq.tasks.language_modeling import LanguageModelingTask

    g = np.load(os.path.join(GOLDEN, "decode_lm_tiny.npz"), allow_pickle=False)
    lm_args = ast.literal_eval(str(g["meta/lm_args"]))
    d = MG.make_dictionary()
    targs = Namespace(data=None, sample_break_mode="eos", tokens_per_sample=1024, output_dictionary_size=-1, self_target=False,
                      future_target=False, past_target=False, add_bos_token=False, max_target_positions=1024, shorten_method="none",
                      shorten_data_split_list="", seed=1, dataset_impl=None)
    task = LanguageModelingTask(targs, d, d, targets=["future"])
    lm = TransformerLanguageModel.build_model(Namespace(**lm_args), task)
    sd = {k[len("lm/param/"):]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("lm/param/")}
    # (the fixture stores no `decoder.version`; without it the reference's upgrade_state_dict takes the file for an old checkpoint and
    # DROPS the decoder's final LayerNorm, transformer.py:896-901)
    sd["decoder.version"] = lm.state_dict()["decoder.version"].clone()
    missing, unexpected = lm.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in n for n in missing), (missing, unexpected)
    lm.eval()
    assert lm.decoder.layer_norm is not None
    from lm_fusion_util import lm_forward
    probe = torch.tensor([[d.eos(), 33, 9, 8]])
    with torch.no_grad():  # the loaded model must BE the fixture's LM: the plain-torch forward of tests/lm_fusion_util.py agrees
        assert float((lm(probe)[0] - lm_forward(sd, probe, lm_args["decoder_attention_heads"], lm_args["decoder_layers"])).abs().max()) < 1e-4
    out["meta/lm_settings"] = np.array(repr(LM_SETTINGS))
    from fairseq import utils
    max_positions = utils.resolve_max_positions(task.max_positions(), lm.max_positions())

    def lp_fn(tokens):
        with torch.no_grad():
            return torch.log_softmax(lm(tokens)[0][:, -1, :].float(), -1)

    best = {}
    for buf, lines in LM_BUFFERS.items():
        out["lm/prompts/" + buf] = np.array(lines)
        tokens, lengths = task.get_interactive_tokens_and_lengths(lines, lambda x: x)
        for i, t in enumerate(tokens):
            out["lm/%s/tokens/%d" % (buf, i)] = t.numpy().astype(np.int64)
        out["lm/%s/lengths" % buf] = np.asarray(lengths, dtype=np.int64)
        for name, kw in LM_SETTINGS.items():
            kw = dict(kw)
            gen = SequenceGenerator([lm], d, max_len_a=0, min_len=1, **kw)
            itr = task.get_batch_iterator(dataset=task.build_dataset_for_inference(tokens, lengths), max_tokens=None, max_sentences=len(lines),
                                          max_positions=max_positions, ignore_invalid_inputs=False).next_epoch_itr(shuffle=False)
            batches = list(itr)
            out["lm/%s/nbatches" % buf] = np.int64(len(batches))
            for j, batch in enumerate(batches):
                key = "lm/%s/batch%d/" % (buf, j)
                out[key + "id"] = batch["id"].numpy()
                out[key + "src_tokens"] = batch["net_input"]["src_tokens"].numpy()
                out[key + "src_lengths"] = batch["net_input"]["src_lengths"].numpy()
                out[key + "target"] = batch["target"].numpy()
                sample = {"net_input": {"src_tokens": batch["net_input"]["src_tokens"], "src_lengths": batch["net_input"]["src_lengths"]}}
                hyps = task.inference_step(gen, [lm], sample)
                put_hyps(out, "lm/%s/%s/batch%d" % (name, buf, j), hyps)
                width = batch["net_input"]["src_tokens"].size(1) - 1
                max_len = min(kw["max_len_b"], lm.max_decoder_positions() - 1)
                for b, h in enumerate(hyps):
                    prompt = [int(t) for t in batch["net_input"]["src_tokens"][b, 1:].tolist() if t != d.pad()]
                    mine, gap = prompt_search(lp_fn, prompt, width, kw["beam_size"], max_len, kw.get("len_penalty", 1.0), kw.get("no_repeat_ngram_size", 0))
                    assert gap > 1e-4, ("top-2*beam boundary gap", name, buf, b, gap)
                    sc = sorted(float(x["score"]) for x in h)
                    assert all(y - x > 1e-3 for x, y in zip(sc, sc[1:])), ("finalized scores too close", name, buf, b, sc)
                    assert len(mine) == len(h), (name, buf, b, len(mine), len(h))
                    for r, hyp in enumerate(h):
                        assert mine[r]["tokens"].tolist() == hyp["tokens"].tolist(), (name, buf, b, r, mine[r]["tokens"], hyp["tokens"])
                        assert abs(mine[r]["score"] - float(hyp["score"])) < 1e-4
                        assert hyp["tokens"].tolist()[:len(prompt)] == prompt, "the prompt is not the hypothesis' beginning"
                    if name == "boundary" and len(prompt) == max_len:
                        assert all(len(hyp["tokens"]) == max_len + 1 for hyp in h)
                        best["boundary"] = True
                    best[(name, buf, int(batch["id"][b]))] = (h[0]["tokens"].tolist(), len(prompt))
                    print("lm", name, buf, int(batch["id"][b]), "n", len(h), "best", h[0]["tokens"].tolist(), "%.4f" % float(h[0]["score"]), "gap %.2e" % gap)
    assert best.get("boundary"), "no prompt is exactly max_len long in the boundary setting"
    lens = sorted(len(l.split()) for l in LM_BUFFERS["ragged"])
    assert lens == [1, 2, 4] and int(out["lm/ragged/nbatches"]) == 1, "the ragged buffer must be ONE batch with prompts of 1, 2 and 4 tokens"
    # unprompted decoding (an empty prompt: eos alone; no prefix)
    gen = SequenceGenerator([lm], d, max_len_a=0, min_len=1, **LM_SETTINGS["beam5"])
    free = gen.generate([lm], {"net_input": {"src_tokens": torch.full((1, 1), d.eos()), "src_lengths": torch.ones(1, dtype=torch.long)}})
    put_hyps(out, "lm/unprompted", free)
    free_best = free[0][0]["tokens"].tolist()
    for buf, lines in LM_BUFFERS.items():
        for i in range(len(lines)):
            toks, n = best[("beam5", buf, i)]
            assert toks != free_best and toks[n:] != free_best, "a prompted hypothesis equals unprompted decoding"
    assert any(best[("beam1", buf, i)][0] != best[("beam5", buf, i)][0] for buf, lines in LM_BUFFERS.items() for i in range(len(lines))), \
        "beam 1 and beam 5 continue every prompt alike"


def print_lines(results, src_dict, tgt_dict, nbest, strip, post_process=None):
    """The lines of one buffer as fairseq_cli/interactive.py prints them (a restatement: see the module docstring)."""
    from fairseq import utils
    lines = []
    for id_, src_tokens, hypos, info in sorted(results, key=lambda x: x[0]):
        src_str = ""
        if src_dict is not None and src_tokens.dtype is not torch.float:
            src_str = src_dict.string(src_tokens, post_process)
            lines.append("S-{}\t{}".format(id_, src_str))
            lines.append("W-{}\t{:.3f}\tseconds".format(id_, info["time"]))
            for constraint in info["constraints"]:
                lines.append("C-{}\t{}".format(id_, tgt_dict.string(constraint, post_process)))
        for hypo in hypos[:min(len(hypos), nbest)]:
            _, hypo_str, _ = utils.post_process_prediction(hypo_tokens=hypo["tokens"].int().cpu(), src_str=src_str, alignment=hypo["alignment"],
                                                           align_dict=None, tgt_dict=tgt_dict, remove_bpe=post_process, extra_symbols_to_ignore=strip)
            detok = hypo_str.replace("<unk>", " ")
            score = hypo["score"] / math.log(2)
            lines.append("H-{}\t{}\t{}".format(id_, score, hypo_str))
            lines.append("D-{}\t{}\t{}".format(id_, score, detok))
            lines.append("P-{}\t{}".format(id_, " ".join(map(lambda x: "{:.4f}".format(x), hypo["positional_scores"].clone().div_(math.log(2)).tolist()))))
    return lines


def run_buffers(out, key, path, buffer_size, cfg, task, models, gen, max_positions, strip):
    """fairseq_cli/interactive.py:207-301 over the reference's own buffered_read and make_batches."""
    from fairseq.token_generation_constraints import unpack_constraints
    from fairseq_cli.interactive import buffered_read, make_batches
    src_dict, tgt_dict = task.source_dictionary, task.target_dictionary
    start_id, lines, reordered = 0, [], False
    for k, inputs in enumerate(buffered_read(path, buffer_size)):
        results = []
        for j, batch in enumerate(make_batches(inputs, cfg, task, max_positions, lambda x: x)):
            bk = "%s/buffer%d/batch%d" % (key, k, j)
            out[bk + "/id"] = batch.ids.numpy()
            out[bk + "/src_lengths"] = batch.src_lengths.numpy()
            out[bk + "/src_tokens"] = batch.src_tokens.numpy()
            if batch.constraints is not None:
                out[bk + "/constraints"] = batch.constraints.numpy()
            sample = {"net_input": {"src_tokens": batch.src_tokens, "src_lengths": batch.src_lengths}}
            translations = task.inference_step(gen, models, sample, constraints=batch.constraints)
            put_hyps(out, bk, translations)
            cons = [unpack_constraints(c) for c in batch.constraints] if batch.constraints is not None else [[] for _ in translations]
            for i, (id_, hypos) in enumerate(zip(batch.ids.tolist(), translations)):
                src_i = batch.src_tokens[i]
                if src_i.dtype is not torch.float:
                    src_i = src_i[src_i.ne(tgt_dict.pad())]
                results.append((start_id + id_, src_i, hypos, {"constraints": cons[i], "time": 0.0}))
            out["%s/buffer%d/nbatches" % (key, k)] = np.int64(j + 1)
        order = [r[0] - start_id for r in results]
        reordered = reordered or order != sorted(order)
        lines += print_lines(results, src_dict, tgt_dict, 1, strip)
        start_id += len(inputs)
        out[key + "/nbuffers"] = np.int64(k + 1)
    out[key + "/stdout"] = np.array("\n".join(lines) + "\n")
    for l in lines:
        print("   ", l)
    return reordered


def record_st(out, tmp):
    """ref_checkpoint_tiny.pt through the reference's TripletTask on a relocated copy of data_tiny whose dictionary is padded to the
    model's 60 symbols (filler<i>, as tests/test_decode_lm_gpu.py does for the command line)."""
    import shutil

    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator
    from fairseq.tasks.triplet import TripletTask
    data = os.path.join(GOLDEN, "data_tiny")
    root = os.path.join(tmp, "st_data")
    os.makedirs(root)
    for f in os.listdir(data):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(data, f), os.path.join(root, f))
    cfg_path = os.path.join(root, "config_wave.yaml")
    text = open(cfg_path).read().replace("AUDIO_ROOT", data)
    open(cfg_path, "w").write(text)
    words = open(os.path.join(root, "dict.txt")).read().splitlines()
    words += ["filler%d 1" % i for i in range(MG.VOCAB - 4 - len(words))]
    open(os.path.join(root, "dict.txt"), "w").write("\n".join(words) + "\n")
    state = torch.load(os.path.join(GOLDEN, "ref_checkpoint_tiny.pt"), weights_only=False)
    targs = Namespace(data=root, config_yaml="config_wave.yaml", max_source_positions=2000000, max_target_positions=1024, seed=1,
                      dump_feature_to_file=None, sample_rate=16000, normalize=False, train_subset="train_st")
    task = TripletTask.setup_task(targs)
    assert len(task.target_dictionary) == MG.VOCAB
    w2v_path = os.path.join(tmp, "w2v_tiny.pt")
    MG.build_w2v_ckpt(w2v_path, seed=11)
    model = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
    model.load_state_dict(state["model"], strict=True)
    model.eval()
    model.encoder.wav2vec_model.encoder.pos_conv.register_forward_pre_hook(lambda m, i: (i[0].contiguous(),))
    lines = [os.path.join(data, l) for l in ST_LINES]
    n = task.get_interactive_tokens_and_lengths(lines, lambda x: x)[1]
    out["st/lines"] = np.array(ST_LINES)
    out["st/lengths"] = np.asarray(n, dtype=np.int64)
    max_tokens = 2 * max(n)  # the two longest share a batch (rows x the longest row), the third does not fit
    assert 3 * max(n) > max_tokens
    out["st/max_tokens"] = np.int64(max_tokens)
    out["st/beam"], out["st/max_len_b"] = np.int64(ST_BEAM), np.int64(ST_MAX_LEN_B)
    path = os.path.join(tmp, "st_input.txt")
    open(path, "w").write("".join(l + "\n" for l in lines))
    gen = SequenceGenerator([model], task.target_dictionary, beam_size=ST_BEAM, max_len_a=0, max_len_b=ST_MAX_LEN_B)
    from fairseq import utils
    max_positions = utils.resolve_max_positions(task.max_positions(), model.max_positions())
    reordered = False
    for size in (1, 3):
        cfg = Namespace(generation=Namespace(constraints=False),
                        dataset=Namespace(max_tokens=max_tokens, batch_size=None, skip_invalid_size_inputs_valid_test=False))
        with torch.no_grad():
            r = run_buffers(out, "st/buf%d" % size, path, size, cfg, task, [model], gen, max_positions, {task.target_dictionary.eos()})
        reordered = reordered or r
        if size == 3:
            assert int(out["st/buf3/buffer0/nbatches"]) == 2, "--max-tokens must cut the buffer of 3 into two batches"
    assert reordered, "st: no buffer's batch order differs from input order"


def record_mt(out, tmp):
    """The chimera_tiny.npz model fed typed sentences through the reference's TranslationTask on translation_tiny."""
    import make_translation_goldens as TG
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator
    from fairseq.tasks.translation import TranslationTask
    from fairseq import search
    g = np.load(os.path.join(GOLDEN, "chimera_tiny.npz"), allow_pickle=False)
    task = TranslationTask.setup_task(TG.task_args())
    d = task.target_dictionary
    w2v_path = os.path.join(tmp, "w2v_tiny_mt.pt")
    MG.build_w2v_ckpt(w2v_path, seed=11)
    model = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), MG.TaskStub(d))
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    model.eval()
    with torch.no_grad():  # the loaded model must BE the fixture's: its stored text-pass logits come back
        (logits, _), _ = model.forward_with_internal(torch.from_numpy(g["in/src_text"]), torch.from_numpy(g["in/src_text_lengths"]),
                                                     torch.from_numpy(g["in/prev_output_tokens"]))
    assert float((logits - torch.from_numpy(g["out/mt_logits"])).abs().max()) < 1e-5
    text = open(os.path.join(TG.ROOT, "corpus", "test.en.txt"), encoding="utf-8").read().split("\n")[:-1]
    from fairseq import utils
    max_positions = utils.resolve_max_positions(task.max_positions(), model.max_positions())
    # (the reference's collater sorts a batch's rows by length but leaves its constraints in sampler order, language_pair_dataset.py
    # :100-113: in a batch of several sentences they reach the wrong rows.  The constrained line is the buffer's longest and
    # --max-tokens leaves it a batch of its own, so the case records what the reference MEANS: the phrases of a line constrain it.)
    cases = {"plain": (text, False, 3), "plain_buf1": (text, False, 1), "constrained": ([text[0] + "\tw5 w9\tw30", text[3], text[5]], "ordered", 3)}
    out["mt/beam"], out["mt/max_len_a"], out["mt/max_len_b"] = np.int64(MT_BEAM), np.float64(MT_MAX_LEN_A), np.int64(MT_MAX_LEN_B)
    out["mt/max_tokens"] = np.int64(MT_MAX_TOKENS)
    reordered = False
    for case, (lines, constraints, size) in cases.items():
        out["mt/%s/lines" % case] = np.array(lines)
        out["mt/%s/buffer_size" % case] = np.int64(size)
        path = os.path.join(tmp, "mt_%s.txt" % case)
        open(path, "w", encoding="utf-8").write("".join(l + "\n" for l in lines))
        strategy = search.LexicallyConstrainedBeamSearch(d, constraints) if constraints else None
        gen = SequenceGenerator([model], d, beam_size=MT_BEAM, max_len_a=MT_MAX_LEN_A, max_len_b=MT_MAX_LEN_B, search_strategy=strategy)
        cfg = Namespace(generation=Namespace(constraints=constraints),
                        dataset=Namespace(max_tokens=MT_MAX_TOKENS, batch_size=None, skip_invalid_size_inputs_valid_test=False))
        with torch.no_grad():
            r = run_buffers(out, "mt/" + case, path, size, cfg, task, [model], gen, max_positions, {d.eos()})
        reordered = reordered or r
        if constraints:
            k = [j for j in range(int(out["mt/constrained/buffer0/nbatches"])) if 0 in out["mt/constrained/buffer0/batch%d/id" % j].tolist()]
            assert len(out["mt/constrained/buffer0/batch%d/id" % k[0]]) == 1, "the constrained line must be a batch of its own"
    assert reordered, "mt: no buffer's batch order differs from input order"


def main(write=True, parts=("lm", "st", "mt")):
    import make_data_goldens as DG
    tmp = tempfile.mkdtemp()
    DG.build_cython_batcher(tmp)
    import make_lm_goldens as LG
    LG.build_cython_token_blocks(tmp)
    out = {"meta/printed_by": np.array("harness restatement (print_lines) over the reference's Dictionary.string and "
                                       "utils.post_process_prediction; W- times are 0.000")}
    if "lm" in parts:
        record_lm(out)
    if "st" in parts:
        record_st(out, tmp)
    if "mt" in parts:
        record_mt(out, tmp)
    if not write:
        return out
    path = os.path.join(GOLDEN, "interactive_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote interactive_tiny.npz: %d bytes, %d arrays" % (os.path.getsize(path), len(out)))
    return out


def search_seed(limit=200):
    import make_data_goldens as DG
    import make_lm_goldens as LG
    tmp = tempfile.mkdtemp()
    DG.build_cython_batcher(tmp)
    LG.build_cython_token_blocks(tmp)
    for seed in range(limit):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                record_lm({}, seed)
        except AssertionError as e:
            print("seed", seed, "fails:", str(e)[:100])
            continue
        print("seed", seed, "meets every condition")
        return seed


if __name__ == "__main__":
    if sys.argv[1:] == ["--search"]:
        search_seed()
    else:
        main(parts=tuple(sys.argv[1:]) or ("lm", "st", "mt"))
