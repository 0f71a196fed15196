"""GPU tests of --score-reference: cst_score_tokens (csrc/score.hip) against the fp64 restatement under the derived bound of
tests/score_ref.py with zero elements over it, the wrapper's checks, SequenceScorer against the fixture the REAL reference's
SequenceScorer produced (decode_score_tiny.npz), and fairseq_generate.py --score-reference in a child process."""
import ast
import functools
import json
import os
import shutil
import subprocess
import sys
from argparse import Namespace
from importlib import import_module

import pytest
import torch

from conftest import ROOT, load_golden, load_pkg
from score_ref import score_bounds, score_check, score_inputs, score_ref64, worst_ratio

pytestmark = pytest.mark.gpu
PAD = 1
F, B16 = torch.float32, torch.bfloat16


def mods():
    load_pkg()
    return import_module("chimera-st_amd.lib"), import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.sequence_scorer")


@functools.lru_cache(maxsize=None)
def case(B, T, V, N, dtype):
    """Inputs and their fp64 reference, computed once per shape (the row stride does not enter)."""
    xs, t = score_inputs(B, T, V, N, dtype)
    return xs, t, score_ref64(xs, t, PAD)


def launch(L, xs, t, ld, shift):
    """cst_score_tokens through the C ABI on copies of xs with row stride ld whose base is `shift` elements behind a 16-byte
    boundary; pos and score start as NaN, len as -1.  -> (pos, score, len, return code)."""
    B, T, V = xs[0].shape
    bufs = []
    for x in xs:
        buf = torch.zeros(B * T * ld + 16, dtype=x.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + B * T * ld].view(B * T, ld)[:, :V] = x.reshape(B * T, V).cuda()
        bufs.append(buf)
    pos = torch.full((B, T), float("nan"), device="cuda")
    score = torch.full((B,), float("nan"), device="cuda")
    length = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    td = t.cuda()
    es = xs[0].element_size()
    others = (L.c_p * 7)(*[b.data_ptr() + shift * es for b in bufs[1:]])
    rc = L.load().cst_score_tokens(bufs[0].data_ptr() + shift * es, others, len(xs), ld, L.ptr(td), PAD, L.ptr(pos), L.ptr(score),
                                   L.ptr(length), B, T, V, L.dtype_code(xs[0].dtype), L.stream_ptr())
    torch.cuda.synchronize()
    return pos, score, length, rc


@pytest.mark.parametrize("dtype", [B16, F], ids=["bf16", "f32"])
@pytest.mark.parametrize("N", [1, 2, 8])
@pytest.mark.parametrize("BT", [(1, 1), (3, 7)], ids=["1x1", "3x7"])
@pytest.mark.parametrize("V", [5, 63, 64, 257, 10000, 20481])
def test_kernel_under_the_derived_bound(V, BT, N, dtype):
    """Both row layouts: ld = V from a 16-byte aligned base, and ld = (V + 7)//8*8 + 8 from a base one element behind a boundary.
    Targets 0 and V - 1 occur, members 1 and 2 are offset by +80 / -80, sentence 1 of the 3 x 7 batch is fully padded (NaN, len 0),
    and the output buffers start as NaN, so the zeros at pad positions have to be written."""
    L, _, _ = mods()
    xs, t, r = case(BT[0], BT[1], V, N, dtype)
    for ld, shift in ((V, 0), ((V + 7) // 8 * 8 + 8, 1)):
        pos, score, length, rc = launch(L, xs, t, ld, shift)
        assert rc == 0, L.load().cst_last_error()
        assert bool((pos.cpu()[t.eq(PAD)] == 0).all()), "pad positions must be written as 0"
        (rp, bp), (rs, bs), exact = score_check(pos, score, length, r, dtype)
        print("V%d %dx%d N%d %s ld%d: worst pos ratio %.3f, worst score ratio %.3f" % (V, BT[0], BT[1], N, dtype, ld, rp, rs))
        assert bp == 0 and bs == 0 and exact, (ld, rp, bp, rs, bs, exact)


def test_two_runs_are_bit_equal():
    L, _, _ = mods()
    xs, t, _ = case(3, 7, 10000, 2, B16)
    a, b = launch(L, xs, t, 10000, 0), launch(L, xs, t, 10000, 0)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_bad_scalar_arguments_are_errors():
    L, _, _ = mods()
    xs, t, _ = case(3, 7, 64, 2, F)
    x, td = xs[0].cuda(), t.cuda()
    out = torch.zeros(64, device="cuda")
    ln = torch.zeros(3, dtype=torch.int32, device="cuda")
    call = lambda members, ld, others, dt=0: L.load().cst_score_tokens(  # noqa: E731
        L.ptr(x), others, members, ld, L.ptr(td), PAD, L.ptr(out), L.ptr(out[32:]), L.ptr(ln), 3, 7, 64, dt, L.stream_ptr())
    none = (L.c_p * 7)()
    assert call(9, 64, none) == -1 and b"members" in L.load().cst_last_error()
    assert call(0, 64, none) == -1
    assert call(1, 63, none) == -1 and b"row stride" in L.load().cst_last_error()
    assert call(2, 64, none) == -1 and b"member 1" in L.load().cst_last_error()
    assert call(1, 64, none, 7) == -1 and b"dtype" in L.load().cst_last_error()
    assert call(1, 64, none) == 0


def test_wrapper_refuses_an_id_outside_the_vocabulary(monkeypatch):
    L, K, _ = mods()
    xs, t, r = case(3, 7, 64, 2, F)
    dev = [x.cuda() for x in xs]
    pos, score, length, packed = K.score_tokens(dev, t.cuda(), PAD)  # the wrapper's own path, and views of one buffer
    (_, bp), (_, bs), exact = score_check(pos, score, length, r, F)
    assert bp == 0 and bs == 0 and exact and packed.numel() == 3 * 7 + 2 * 3
    wide = torch.zeros(2, 3, 7, 80, device="cuda")  # views with a row stride and an unaligned base go in as they are
    wide[..., 3:67] = torch.stack(dev)
    p2 = K.score_tokens([wide[0, ..., 3:67], wide[1, ..., 3:67]], t.cuda(), PAD)[0]
    assert torch.equal(p2, pos)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    monkeypatch.setattr(K.L, "load", lambda: NoLaunch())
    for bad in (64, -1):
        tb = t.clone()
        tb[0, 2] = bad
        with pytest.raises(ValueError, match="target ids"):
            K.score_tokens(dev, tb.cuda(), PAD)


# ---- SequenceScorer on the fixture's models ----------------------------------------------------------------------------------------
def fixture_sample(fix, rec, tag):
    return {"net_input": {"src_tokens": torch.from_numpy(rec["in/%s/src_tokens" % tag]).repeat_interleave(2, 0).cuda(),
                          "src_lengths": torch.from_numpy(rec["in/%s/src_lengths" % tag]).repeat_interleave(2, 0).cuda(),
                          "prev_output_tokens": torch.from_numpy(fix["%s/prev_output_tokens" % tag]).cuda()},
            "target": torch.from_numpy(fix["%s/target" % tag]).cuda()}


def padded(hyps, T):
    pos = torch.zeros(len(hyps), T)
    for b, h in enumerate(hyps):
        assert len(h) == 1 and h[0]["attention"] is None and h[0]["alignment"] is None
        pos[b, :h[0]["positional_scores"].numel()] = h[0]["positional_scores"].float().cpu()
    return pos, torch.stack([h[0]["score"].float().cpu() for h in hyps]), torch.tensor([h[0]["tokens"].numel() for h in hyps])


@pytest.mark.parametrize("N", [1, 2, 3])
def test_scorer_reproduces_the_reference_fp32(N):
    from test_ensemble_gpu import fixture_members
    _, _, SS = mods()
    models, task, _, _ = fixture_members(N)
    fix, rec = load_golden("decode_score_tiny.npz"), load_golden("decode_recipe_tiny.npz")
    for tag in ("a", "b"):
        sample = fixture_sample(fix, rec, tag)
        T = sample["target"].size(1)
        out = {}
        for fused in (True, False):
            hyps = SS.SequenceScorer(task.target_dictionary, fused=fused).generate(models, sample)
            pos, score, length = out[fused] = padded(hyps, T)
            assert length.tolist() == fix["n%d/%s/len" % (N, tag)].tolist()
            for b, h in enumerate(hyps):
                assert h[0]["tokens"].tolist() == fix["%s/target" % tag][b][:int(length[b])].tolist()
            assert float((pos - torch.from_numpy(fix["n%d/%s/pos_scores" % (N, tag)])).abs().max()) < 1e-4, (tag, fused)
            assert float((score - torch.from_numpy(fix["n%d/%s/score" % (N, tag)])).abs().max()) < 1e-4, (tag, fused)
        fused_equals_unfused(models, sample, out, F)


def fused_equals_unfused(models, sample, out, dtype):
    """The kernel and the plain-torch scorer on the SAME logits: their difference within the kernel's bound, and the kernel within
    it of the fp64 restatement."""
    with torch.no_grad():
        logits = [m(**sample["net_input"])[0].cpu() for m in models]
    r = score_ref64(logits, sample["target"].cpu(), PAD)
    b_pos, b_score = score_bounds(r, dtype)
    (rp, bp), (rs, bs), exact = score_check(*out[True], r, dtype)
    assert bp == 0 and bs == 0 and exact, (rp, rs)
    dp, ds = worst_ratio(out[True][0], out[False][0], b_pos), worst_ratio(out[True][1], out[False][1], b_score)
    print("fused vs fp64: %.3f / %.3f of the bound; fused vs unfused: %.3f / %.3f" % (rp, rs, dp[0], ds[0]))
    assert dp[1] == 0 and ds[1] == 0 and out[True][2].tolist() == out[False][2].tolist()


@pytest.mark.parametrize("N", [1, 3])
def test_scorer_bf16_fused_equals_unfused(N):
    from test_ensemble_gpu import fixture_members
    _, _, SS = mods()
    models, task, _, _ = fixture_members(N, torch.bfloat16)
    fix, rec = load_golden("decode_score_tiny.npz"), load_golden("decode_recipe_tiny.npz")
    sample = fixture_sample(fix, rec, "b")
    sample["net_input"]["src_tokens"] = sample["net_input"]["src_tokens"].float()  # (raw audio stays fp32, as in training)
    out = {fused: padded(SS.SequenceScorer(task.target_dictionary, fused=fused).generate(models, sample), sample["target"].size(1))
           for fused in (True, False)}
    fused_equals_unfused(models, sample, out, B16)


def test_scorer_input_errors():
    from test_ensemble_gpu import fixture_members
    _, _, SS = mods()
    models, task, _, _ = fixture_members(1)
    fix, rec = load_golden("decode_score_tiny.npz"), load_golden("decode_recipe_tiny.npz")
    sample = fixture_sample(fix, rec, "a")
    with pytest.raises(ValueError, match="target"):
        SS.SequenceScorer(task.target_dictionary).generate(models, {"net_input": sample["net_input"]})
    other = import_module("chimera-st_amd.dictionary").Dictionary.synthetic(len(task.target_dictionary) + 3)
    with pytest.raises(ValueError, match="target vocabulary"):
        SS.SequenceScorer(other).generate(models, sample)


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_score_reference_in_a_child_process(tmp_path, capsys):
    """fairseq_generate.py --score-reference on tests/golden/data_tiny with a checkpoint trained as test_cli_gpu.py trains its own
    (one epoch), each run in a fresh process."""
    from test_cli_gpu import DATA, _tiny_cli_flags
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    g = load_golden("chimera_tiny.npz")
    w2v = str(tmp_path / "w2v_tiny_random.pt")
    torch.save({"args": Namespace(**ast.literal_eval(str(g["meta/w2v_args"]))), "model": None}, w2v)
    root = tmp_path / "data"
    root.mkdir()
    for f in os.listdir(DATA):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(DATA, f), root / f)
    (root / "config_wave.yaml").write_text((root / "config_wave.yaml").read_text().replace("AUDIO_ROOT", DATA))
    save = str(tmp_path / "ckpt")
    assert cli.train_main(_tiny_cli_flags(root, save, w2v) + ["--max-epoch", "1", "--disable-validation"]) is not None
    capsys.readouterr()
    cmd = [sys.executable, os.path.join(ROOT, "fairseq_generate.py"), str(root), "--task", "triplet", "--config-yaml", "config_wave.yaml",
           "--path", os.path.join(save, "checkpoint_last.pt"), "--gen-subset", "dev_st", "--max-tokens", "12000", "--beam", "3", "--nbest", "2",
           "--max-len-b", "10", "--max-source-positions", "2000000"]

    def run(extra):
        p = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
        lines = p.stdout.splitlines()
        rows = {k: {} for k in "THDP"}
        for line in lines:
            if line[:2] in ("T-", "H-", "D-", "P-"):
                sid, *rest = line[2:].split("\t")
                assert int(sid) not in rows[line[0]] or not extra, "one hypothesis per sentence"
                rows[line[0]][int(sid)] = rest
        return json.loads([line for line in lines if line.startswith("{")][-1]), rows

    summary, rows = run(["--score-reference"])
    assert summary["score_reference"] is True and summary["sentences"] == 4 == len(rows["T"]) == len(rows["H"]) == len(rows["P"])
    for sid, (ref,) in rows["T"].items():
        score, hyp = rows["H"][sid]
        assert hyp == ref, sid
        p = [float(x) for x in rows["P"][sid][0].split()]
        assert len(p) == len(ref.split()) + 1, (sid, p, ref)  # the target's tokens and eos
        # H prints 6 decimals of the mean, P 4 decimals of each term: |mean(P) - H| <= 0.5e-4 + 0.5e-6 (+ fp32 rounding of the mean)
        assert abs(sum(p) / len(p) - float(score)) <= 0.5e-4 + 0.5e-6 + 1e-6 * abs(float(score)), (sid, p, score)
    summary, rows = run([])
    assert summary["score_reference"] is False and summary["sentences"] == 4 == len(rows["T"]) and len(rows["H"]) == 4
