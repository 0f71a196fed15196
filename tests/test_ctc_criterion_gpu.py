"""Criterion `ctc` on the GPU with a stub model that returns given logits: loss, gradient and sample sizes against the reference
criterion's own calls (F.ctc_loss on fp32 log_softmax, targets flattened by masked_select) evaluated in fp64 on the CPU; the eval-mode
error counts against the reference's host loop restated with a plain edit distance; no host synchronisation in a training step."""
from importlib import import_module
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_pkg
from test_ctc_host_cpu import levenshtein

pytestmark = pytest.mark.gpu


def letter_task():
    load_pkg()
    D = import_module("chimera-st_amd.dictionary").Dictionary
    d = D()
    for s in "|abcde":
        d.add_symbol(s)
    return SimpleNamespace(target_dictionary=d)


class Stub(nn.Module):
    def __init__(self, logits, padding_mask):
        super().__init__()
        self.logits = nn.Parameter(logits)
        self.padding_mask = padding_mask

    def forward(self, source=None, padding_mask=None):
        return {"encoder_out": self.logits, "padding_mask": self.padding_mask, "encoder_padding_mask": self.padding_mask}


def make_sample(task, texts, T, seed=3, planted=None):
    d = task.target_dictionary
    B, V = len(texts), len(d)
    rows = [[d.index(c) for c in t] for t in texts]
    Lmax = max(len(r) for r in rows) + 1
    target = torch.full((B, Lmax), d.pad(), dtype=torch.int64)
    for b, r in enumerate(rows):
        target[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
    target[0, len(rows[0])] = d.eos()  # an eos behind the labels is removed like the padding
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    x = torch.randn(T, B, V, generator=g) * 2
    in_len = torch.tensor([T - 3 * b for b in range(B)], dtype=torch.int64)
    if planted is not None:
        for b, path in enumerate(planted):
            for t, c in enumerate(path):
                x[t, b, d.index(c) if c != "_" else d.bos()] = 12.0
    pm = torch.arange(T)[None, :] >= in_len[:, None]
    sample = {"id": torch.arange(B), "net_input": {"source": torch.zeros(B, 8), "padding_mask": torch.zeros(B, 8, dtype=torch.bool)},
              "target": target, "target_lengths": lens, "ntokens": int(lens.sum())}
    return sample, x, pm, in_len


def to_cuda(s):
    if torch.is_tensor(s):
        return s.cuda()
    if isinstance(s, dict):
        return {k: to_cuda(v) for k, v in s.items()}
    return s


def reference_loss(task, sample, x, in_len, zero_infinity=False):
    d = task.target_dictionary
    xd = x.double().requires_grad_(True)
    keep = (sample["target"] != d.pad()) & (sample["target"] != d.eos())
    loss = F.ctc_loss(F.log_softmax(xd, -1), sample["target"].masked_select(keep), in_len, sample["target_lengths"], blank=d.bos(),
                      reduction="sum", zero_infinity=zero_infinity)
    loss.backward()
    return float(loss), xd.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("sentence_avg", [False, True])
def test_training_step(dtype, sentence_avg):
    task = letter_task()
    C = import_module("chimera-st_amd.criterions")
    sample, x, pm, in_len = make_sample(task, ["ab|cab", "e|dd", "c"], T=17)
    x = x.to(dtype)
    crit = C.CtcCriterion(task, sentence_avg=sentence_avg)
    model = Stub(x.cuda(), pm.cuda()).train()
    dev = to_cuda(sample)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # a host synchronisation inside the step raises
    try:
        loss, sample_size, log = crit(model, dev)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref, gref = reference_loss(task, sample, x.float(), in_len)
    # fp32 recursion over 17 frames: ctc_ref's bound at this size is below 1e-5 relative (tests/test_ctc_gpu.py pins the kernel itself)
    assert abs(float(loss) - ref) < 1e-5 * abs(ref)
    tol = 2.0 ** -8 if dtype == torch.bfloat16 else 1e-5
    assert float((model.logits.grad.float().cpu() - gref).abs().max()) < tol
    assert sample_size == (3 if sentence_avg else sample["ntokens"])
    assert set(log) == set(crit.logging_keys()) and log["nsentences"] == 3 and log["ntokens"] == sample["ntokens"]
    assert crit.logging_outputs_can_be_summed() and crit.single_pass


def test_validation_counts_and_derived_metrics():
    task = letter_task()
    d = task.target_dictionary
    C = import_module("chimera-st_amd.criterions")
    texts = ["ab|cab", "e|dd", "c"]
    # best paths: "ab|cb" (one unit and one word wrong), "e|dd" exact (the repeat needs the blank), "" (everything missing)
    planted = ["aab_|ccb_________", "e_|_d_d_______", "___________"]
    sample, x, pm, in_len = make_sample(task, texts, T=17, planted=planted)
    crit = C.CtcCriterion(task)
    model = Stub(x.cuda(), pm.cuda()).eval()
    with torch.no_grad():
        loss, _, log = crit(model, to_cuda(sample))
    # the reference's loop (criterions/ctc.py:127-175) on the host
    c_err = c_len = w_err = w_len = 0
    for b in range(3):
        lp = F.log_softmax(x[:int(in_len[b]), b].float(), -1)
        toks = lp.argmax(dim=-1).unique_consecutive()
        pred = toks[toks != d.bos()].tolist()
        targ = [d.index(c) for c in texts[b]]
        c_err += levenshtein(pred, targ)
        c_len += len(targ)
        tw = C.post_process(d.string(targ), "letter").split()
        pw = C.post_process(d.string(pred), "letter").split()
        w_err += levenshtein(pw, tw)
        w_len += len(tw)
    assert (c_err, c_len, w_err, w_len) == (2, 11, 2, 5)
    assert {k: log[k] for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total")} == \
        {"c_errors": c_err, "c_total": c_len, "w_errors": w_err, "wv_errors": w_err, "w_total": w_len}
    ref, _ = reference_loss(task, sample, x, in_len)
    assert abs(float(loss) - ref) < 1e-5 * abs(ref)
    m = crit.derived_metrics({k: float(v) for k, v in log.items() if k != "loss"})
    assert m == {"uer": round(200.0 / 11, 3), "wer": 40.0, "raw_wer": 40.0}


def test_zero_infinity_and_registry():
    task = letter_task()
    C = import_module("chimera-st_amd.criterions")
    R = import_module("chimera-st_amd.registry")
    assert R.CRITERION_REGISTRY["ctc"] is C.CtcCriterion
    sample, x, pm, in_len = make_sample(task, ["aabbccddee", "ab"], T=12)  # 10 labels + 5 repeats in 12 frames: infeasible
    for zi in (False, True):
        crit = C.CtcCriterion(task, zero_infinity=zi)
        model = Stub(x.cuda(), pm.cuda()).train()
        loss, _, _ = crit(model, to_cuda(sample))
        loss.backward()
        ref, gref = reference_loss(task, sample, x, in_len, zero_infinity=zi)
        if zi:
            assert abs(float(loss) - ref) < 1e-5 * abs(ref)
            assert float((model.logits.grad.cpu() - gref).abs().max()) < 1e-5
        else:
            assert float(loss) == float("inf") and ref == float("inf")
