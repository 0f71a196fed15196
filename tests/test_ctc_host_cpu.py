"""No-GPU checks of the CTC entries of the C ABI: cst_ctc_fwd / cst_ctc_bwd / cst_ctc_greedy reject null operands, bad dtypes and bad
scalars before any HIP call, with a message; cst_edit_distance equals a plain dynamic programme."""
import ctypes
import random

import numpy as np
import pytest

from conftest import load_pkg


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as ge
    L = load_pkg().lib
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    return L


def test_ctc_entries_reject_bad_arguments_before_any_hip_call(lib):
    l = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    T, B, V = 2, 2, 4

    def fwd(logits=p, tl=p, il=p, nll=p, dtype=0, blank=0, Lmax=1, V_=V):
        return l.cst_ctc_fwd(logits, B * V, V, p, Lmax, tl, il, blank, 0, nll, p, p, p, p, None, T, B, V_, dtype, None)

    def bwd(logits=p, gscale=p, d=p, dtype=0, dst=B * V):
        return l.cst_ctc_bwd(logits, B * V, V, p, 1, p, p, 0, 0, p, p, p, p, gscale, d, dst, V, T, B, V, dtype, None)

    def greedy(logits=p, ids=p, dtype=0, blank=0):
        return l.cst_ctc_greedy(logits, B * V, V, p, blank, p, ids, p, T, B, V, dtype, None)

    for call, kw, msg in ((fwd, dict(logits=None), b"null operand"), (fwd, dict(tl=None), b"null operand"), (fwd, dict(il=None), b"null operand"),
                          (fwd, dict(nll=None), b"null operand"), (fwd, dict(dtype=2), b"bad dtype"), (fwd, dict(blank=V), b"blank"),
                          (fwd, dict(V_=0), b"bad shape"),
                          (bwd, dict(logits=None), b"null operand"), (bwd, dict(gscale=None), b"null operand"), (bwd, dict(d=None), b"null operand"),
                          (bwd, dict(dtype=-1), b"bad dtype"), (bwd, dict(dst=V - 1), b"gradient layout"),
                          (greedy, dict(logits=None), b"null operand"), (greedy, dict(ids=None), b"null operand"),
                          (greedy, dict(dtype=9), b"bad dtype"), (greedy, dict(blank=-2), b"blank")):
        assert call(**kw) == -1, (call.__name__, kw)
        assert msg in l.cst_last_error(), (call.__name__, kw, l.cst_last_error())
    assert fwd(Lmax=2048) == -4 and b"exceed the supported 2047" in l.cst_last_error()


def levenshtein(a, b):
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def test_edit_distance_against_plain_dp(lib):
    K = __import__("importlib").import_module("chimera-st_amd.kernels")
    rng = random.Random(5)
    pairs = [([], []), ([], [3, 4]), ([7], []), ([1, 2, 3], [1, 2, 3]), ([1, 2, 3], [3, 2, 1])]
    for _ in range(60):
        alphabet = rng.choice([2, 4, 30])
        pairs.append(([rng.randrange(alphabet) for _ in range(rng.randrange(0, 40))], [rng.randrange(alphabet) for _ in range(rng.randrange(0, 40))]))
    for a, b in pairs:
        assert K.edit_distance(a, b) == levenshtein(a, b), (a, b)
        assert K.edit_distance(b, a) == levenshtein(a, b)
    assert K.edit_distance(np.array([2 ** 40, 5]), [2 ** 40 + 1, 5]) == 1  # 64-bit ids
    assert lib.load().cst_edit_distance(None, -1, None, 0) == -1


def test_post_process_and_wer_args_refusal():
    from types import SimpleNamespace
    load_pkg()
    C = __import__("importlib").import_module("chimera-st_amd.criterions")
    D = __import__("importlib").import_module("chimera-st_amd.dictionary").Dictionary
    # data/data_utils.py:340-351
    assert C.post_process("h e l l o | w o r l d |", "letter") == "hello world"
    assert C.post_process("▁he llo ▁wor ld", "sentencepiece") == "hello world"
    assert C.post_process("he llo_ wor ld_", "wordpiece") == "hello world"
    assert C.post_process("he llo_EOW wor ld_EOW", "_EOW") == "hello world"
    assert C.post_process("he@@ llo wor@@ ld", "@@ ") == "hello world"
    assert C.post_process("a b", "none") == "a b" and C.post_process("a b", None) == "a b"
    task = SimpleNamespace(target_dictionary=D())
    with pytest.raises(NotImplementedError, match="wer-args"):
        C.CtcCriterion(task, wer_args="('lm.bin', 'lexicon.txt', 2, -1)")
    crit = C.CtcCriterion(task, post_process=None)
    assert crit.blank_idx == 0 and crit.post_process == "letter" and crit.logging_keys() == ("loss", "ntokens", "nsentences", "sample_size")
    assert crit.derived_metrics({"c_total": 0.0, "w_total": 0.0}) == {}
