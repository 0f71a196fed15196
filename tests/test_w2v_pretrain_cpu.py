"""Host side of the wav2vec2 pre-training head without a GPU: the four entries are declared, bound and exported; every refusal of
include/cst.h happens in argument validation, before any HIP call (so it can be shown here, on fake addresses that are never followed);
the wrappers fail loudly on CPU tensors; the scope notes say what is and is not built."""
import os
from importlib import import_module

import pytest
import torch

from conftest import ROOT, load_pkg

ENTRIES = ("cst_w2v_negatives", "cst_infonce_fwd", "cst_infonce_bwd_x", "cst_infonce_bwd_y", "cst_gumbel_vq_fwd", "cst_gumbel_vq_bwd")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    L = load_pkg().lib
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    return L


def test_entries_are_declared_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "cst.h")).read()
    bound = {n for n, _, _ in lib.SYMBOLS}
    for name in ENTRIES:
        assert "int %s(" % name in header and name in bound and hasattr(lib.load(), name)
    assert lib.ABI_VERSION == 13  # added without a bump: no existing signature changed
    assert "w2v_pretrain.hip" in open(os.path.join(ROOT, "chimera-st_amd", "csrc", "Makefile")).read()


def test_refusals_happen_before_any_device_call(lib):
    """The addresses below are never followed: every call is refused by its shape."""
    c, last = lib.load(), lib.load().cst_last_error
    A = 0x10000  # 16-byte aligned, non-null

    def fwd(N=6, KP=3, D=16, dtype=0, x=A):
        return c.cst_infonce_fwd(x, A, A, 10.0, A, A, A, A, A, A, A, None, N, KP, D, dtype, None)
    for kw, msg in ((dict(D=12), b"multiple of 8"), (dict(D=1032), b"at most 1024"), (dict(KP=1024), b"negatives exceed"),
                    (dict(KP=0), b"bad shape"), (dict(N=0), b"bad shape"), (dict(dtype=3), b"bad dtype"), (dict(x=A + 4), b"aligned"),
                    (dict(x=None), b"null operand"), (dict(N=1 << 28, KP=100), b"bad shape")):
        assert fwd(**kw) == -1 and msg in last(), kw
    assert c.cst_infonce_bwd_x(A, A, A, 10.0, A, A, A, A, A, A, 6, 3, 20, 0, None) == -1 and b"multiple of 8" in last()
    assert c.cst_infonce_bwd_x(A, A, A, 10.0, A, A, A, None, A, A, 6, 3, 16, 0, None) == -1 and b"null operand" in last()
    assert c.cst_infonce_bwd_y(A, A, A, A, A, A, A, A, 6, 3, 2048, 0, None) == -1 and b"at most 1024" in last()
    assert c.cst_infonce_bwd_y(A, A, None, A, A, A, A, A, 6, 3, 16, 0, None) == -1 and b"null operand" in last()
    assert c.cst_w2v_negatives(1, 2, 1, 4, 0, A, None) == -1 and b"M >= 2" in last()
    assert c.cst_w2v_negatives(1, 1, 1, 0, 4, A, None) == -1 and b"B M >= 2" in last()
    assert c.cst_w2v_negatives(1, 2, 2, 0, 0, A, None) == -1 and b"bad shape" in last()
    assert c.cst_w2v_negatives(1, 1 << 20, 1 << 12, 1, 0, A, None) == -1 and b"bad shape" in last()
    assert c.cst_w2v_negatives(1, 2, 2, 1, 0, None, None) == -1 and b"null operand" in last()

    def vq(N=4, G=2, V=8, d=8, dtype=0, vars_=A):
        return c.cst_gumbel_vq_fwd(A, vars_, None, 1, 1, A, A, A, A, A, A, A, N, G, V, d, dtype, None)
    for kw, msg in ((dict(V=1025), b"exceed the supported"), (dict(d=12), b"multiple of 8"), (dict(d=0), b"multiple of 8"), (dict(dtype=9), b"bad dtype"),
                    (dict(N=0), b"bad shape"), (dict(G=0), b"bad shape"), (dict(vars_=None), b"null operand"), (dict(vars_=A + 8), b"aligned")):
        assert vq(**kw) == -1 and msg in last(), kw
    assert c.cst_gumbel_vq_bwd(A, None, 1, 0.0, A, A, A, A, A, 4, 2, 8, 0, None) == -1 and b"positive" in last()
    assert c.cst_gumbel_vq_bwd(A, None, 1, 1.0, A, A, A, A, A, 4, 2, 4096, 0, None) == -1 and b"exceed the supported" in last()
    assert c.cst_gumbel_vq_bwd(A, None, 1, 1.0, None, A, A, A, A, 4, 2, 8, 0, None) == -1 and b"null operand" in last()
    assert c.cst_gumbel_vq_workspace(67, 2, 320) == 3 * 2 * 320 * 8 and c.cst_gumbel_vq_workspace(0, 2, 8) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_head_fails_loudly_on_cpu_tensors(lib):
    CF = import_module("chimera-st_amd.functional")
    x, y = torch.randn(6, 16), torch.randn(6, 16)
    idx = torch.zeros(6, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback|not on the GPU|No HIP GPUs"):
        CF.infonce_loss(x, y, idx, 0.1)


def test_wrapper_checks_shapes_on_the_host(lib):
    K = import_module("chimera-st_amd.kernels")
    x, y = torch.randn(6, 16), torch.randn(6, 16)
    with pytest.raises(ValueError, match="idx must be int32"):
        K.infonce_fwd(x, y, torch.zeros(6, 3, dtype=torch.int64), 10.0)
    with pytest.raises(ValueError, match="one dtype"):
        K.infonce_fwd(x, y.bfloat16(), torch.zeros(6, 3, dtype=torch.int32), 10.0)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        K.infonce_fwd(x, torch.randn(5, 16), torch.zeros(6, 3, dtype=torch.int32), 10.0)


def test_quantizer_module_keeps_the_checkpoint_layout():
    """The working quantizer has the inert one's parameter names, shapes and order (tests/golden/w2v_quant_tiny.pt loads strictly through
    the model elsewhere), reads --latent-temp as the reference writes it, and follows set_num_updates."""
    W = import_module("chimera-st_amd.wav2vec2")
    m = W.GumbelVectorQuantizer(32, 8, 2, 16, temp=W._latent_temp(type("A", (), {"latent_temp": "(2,0.5,0.999995)"})()))
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [("vars", (1, 16, 8)), ("weight_proj.weight", (16, 32)), ("weight_proj.bias", (16,))]
    assert (m.max_temp, m.min_temp, m.temp_decay, m.curr_temp) == (2.0, 0.5, 0.999995, 2.0)
    m.set_num_updates(100000)
    assert m.curr_temp == max(2.0 * 0.999995 ** 100000, 0.5)
    assert W._latent_temp(type("A", (), {})()) == (2.0, 0.5, 0.999995)
    assert float(m.vars.detach().min()) >= 0.0 and float(m.vars.detach().max()) <= 1.0 and float(m.weight_proj.bias.detach().abs().max()) == 0.0


# ---- model, criterion and task layers ----
def tiny_args(**over):
    import argparse
    from argparse import Namespace
    torch.serialization.add_safe_globals([argparse.Namespace])
    a = torch.load(os.path.join(ROOT, "tests", "golden", "w2v_quant_tiny.pt"), map_location="cpu")["args"]
    return Namespace(**{**vars(a), **over})


def test_registry_flags_and_defaults():
    import argparse
    load_pkg()
    reg, W = import_module("chimera-st_amd.registry"), import_module("chimera-st_amd.wav2vec2")
    C = import_module("chimera-st_amd.criterions")
    assert reg.CRITERION_REGISTRY["wav2vec"] is C.Wav2vecCriterion and reg.MODEL_REGISTRY["wav2vec2"] is W.Wav2Vec2Model
    p = argparse.ArgumentParser()
    W.Wav2Vec2Model.add_args(p)
    C.Wav2vecCriterion.add_args(p)
    a = p.parse_args(["--infonce", "--loss-weights", "[0.1, 10]", "--log-keys", '["temp"]', "--quantize-targets", "--final-dim", "256",
                      "--latent-vars", "320", "--latent-groups", "2", "--latent-temp", "(2,0.5,0.999995)", "--mask-prob", "0.65",
                      "--mask-length", "10", "--num-negatives", "100", "--feature-grad-mult", "0.1", "--encoder-layerdrop", "0.05",
                      "--dropout-input", "0.1", "--dropout-features", "0.1"])
    assert a.infonce and a.quantize_targets and a.final_dim == 256 and a.num_negatives == 100 and not hasattr(a, "cross_sample_negatives")
    W.base_architecture(a)
    assert (a.num_negatives, a.cross_sample_negatives, a.codebook_negatives, a.negatives_from_everywhere) == (100, 0, 0, False)
    assert a.latent_temp == "(2,0.5,0.999995)" and a.mask_prob == 0.65 and a.mask_selection == "static" and a.mask_channel_prob == 0
    b = argparse.Namespace()
    W.base_architecture(b)
    assert b.num_negatives == 100 and b.latent_temp == "(2,0.5,0.999995)" and b.mask_length == 10 and b.encoder_layers == 12


def test_the_five_refusals_name_their_flag():
    load_pkg()
    W, C = import_module("chimera-st_amd.wav2vec2"), import_module("chimera-st_amd.criterions")
    for over, flag in ((dict(quantize_input=True), "--quantize-input"), (dict(target_glu=True, criterion="wav2vec"), "--target-glu"),
                       (dict(negatives_from_everywhere=True), "--negatives-from-everywhere"), (dict(codebook_negatives=3), "--codebook-negatives")):
        with pytest.raises(NotImplementedError, match=flag):
            W.Wav2Vec2Model.build_model(tiny_args(**over))
    with pytest.raises(NotImplementedError, match="--infonce"):
        C.Wav2vecCriterion.build_criterion(argparse_ns(infonce=False), None)
    crit = C.Wav2vecCriterion.build_criterion(argparse_ns(infonce=True, loss_weights="[0.1, 10]", log_keys='["temp"]'), None)
    assert crit.loss_weights == [0.1, 10.0] and crit.log_keys == ["temp"]
    assert set(crit.logging_keys()) == {"loss", "loss_0", "loss_1", "loss_2", "ntokens", "nsentences", "sample_size", "correct", "count", "temp"}


def argparse_ns(**kw):
    from argparse import Namespace
    return Namespace(**kw)


def test_model_keeps_the_checkpoint_layout_and_loads_it_strictly():
    import argparse
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    torch.serialization.add_safe_globals([argparse.Namespace])
    ck = torch.load(os.path.join(ROOT, "tests", "golden", "w2v_quant_tiny.pt"), map_location="cpu")
    model = W.Wav2Vec2Model.build_model(tiny_args(criterion="wav2vec"))
    assert list(model.state_dict().keys()) == list(ck["model"].keys())
    model.load_state_dict(ck["model"], strict=True)
    assert [k for k, _ in model.named_parameters()] == [k for k in ck["model"]]  # (no buffers: the optimizer's index space is the file's)
    model.set_num_updates(1000)
    assert model.quantizer.curr_temp == 2.0 * 0.999995 ** 1000
    assert len(model.get_extra_losses({"prob_perplexity": torch.tensor(3.0), "num_vars": 16, "features_pen": torch.tensor(1.0)})) == 2


def test_reduce_metrics():
    import math
    load_pkg()
    C = import_module("chimera-st_amd.criterions")
    logs = [dict(loss=40.0, loss_0=30.0, loss_1=6.0, loss_2=4.0, ntokens=20, nsentences=2, sample_size=20, correct=5, count=20, temp=2.0,
                 prob_perplexity=10.0),
            dict(loss=20.0, loss_0=15.0, loss_1=3.0, loss_2=2.0, ntokens=10, nsentences=1, sample_size=10, correct=4, count=10, temp=1.0,
                 prob_perplexity=12.0)]
    m = C.Wav2vecCriterion.reduce_metrics(logs)
    assert m["loss"] == pytest.approx(60.0 / 30 / math.log(2)) and m["accuracy"] == round(9 / 30, 5) and m["nsentences"] == 3
    assert m["loss_0"] == pytest.approx((45.0 / 2) / 30 / math.log(2)) and m["temp"] == 1.5 and m["prob_perplexity"] == 11.0
    assert not C.Wav2vecCriterion.logging_outputs_can_be_summed()
    d = C.Wav2vecCriterion.derived_metrics(dict(correct=9.0, count=30.0, sample_size=30.0, loss_1=9.0, loss=60.0))
    assert d["accuracy"] == 0.3 and d["loss_1"] == pytest.approx(9.0 / 30 / math.log(2)) and "loss" not in d


def test_label_free_dataset_crops_to_the_shortest_with_seeded_draws(tmp_path):
    import numpy as np
    from argparse import Namespace
    import wav2vec_ctc_util as U
    load_pkg()
    T = import_module("chimera-st_amd.tasks")
    rows = U.write_manifest(str(tmp_path), U.fixture())
    args = Namespace(data=str(tmp_path), labels=None, criterion="wav2vec", sample_rate=16000, normalize=False, max_sample_size=3000,
                     min_sample_size=2500, enable_padding=False)
    task = T.AudioPretrainingTask.setup_task(args)
    assert task.target_dictionary is None
    ds = task.load_dataset("train")
    kept = [r for r in rows["train"] if r[1] >= 2500]
    assert len(ds) == len(kept) and ds.labels is None and not ds.pad
    items = [ds[i] for i in range(len(ds))]
    size = min(min(len(it["source"]) for it in items), 3000)
    np.random.seed(3)
    a = task.load_dataset("train").collater(items)  # (the crop generator is seeded from numpy's when the dataset is built)
    np.random.seed(3)
    b = task.load_dataset("train").collater(items)
    np.random.seed(4)
    c = task.load_dataset("train").collater(items)
    assert not torch.equal(a["net_input"]["source"], c["net_input"]["source"])
    assert set(a) == {"id", "net_input"} and set(a["net_input"]) == {"source"} and a["net_input"]["source"].shape == (len(items), size)
    assert torch.equal(a["net_input"]["source"], b["net_input"]["source"])
    for it, row in zip(items, a["net_input"]["source"]):  # every row is a contiguous stretch of its utterance
        src = it["source"]
        starts = (src.unfold(0, size, 1) == row).all(1).nonzero()
        assert len(starts) >= 1
    with pytest.raises(NotImplementedError, match="--enable-padding"):
        T.AudioPretrainingTask.setup_task(Namespace(**{**vars(args), "enable_padding": True}))
    with pytest.raises(NotImplementedError, match="wav2vec2 pre-training is not built"):
        T.AudioPretrainingTask.setup_task(Namespace(data=str(tmp_path), labels=None))
