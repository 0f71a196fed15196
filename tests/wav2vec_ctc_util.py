"""Shared by test_wav2vec_ctc_cpu.py / test_wav2vec_ctc_gpu.py: the tiny wav2vec_ctc model over tests/golden/w2v_quant_tiny.pt as the
fixture tests/golden/ctc_tiny.npz (tools/ref_harness/make_ctc_goldens.py, the real reference) builds it, and a manifest of WAV files."""
import os
import wave
from argparse import Namespace
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import torch

from conftest import GOLDEN, load_golden, load_pkg

W2V = os.path.join(GOLDEN, "w2v_quant_tiny.pt")


def fixture():
    return load_golden("ctc_tiny.npz")


def letter_dictionary(g):
    load_pkg()
    d = import_module("chimera-st_amd.dictionary").Dictionary()
    for c in str(g["meta/dict"]):
        d.add_symbol(c)
    return d


def build_model(g, **over):
    """Wav2VecCtc as the fixture's: no dropout, no masking, feature_grad_mult of the pre-trained file (0.1), the fixture's projection."""
    A = import_module("chimera-st_amd.wav2vec2_asr")
    args = Namespace(w2v_path=W2V, feature_grad_mult=0.1, normalize=False, **over)
    task = SimpleNamespace(target_dictionary=letter_dictionary(g))
    model = A.Wav2VecCtc.build_model(args, task)
    with torch.no_grad():
        model.w2v_encoder.proj.weight.copy_(torch.from_numpy(g["param/w2v_encoder.proj.weight"]))
        model.w2v_encoder.proj.bias.copy_(torch.from_numpy(g["param/w2v_encoder.proj.bias"]))
    return model, task, args


def fixture_sample(g):
    tl = torch.from_numpy(g["in/target_lengths"])
    return {"id": torch.arange(len(tl)), "net_input": {"source": torch.from_numpy(g["in/source"]), "padding_mask": torch.from_numpy(g["in/padding_mask"])},
            "target": torch.from_numpy(g["in/target"]), "target_lengths": tl, "ntokens": int(tl.sum())}


def to_cuda(s):
    if torch.is_tensor(s):
        return s.cuda()
    if isinstance(s, dict):
        return {k: to_cuda(v) for k, v in s.items()}
    return s


def write_manifest(root, g, splits=(("train", 6), ("valid", 3)), seed=9):
    """<root>/<split>.tsv, <root>/<split>.ltr, <root>/dict.ltr.txt and 16-bit PCM WAV files written with the `wave` module.
    Returns {split: [(relpath, nsamples, label line)]}."""
    rng = np.random.RandomState(seed)
    letters = str(g["meta/dict"])
    os.makedirs(os.path.join(root, "audio"), exist_ok=True)
    with open(os.path.join(root, "dict.ltr.txt"), "w") as f:
        for i, c in enumerate(letters):
            f.write("%s %d\n" % (c, 100 - i))
    out = {}
    for split, n in splits:
        rows = []
        for i in range(n):
            ns = int(rng.randint(2400, 4400))
            pcm = (rng.randn(ns) * 3000).clip(-32768, 32767).astype("<i2")
            rel = os.path.join("audio", "%s_%d.wav" % (split, i))
            with wave.open(os.path.join(root, rel), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(pcm.tobytes())
            words = ["".join(letters[1 + rng.randint(len(letters) - 1)] for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 4))]
            label = " ".join(" ".join(w) + " |" for w in words)
            rows.append((rel, ns, label, pcm))
        with open(os.path.join(root, split + ".tsv"), "w") as f:
            f.write(str(root) + "\n")
            for rel, ns, _, _ in rows:
                f.write("%s\t%d\n" % (rel, ns))
        with open(os.path.join(root, split + ".ltr"), "w") as f:
            for _, _, label, _ in rows:
                f.write(label + "\n")
        out[split] = rows
    return out


def oracle_cfg(g):
    """The oracle's configuration of the tiny wav2vec2 under the fixture's model (tests/golden/w2v_quant_tiny.pt's arguments)."""
    import argparse
    torch.serialization.add_safe_globals([argparse.Namespace])
    a = torch.load(W2V, map_location="cpu")["args"]
    return dict(conv_layers=eval(a.conv_feature_layers), conv_pos=a.conv_pos, conv_pos_groups=a.conv_pos_groups, w2v_layers=a.encoder_layers,
                w2v_heads=a.encoder_attention_heads, feature_grad_mult=a.feature_grad_mult)


def ctc_oracle(p, sample, cfg):
    """Wav2VecCtc + CtcCriterion restated on the oracle's wav2vec2 feature path (CPU): features -> projection -> time-major logits ->
    F.ctc_loss on the fp32 log-softmax, reduction sum, blank = bos = 0, pad = 1.  With oracle.STORAGE set, every tensor the HIP path
    stores is rounded as the oracle rounds it (the projection's output included)."""
    from oracle import chimera_oracle as O
    ni = sample["net_input"]
    x, pm, _ = O.w2v2_extract_features(p, "w2v_encoder.w2v_model.", ni["source"], ni["padding_mask"], cfg)
    logits = O.linear(x, p["w2v_encoder.proj.weight"], p["w2v_encoder.proj.bias"]).transpose(0, 1)
    in_len = (~pm).long().sum(-1)
    t = sample["target"]
    nll = torch.nn.functional.ctc_loss(torch.log_softmax(logits.float(), -1), t[t != 1], in_len, sample["target_lengths"], blank=0,
                                       reduction="none")
    return {"loss": nll.sum(), "nll": nll, "logits": logits, "padding_mask": pm}


def full_state_dict(g):
    """The fixture model's state dict on the CPU: the pre-trained file's wav2vec2 weights (heads dropped) and the fixture's projection."""
    import argparse
    torch.serialization.add_safe_globals([argparse.Namespace])
    keys = str(g["meta/keys"]).split("\n")
    ck = torch.load(W2V, map_location="cpu")
    sd = {"w2v_encoder.w2v_model." + k: v for k, v in ck["model"].items() if "w2v_encoder.w2v_model." + k in keys}
    sd.update({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return {k: sd[k] for k in keys}
