"""Shared by tests/test_interactive_cpu.py and tests/test_interactive_gpu.py: the tasks of the fixture interactive_tiny.npz
(tools/ref_harness/make_interactive_goldens.py) rebuilt in this package, the fixture's hypotheses as the generator returns them, and the
comparison of printed lines."""
import ast
import os
import shutil
from argparse import Namespace
from importlib import import_module

import torch

from conftest import GOLDEN, load_pkg

load_pkg()
cli = import_module("chimera-st_amd.cli")
tasks = import_module("chimera-st_amd.tasks")
Dictionary = import_module("chimera-st_amd.dictionary").Dictionary

VOCAB = 60
DATA_TINY = os.path.join(GOLDEN, "data_tiny")
MT_ROOT = os.path.join(GOLDEN, "translation_tiny")


def word_dictionary():
    """The tiny fixtures' dictionary: 4 specials + w0 .. w55."""
    d = Dictionary()
    for i in range(VOCAB - 4):
        d.add_symbol("w%d" % i)
    assert len(d) == VOCAB and (d.pad(), d.eos(), d.unk()) == (1, 2, 3)
    return d


def lm_task():
    args = Namespace(data=None, sample_break_mode="eos", tokens_per_sample=1024, max_target_positions=1024, dataset_impl=None)
    return tasks.LanguageModelingTask.setup_task(args, dictionary=word_dictionary())


def speech_data_dir(root):
    """data_tiny relocated (the YAML's audio root resolved) with its dictionary padded to the fixture models' 60 symbols."""
    os.makedirs(root, exist_ok=True)
    for f in os.listdir(DATA_TINY):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(DATA_TINY, f), os.path.join(root, f))
    cfg = os.path.join(root, "config_wave.yaml")
    text = open(cfg).read().replace("AUDIO_ROOT", DATA_TINY)
    open(cfg, "w").write(text)
    words = open(os.path.join(root, "dict.txt")).read().splitlines()
    words += ["filler%d 1" % i for i in range(VOCAB - 4 - len(words))]
    open(os.path.join(root, "dict.txt"), "w").write("\n".join(words) + "\n")
    return str(root)


def speech_task(root, kind="triplet"):
    args = Namespace(data=speech_data_dir(root), config_yaml="config_wave.yaml", max_source_positions=2000000, max_target_positions=1024,
                     sample_rate=16000, normalize=False, seed=1)
    return (tasks.TripletTask if kind == "triplet" else tasks.SpeechToTextTask).setup_task(args)


def mt_task():
    args = Namespace(data=MT_ROOT, source_lang=None, target_lang=None, left_pad_source="True", left_pad_target="False",
                     max_source_positions=1024, max_target_positions=1024, dataset_impl="mmap", seed=1)
    return tasks.TranslationTask.setup_task(args)


def batch_args(**kw):
    a = Namespace(constraints=None, max_tokens=None, batch_size=None, skip_invalid_size_inputs_valid_test=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def fixture_hyps(g, key):
    """The hypotheses under `key` (.../batch<j>) as the generator returns them: per sentence a list of dicts, best first."""
    out, b = [], 0
    while "%s/b%d/n" % (key, b) in g:
        out.append([{"tokens": torch.from_numpy(g["%s/b%d/r%d/tokens" % (key, b, r)]), "score": torch.tensor(g["%s/b%d/r%d/score" % (key, b, r)]),
                     "positional_scores": torch.from_numpy(g["%s/b%d/r%d/pos_scores" % (key, b, r)]), "attention": None, "alignment": None}
                    for r in range(int(g["%s/b%d/n" % (key, b)]))])
        b += 1
    return out


def buffers(g, key):
    """[(buffer index, [batch keys])] of a recorded run."""
    return [(k, ["%s/buffer%d/batch%d" % (key, k, j) for j in range(int(g["%s/buffer%d/nbatches" % (key, k)]))])
            for k in range(int(g["%s/nbuffers" % key]))]


def lm_settings(g):
    return ast.literal_eval(str(g["meta/lm_settings"]))


def split_line(line):
    """(prefix and id, the numeric fields, the text fields) of an output line."""
    f = line.split("\t")
    tag = f[0][:2]
    if tag in ("H-", "D-"):
        return f[0], [float(f[1])], f[2:]
    if tag == "P-":
        return f[0], [float(x) for x in f[1].split()], []
    if tag == "W-":
        return f[0], [], f[2:]  # (the time itself is the run's)
    return f[0], [], f[1:]
