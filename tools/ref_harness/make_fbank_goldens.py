#!/usr/bin/env python3
"""Golden fixture of the filter-bank input route: a tiny manifest root (tests/golden/fbank_tiny/: six 16-bit PCM WAV utterances,
the restatement's features of each as .npy files, the same .npy files packed into a stored zip as the reference's prep packs
fbank80.zip, TSV manifests over the three, data-config YAMLs, global CMVN stats and a dictionary — all synthetic, generated
HERE) is read by the REAL reference (TripletDatasetCreator.from_tsv, __getitem__ with its feature transforms, the collater)
under a seeded np.random, and the results are stored in tests/golden/fbank_pipeline_tiny.npz:
  <config>/<manifest>/{id, src_tokens, src_lengths}   the collated batch of all utterances, __getitem__ called in index order
  <config>/<manifest>/draws, draws_len                 the np.random.randint results of each __getitem__ (SpecAugment's draws)
On the .wav manifest the reference's get_fbank calls torchaudio, which is absent here: stubs/torchaudio delegates to
tests/fbank_ref.py.  That part of the fixture pins the reference's glue (scaling, transform order, draws, padding, order), not
the filter-bank numerics.

Run in the build container only:  python tools/ref_harness/make_fbank_goldens.py"""
import os
import sys
import tempfile
import wave
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "tests")))
import fbank_ref  # noqa: E402
from ref_import import import_reference  # noqa: E402

ROOT = os.path.abspath(os.path.join(HERE, "..", "..", "tests", "golden", "fbank_tiny"))
OUT = os.path.abspath(os.path.join(HERE, "..", "..", "tests", "golden", "fbank_pipeline_tiny.npz"))
LENS = [4000, 4100, 2500, 6000, 1200, 3170]  # 4000 and 4100 samples both give 23 frames
WORDS = ["▁the", "▁a", "▁cat", "▁dog", "s", "▁sat", "▁on", "▁mat", "ing", "▁run", "▁und", "▁der", "▁die", "▁haus", "▁ist"]
LB = ("specaugment:\n  freq_mask_F: 27\n  freq_mask_N: 1\n  time_mask_N: 1\n  time_mask_T: 100\n  time_mask_p: 1.0\n"
      "  time_warp_W: 0\n")
CONFIGS = {
    "prep": "transforms:\n  _train:\n  - specaugment\n" + LB,
    "ucmvn_sa": "transforms:\n  _train:\n  - utterance_cmvn\n  - specaugment\n" + LB,
    "gcmvn_sa": "global_cmvn:\n  stats_npz_path: AUDIO_ROOT/gcmvn.npz\ntransforms:\n  _train:\n  - global_cmvn\n  - specaugment\n" + LB,
}
RUNS = [("prep", "zip"), ("ucmvn_sa", "npy"), ("ucmvn_sa", "zip"), ("ucmvn_sa", "wav"), ("gcmvn_sa", "npy"), ("gcmvn_sa", "wav")]


def make_root():
    os.makedirs(ROOT, exist_ok=True)
    rng = np.random.RandomState(17)
    t = np.arange(max(LENS)) / 16000.0
    feats = {}
    for i, n in enumerate(LENS):
        if i % 2 == 0:
            x = rng.randn(n) * (800 + 1500 * i)
        else:
            x = 6000 * np.sin(2 * np.pi * (300 + 700 * i) * t[:n]) + rng.randn(n) * 200
        x = np.round(x).clip(-32768, 32767).astype("<i2")
        with wave.open(os.path.join(ROOT, "utt%d.wav" % i), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(x.tobytes())
        feats[i] = fbank_ref.fbank(x.astype(np.float64) / 32768.0).astype(np.float32)
        np.save(os.path.join(ROOT, "utt%d.npy" % i), feats[i])
    zpath = os.path.join(ROOT, "fbank80.zip")
    with zipfile.ZipFile(zpath, "w", zipfile.ZIP_STORED) as z:
        for i in range(len(LENS)):
            z.write(os.path.join(ROOT, "utt%d.npy" % i), "utt%d.npy" % i)
    with zipfile.ZipFile(zpath) as z:  # chimera/prepare_data/data_utils.py get_zip_manifest
        zman = {os.path.splitext(i.filename)[0]: "fbank80.zip:%d:%d" % (i.header_offset + 30 + len(i.filename), i.file_size)
                for i in z.infolist()}
    allf = np.concatenate(list(feats.values()))
    np.savez(os.path.join(ROOT, "gcmvn.npz"), mean=allf.mean(axis=0), std=allf.std(axis=0))
    with open(os.path.join(ROOT, "dict.txt"), "w", encoding="utf-8") as f:
        for i, wd in enumerate(WORDS):
            f.write("%s %d\n" % (wd, 100 - i))
    r = np.random.RandomState(5)
    rows = []
    for i, n in enumerate(LENS):
        tgt = " ".join(r.choice(WORDS[9:], size=r.randint(2, 6)))
        src = " ".join(r.choice(WORDS[:9], size=r.randint(2, 6)))
        rows.append(("utt%d" % i, n, tgt, src))
    for kind in ("npy", "zip", "wav"):
        with open(os.path.join(ROOT, "train_%s.tsv" % kind), "w", encoding="utf-8") as f:
            f.write("id\taudio\tn_frames\ttgt_text\tsrc_text\tspeaker\n")
            for uid, n, tgt, src in rows:
                audio = zman[uid] if kind == "zip" else "%s.%s" % (uid, kind)
                f.write("\t".join((uid, audio, str(fbank_ref.n_frames(n)), tgt, src, "spk0")) + "\n")
    for name, body in CONFIGS.items():
        with open(os.path.join(ROOT, "config_%s.yaml" % name), "w") as f:
            f.write("audio_root: AUDIO_ROOT\nbpe_tokenizer:\n  bpe: null\nsrc_bpe_tokenizer:\n  bpe: null\ninput_channels: 1\n"
                    "input_feat_per_channel: 80\nsampling_alpha: 1.0\nsrc_vocab_filename: dict.txt\nuse_audio_input: false\n"
                    "vocab_filename: dict.txt\n" + body)


def main():
    make_root()
    import_reference()
    from fairseq.data import Dictionary
    from fairseq.data.audio.triplet_dataset import TripletDataConfig, TripletDatasetCreator

    tmp = tempfile.mkdtemp()
    d = Dictionary.load(os.path.join(ROOT, "dict.txt"))
    out = {}
    orig = np.random.randint
    for cfg_name, kind in RUNS:
        # the committed YAML carries a placeholder root (the fixture is relocatable); resolve it in a temp copy
        cfg_path = os.path.join(tmp, "config_%s.yaml" % cfg_name)
        open(cfg_path, "w").write(open(os.path.join(ROOT, "config_%s.yaml" % cfg_name)).read().replace("AUDIO_ROOT", ROOT))
        cfg = TripletDataConfig(cfg_path)
        ds = TripletDatasetCreator.from_tsv(ROOT, cfg, "train_" + kind, d, d, None, None, None, is_train_split=True, epoch=1, seed=1)
        draws = []

        def rec(*a, **k):
            v = orig(*a, **k)
            draws[-1].append(int(v))
            return v
        np.random.seed(1)
        np.random.randint = rec
        try:
            items = []
            for i in range(len(ds)):
                draws.append([])
                items.append(ds[i])
        finally:
            np.random.randint = orig
        s = ds.collater(items)
        key = "%s/%s/" % (cfg_name, kind)
        out[key + "id"] = s["id"].numpy()
        out[key + "src_tokens"] = s["net_input"]["src_tokens"].numpy()
        out[key + "src_lengths"] = s["net_input"]["src_lengths"].numpy()
        out[key + "draws"] = np.array(sum(draws, []), dtype=np.int64)
        out[key + "draws_len"] = np.array([len(x) for x in draws], dtype=np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
