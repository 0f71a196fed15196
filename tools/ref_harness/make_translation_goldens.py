#!/usr/bin/env python3
"""Golden fixtures of the `translation` task (the MT pre-training stage, chimera/scripts/train-en2any-MT.sh), made by the REAL reference:

  tests/golden/translation_tiny/      a synthetic parallel corpus (written HERE: ~25 train / 8 valid / 6 test pairs over the 56 words of
                                      the tiny fixtures' dictionary) binarised by the reference's fairseq_cli/preprocess.py with a joint
                                      dictionary: {train,valid,test}.en-de.{en,de}.{bin,idx} (uint16 streams), dict.{en,de}.txt, and one
                                      more split `valid32` written through the reference's MMapIndexedDatasetBuilder with
                                      vocab_size=None (int32 streams); the text itself is kept beside them (corpus/*.txt)
  tests/golden/translation_tiny.npz   what the reference's TranslationTask / LanguagePairDataset / EpochBatchIterator make of it: the
                                      inferred pair, sizes, ordered_indices under a seed, the size filter, --max-tokens batches, epoch
                                      shuffles for 1 and 2 shards, every collated batch of one epoch under default padding, three batches
                                      under the other left-pad combinations and --required-seq-len-multiple 8 — and the reference
                                      SequenceGenerator's finalised hypotheses (beam 5, max_len_a 1.2, max_len_b 10: the script's
                                      --eval-bleu-args) of the chimera_tiny.npz model fed the valid split's TEXT batches.

Build container only:   python tools/ref_harness/make_translation_goldens.py
The fixtures hold data only (what the reference's programs wrote and computed), never reference source."""
import os
import shutil
import sys
import tempfile
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.abspath(os.path.join(HERE, "..", "..", "tests", "golden"))
ROOT = os.path.join(GOLDEN, "translation_tiny")
OUT = os.path.join(GOLDEN, "translation_tiny.npz")
SRC, TGT = "en", "de"
WORDS = ["w%d" % i for i in range(56)]   # the tiny fixtures' dictionary: 4 specials + 56 words = 60 symbols
LIMIT = (20, 20)                         # the position limit the tests filter with
MAX_TOKENS = 40
GEN = dict(beam_size=5, max_len_a=1.2, max_len_b=10)


def make_corpus(tmp):
    """{split: ([source lines], [target lines])}; the special cases: a one-word sentence, an empty line (eos alone once binarised),
    out-of-vocabulary words, runs of equal source lengths (sort ties), one pair beyond LIMIT."""
    r = np.random.RandomState(5)

    def line(n, oov=False):
        ws = list(r.choice(WORDS, size=n))
        if oov and n:
            ws[int(r.randint(0, n))] = "zzz%d" % r.randint(0, 9)
        return " ".join(ws)

    splits = {}
    for split, n in (("train", 25), ("valid", 8), ("test", 6)):
        src, tgt = [], []
        for i in range(n):
            ls = int(r.randint(2, 13)) if i % 4 else 6  # every fourth source has 5 words + eos: ties
            lt = int(r.randint(2, 13))
            src.append(line(ls, oov=(i % 7 == 3)))
            tgt.append(line(lt, oov=(i % 5 == 2)))
        src[1], tgt[1] = line(1), line(3)       # a one-word sentence
        src[2], tgt[2] = "", line(2)            # an empty source line
        if split == "train":
            src[5], tgt[5] = line(27), line(24)  # beyond LIMIT on both sides
            src[9], tgt[9] = line(4), line(23)   # beyond LIMIT on the target side only
        splits[split] = (src, tgt)
    text = os.path.join(ROOT, "corpus")
    os.makedirs(text, exist_ok=True)
    for split, (src, tgt) in splits.items():
        for lang, lines in ((SRC, src), (TGT, tgt)):
            for d in (tmp, text):
                with open(os.path.join(d, "%s.%s" % (split, lang) + (".txt" if d == text else "")), "w", encoding="utf-8") as f:
                    f.write("".join(l + "\n" for l in lines))
    with open(os.path.join(tmp, "dict.txt"), "w", encoding="utf-8") as f:
        for i, w in enumerate(WORDS):
            f.write("%s %d\n" % (w, 1000 - i))
    return splits


def binarise(tmp):
    """fairseq-preprocess --source-lang en --target-lang de --trainpref .. --validpref .. --testpref .. --srcdict D --tgtdict D (the
    script's own command line, train-en2any-MT.sh:20-26, one worker)."""
    from fairseq import options
    from fairseq_cli import preprocess
    parser = options.get_preprocessing_parser()
    args = parser.parse_args(["--source-lang", SRC, "--target-lang", TGT, "--trainpref", os.path.join(tmp, "train"),
                              "--validpref", os.path.join(tmp, "valid"), "--testpref", os.path.join(tmp, "test"), "--destdir", ROOT,
                              "--thresholdtgt", "0", "--thresholdsrc", "0", "--srcdict", os.path.join(tmp, "dict.txt"),
                              "--tgtdict", os.path.join(tmp, "dict.txt"), "--workers", "1"])
    preprocess.main(args)
    log = os.path.join(ROOT, "preprocess.log")  # (names the temp directory: not a fixture)
    if os.path.exists(log):
        os.remove(log)


def write_int32_split(d):
    """The valid split once more as `valid32`, through the reference's builder with vocab_size=None: int32 streams."""
    from fairseq.data import indexed_dataset
    for lang in (SRC, TGT):
        ds = indexed_dataset.MMapIndexedDataset(os.path.join(ROOT, "valid.%s-%s.%s" % (SRC, TGT, lang)))
        prefix = os.path.join(ROOT, "valid32.%s-%s.%s" % (SRC, TGT, lang))
        b = indexed_dataset.make_builder(prefix + ".bin", impl="mmap", vocab_size=None)
        for i in range(len(ds)):
            b.add_item(ds[i])
        b.finalize(prefix + ".idx")
        assert indexed_dataset.MMapIndexedDataset(prefix)._index.dtype == np.int32


def task_args(**over):
    a = Namespace(data=ROOT, source_lang=None, target_lang=None, load_alignments=False, left_pad_source="True", left_pad_target="False",
                  max_source_positions=1024, max_target_positions=1024, upsample_primary=1, truncate_source=False, num_batch_buckets=0,
                  dataset_impl="mmap", required_seq_len_multiple=1, eval_bleu=False, train_subset="train", seed=1)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def put_batch(out, key, s):
    out[key + "/id"] = s["id"].numpy()
    out[key + "/ntokens"] = np.int64(s["ntokens"])
    out[key + "/nsentences"] = np.int64(s["nsentences"])
    out[key + "/target"] = s["target"].numpy()
    for k in ("src_tokens", "src_lengths", "prev_output_tokens"):
        out[key + "/" + k] = s["net_input"][k].numpy()


def record_data(out):
    from fairseq.data import data_utils, iterators
    from fairseq.tasks.translation import TranslationTask
    args = task_args()
    task = TranslationTask.setup_task(args)
    out["pair"] = np.array([args.source_lang, args.target_lang])
    out["dict_len"] = np.int64(len(task.source_dictionary))
    for split in ("train", "valid", "test", "valid32"):
        task.load_dataset(split)
        ds = task.dataset(split)
        out[split + "/dtype"] = np.array(str(np.dtype(ds.src._index.dtype)))
        out[split + "/sizes"] = np.asarray(ds.sizes)
        out[split + "/src_flat"] = np.concatenate([ds.src[i].numpy() for i in range(len(ds))])
        out[split + "/tgt_flat"] = np.concatenate([ds.tgt[i].numpy() for i in range(len(ds))])
        with data_utils.numpy_seed(1):
            idx = ds.ordered_indices()
        out[split + "/ordered"] = np.asarray(idx)
        idx_f, ignored = ds.filter_indices_by_size(idx, LIMIT)
        out[split + "/filtered"] = np.asarray(idx_f)
        out[split + "/ignored"] = np.asarray(ignored, dtype=np.int64)
        for tag, kw in (("tok40", dict(max_tokens=MAX_TOKENS)), ("sent3", dict(max_sentences=3)),
                        ("tok64_mult8", dict(max_tokens=64, required_batch_size_multiple=8))):
            batches = ds.batch_by_size(idx_f, **kw)
            out["%s/batches/%s/sizes" % (split, tag)] = np.array([len(b) for b in batches])
            out["%s/batches/%s/flat" % (split, tag)] = np.concatenate([np.asarray(b) for b in batches])
        batches = ds.batch_by_size(idx_f, max_tokens=MAX_TOKENS)
        for num_shards in (1, 2):
            for shard in range(num_shards):
                it = iterators.EpochBatchIterator(ds, ds.collater, batches, seed=1, num_shards=num_shards, shard_id=shard, epoch=1)
                for ep in (1, 2):
                    itr = it.next_epoch_itr(shuffle=(split == "train"))
                    samples = list(itr)
                    ids = [s["id"].numpy() if len(s) else np.zeros(0, dtype=np.int64) for s in samples]
                    out["%s/epoch%d/shards%d/%d/sizes" % (split, ep, num_shards, shard)] = np.array([len(i) for i in ids])
                    out["%s/epoch%d/shards%d/%d/ids" % (split, ep, num_shards, shard)] = np.concatenate(ids)
                    if num_shards == 1 and ep == 1:  # every collated batch of one epoch, default padding
                        out["%s/collated/n" % split] = np.int64(len(samples))
                        for j, s in enumerate(samples):
                            put_batch(out, "%s/collated/%d" % (split, j), s)
    # the other three left-pad combinations, widths padded to a multiple of 8: three train batches each
    for lps, lpt in (("True", "True"), ("False", "False"), ("False", "True")):
        a = task_args(left_pad_source=lps, left_pad_target=lpt, required_seq_len_multiple=8)
        t = TranslationTask.setup_task(a)
        t.load_dataset("train")
        ds = t.dataset("train")
        with data_utils.numpy_seed(1):
            idx = ds.ordered_indices()
        idx_f, _ = ds.filter_indices_by_size(idx, LIMIT)
        batches = ds.batch_by_size(idx_f, max_tokens=MAX_TOKENS)
        for j in (0, len(batches) // 2, len(batches) - 1):
            key = "train/padded/src%s_tgt%s/%d" % (lps, lpt, j)
            out[key + "/batch"] = np.asarray(batches[j])
            put_batch(out, key, ds.collater([ds[int(i)] for i in batches[j]]))
    return task


def record_hypotheses(out, task):
    """The reference SequenceGenerator on the chimera_tiny.npz model, fed the valid split's text batches."""
    import make_goldens as MG
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator
    g = np.load(os.path.join(GOLDEN, "chimera_tiny.npz"), allow_pickle=False)
    d = task.target_dictionary
    assert len(d) == MG.VOCAB
    with tempfile.TemporaryDirectory() as tmp:
        w2v_path = os.path.join(tmp, "w2v_tiny.pt")
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
    out["gen/settings"] = np.array(repr(GEN))
    gen = SequenceGenerator([model], d, **GEN)
    n = int(out["valid/collated/n"])
    for j in range(n):
        key = "valid/collated/%d" % j
        sample = {"net_input": {"src_tokens": torch.from_numpy(out[key + "/src_tokens"]), "src_lengths": torch.from_numpy(out[key + "/src_lengths"])}}
        with torch.no_grad():
            hyps = gen.generate([model], sample)
        for b, h in enumerate(hyps):
            out["gen/%d/b%d/n" % (j, b)] = np.int64(len(h))
            for r, hyp in enumerate(h):
                k = "gen/%d/b%d/r%d/" % (j, b, r)
                out[k + "tokens"] = hyp["tokens"].numpy()
                out[k + "score"] = np.float64(float(hyp["score"]))
                out[k + "pos_scores"] = hyp["positional_scores"].numpy()
            print("batch", j, "sentence", b, "best", h[0]["tokens"].tolist(), "%.4f" % float(h[0]["score"]))


def main():
    if os.path.isdir(ROOT):
        shutil.rmtree(ROOT)
    os.makedirs(ROOT)
    import_reference()
    import make_data_goldens as DG
    tmp = tempfile.mkdtemp()
    DG.build_cython_batcher(tmp)
    make_corpus(tmp)
    binarise(tmp)
    write_int32_split(ROOT)
    out = {}
    task = record_data(out)
    record_hypotheses(out, task)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays;", sorted(os.listdir(ROOT)))


if __name__ == "__main__":
    main()
