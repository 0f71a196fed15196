"""Mirror of the task surface the hot path is called through: fairseq/tasks/fairseq_task.py (build_model :265-281,
build_criterion :283-298, train_step :414-445, valid_step :447-451, inference_step :453-459, build_generator
:309-412), fairseq/tasks/speech_to_text.py (:27-154), fairseq/tasks/triplet.py (:23-241), fairseq/tasks/translation.py (:164-475:
the MT pre-training stage on binarised parallel text, with BLEU during validation) and fairseq/tasks/language_modeling.py (:96-328: the
fusion language model on binarised monolingual text).

Datasets / TSV manifests / audio decoding are a "next" row; this build provides the collater's
`sample` dict layout (data/audio/triplet_dataset.py:220-234) through `synthetic_sample`, the same shapes the
reference batches have: audio sorted by length descending, right-padded; targets with eos; prev_output_tokens
= eos-shifted targets (data/data_utils.py:34-64)."""
import os

import torch

from . import registry
from .dictionary import Dictionary
from .registry import register_task
from .profiling import scope


def collate_tokens(values, pad_idx, eos_idx, left_pad=False, move_eos_to_beginning=False):
    """data/data_utils.py:34-64."""
    size = max(v.size(0) for v in values)
    res = values[0].new(len(values), size).fill_(pad_idx)
    for i, v in enumerate(values):
        dst = res[i][size - len(v):] if left_pad else res[i][:len(v)]
        if move_eos_to_beginning:
            dst[0] = eos_idx
            dst[1:] = v[:-1]
        else:
            dst.copy_(v)
    return res


class FairseqTask:
    def __init__(self, args):
        self.args = args

    @staticmethod
    def add_args(parser):
        pass

    @classmethod
    def setup_task(cls, args, **kwargs):
        return cls(args, **kwargs)

    @property
    def source_dictionary(self):
        return None

    @property
    def target_dictionary(self):
        return None

    def build_model(self, args):
        return registry.build_model(args, self)

    def build_criterion(self, args):
        return registry.build_criterion(args, self)

    def train_step(self, sample, model, criterion, optimizer, update_num, ignore_grad=False):
        """fairseq_task.py:414-445."""
        model.train()
        if hasattr(model, "set_num_updates"):
            model.set_num_updates(update_num)
        if hasattr(criterion, "set_num_updates"):
            criterion.set_num_updates(update_num)
        with scope("forward"):
            loss, sample_size, logging_output = criterion(model, sample)
        if ignore_grad:
            loss = loss * 0
        with scope("backward"):
            optimizer.backward(loss)
        return loss, sample_size, logging_output

    def valid_step(self, sample, model, criterion):
        model.eval()
        with torch.no_grad():
            loss, sample_size, logging_output = criterion(model, sample)
        return loss, sample_size, logging_output

    def inference_step(self, generator, models, sample, prefix_tokens=None, constraints=None):
        with torch.no_grad():
            if constraints is None:
                return generator.generate(models, sample, prefix_tokens=prefix_tokens)
            return generator.generate(models, sample, prefix_tokens=prefix_tokens, constraints=constraints)

    # ---- typed input (fairseq_interactive.py; tasks/fairseq_task.py:289-307, :530-550) -----------------------------
    def get_interactive_tokens_and_lengths(self, lines, encode_fn):
        """fairseq_task.py:542-550: every line encoded, then looked up in the source dictionary (eos appended, no new symbols)."""
        tokens = [self.source_dictionary.encode_line(encode_fn(src_str), add_if_not_exist=False).long() for src_str in lines]
        return tokens, [t.numel() for t in tokens]

    def build_dataset_for_inference(self, src_tokens, src_lengths, **kwargs):
        raise NotImplementedError("task %s has no dataset for typed input" % type(self).__name__)

    def build_tokenizer(self, args):
        """fairseq_task.py:530-532 (--tokenizer): what data.build_tokenizer builds, and refuses."""
        from . import data as D
        return D.build_tokenizer({"tokenizer": getattr(args, "tokenizer", None)})

    def build_bpe(self, args):
        """fairseq_task.py:534-537 (--bpe, --sentencepiece-model)."""
        from . import data as D
        return D.build_bpe({"bpe": getattr(args, "bpe", None), "sentencepiece_model": getattr(args, "sentencepiece_model", None)})

    # ---- datasets (data.py; tasks/fairseq_task.py:162-275) --------------------------------------------------------
    def dataset(self, split):
        if split not in getattr(self, "datasets", {}):
            raise KeyError("Dataset not loaded: " + split)
        return self.datasets[split]

    def max_positions(self):
        return getattr(self.args, "max_source_positions", 6000), getattr(self.args, "max_target_positions", 1024)

    def get_batch_iterator(self, dataset, max_tokens=None, max_sentences=None, max_positions=None, ignore_invalid_inputs=False,
                           required_batch_size_multiple=1, seed=1, num_shards=1, shard_id=0, num_workers=0, epoch=1, **unused):
        from . import data as D
        return D.get_batch_iterator(dataset, max_tokens, max_sentences, max_positions, ignore_invalid_inputs,
                                    required_batch_size_multiple, seed, num_shards, shard_id, epoch)

    def build_generator(self, models, args, seq_gen_cls=None, extra_gen_cls_kwargs=None):
        """fairseq_task.py:309-412: SequenceScorer with --score-reference (:313-320), else beam search, Sampling with --sampling (:329-357), DiverseBeamSearch with --diverse-beam-groups
        (:358-361), DiverseSiblingsSearch with --diversity-rate (:373-376), LexicallyConstrainedBeamSearch with --constraints (:377-380) — the reference's selection: exclusivity is tested with
        `diversity_rate > 0`, the sibling search is chosen with `diversity_rate > -1` (so rate 0 builds it and equals beam search)."""
        from .sequence_generator import (DiverseBeamSearch, DiverseSiblingsSearch, LexicallyConstrainedBeamSearch, Sampling,
                                         SequenceGenerator)

        extra = dict(extra_gen_cls_kwargs or {})  # (lm_model / lm_weight of --lm-path, fairseq_cli/generate.py:171)
        if getattr(args, "score_reference", False):  # (:313-320: before any search strategy is looked at; the search flags go unused)
            from .sequence_scorer import SequenceScorer
            return SequenceScorer(self.target_dictionary)
        sampling = getattr(args, "sampling", False)
        sampling_topk = getattr(args, "sampling_topk", -1)
        sampling_topp = getattr(args, "sampling_topp", -1.0)
        diverse_beam_groups = getattr(args, "diverse_beam_groups", -1)
        diverse_beam_strength = getattr(args, "diverse_beam_strength", 0.5)
        diversity_rate = getattr(args, "diversity_rate", -1.0)
        constrained = getattr(args, "constraints", None) or False  # None | "ordered" | "unordered"
        if sum(int(bool(c)) for c in (sampling, diverse_beam_groups > 0, diversity_rate > 0)) > 1:
            raise ValueError("Provided Search parameters are mutually exclusive.")
        # (the reference's `elif` chain would silently drop --constraints behind another strategy; here the combination is refused)
        if constrained and (sampling or diverse_beam_groups > 0 or diversity_rate > -1):
            raise ValueError("Provided Search parameters are mutually exclusive: --constraints with sampling or a diverse strategy.")
        if constrained and getattr(args, "prefix_size", 0) > 0:
            raise ValueError("--constraints cannot be combined with --prefix-size")
        assert sampling_topk < 0 or sampling, "--sampling-topk requires --sampling"
        assert sampling_topp < 0 or sampling, "--sampling-topp requires --sampling"
        if sampling:
            search = Sampling(self.target_dictionary, sampling_topk, sampling_topp)
        elif diverse_beam_groups > 0:
            search = DiverseBeamSearch(self.target_dictionary, diverse_beam_groups, diverse_beam_strength)
        elif diversity_rate > -1:
            search = DiverseSiblingsSearch(self.target_dictionary, diversity_rate)
        elif constrained:
            search = LexicallyConstrainedBeamSearch(self.target_dictionary, constrained)
        else:
            search = None
        return SequenceGenerator(
            models, self.target_dictionary, beam_size=getattr(args, "beam", 5), max_len_a=getattr(args, "max_len_a", 0),
            max_len_b=getattr(args, "max_len_b", 200), min_len=getattr(args, "min_len", 1),
            normalize_scores=(not getattr(args, "unnormalized", False)), len_penalty=getattr(args, "lenpen", 1),
            unk_penalty=getattr(args, "unkpen", 0), temperature=getattr(args, "temperature", 1.0),
            no_repeat_ngram_size=getattr(args, "no_repeat_ngram_size", 0), search_strategy=search, seed=getattr(args, "seed", 1),
            return_attention=getattr(args, "print_alignment", False), **extra)  # (fairseq_task.py:401-402)


def _load_dict(args, default_size):
    data = getattr(args, "data", None)
    if data:
        for name in (getattr(args, "dict_file", None), "spm_unigram10000_wave_joint.txt", "dict.txt"):
            if name and os.path.exists(os.path.join(data, name)):
                return Dictionary.load(os.path.join(data, name))
    return Dictionary.synthetic(getattr(args, "synthetic_vocab_size", default_size))


@register_task("speech_to_text")
class SpeechToTextTask(FairseqTask):
    """tasks/speech_to_text.py:27-154."""

    @staticmethod
    def add_args(parser):
        parser.add_argument("data", nargs="?", default=None, help="manifest root path")  # tasks/speech_to_text.py:27 (optional here: synthetic data)
        parser.add_argument("--config-yaml", type=str, default="config.yaml")
        parser.add_argument("--normalize", action="store_true")
        parser.add_argument("--max-source-positions", default=6000, type=int, metavar="N")
        parser.add_argument("--max-target-positions", default=1024, type=int, metavar="N")
        parser.add_argument("--synthetic-vocab-size", default=10000, type=int)

    TRIPLET = False

    def __init__(self, args, tgt_dict=None, data_cfg=None):
        super().__init__(args)
        self.data_cfg = data_cfg if data_cfg is not None else self._load_data_cfg(args)
        if tgt_dict is None and self.data_cfg is not None and getattr(args, "data", None) and \
                os.path.isfile(os.path.join(args.data, self.data_cfg.vocab_filename)):
            tgt_dict = Dictionary.load(os.path.join(args.data, self.data_cfg.vocab_filename))  # speech_to_text.py:60-70
        self.tgt_dict = tgt_dict if tgt_dict is not None else _load_dict(args, 10000)
        self.datasets = {}

    @staticmethod
    def _load_data_cfg(args):
        data, name = getattr(args, "data", None), getattr(args, "config_yaml", "config.yaml")
        if data and os.path.isfile(os.path.join(data, name)):
            from . import data as D
            return D.TripletDataConfig(os.path.join(data, name))
        return None

    def load_dataset(self, split, epoch=1, combine=False, **kwargs):
        """tasks/speech_to_text.py:95-111 / tasks/triplet.py:112-132: <data>/<split>.tsv through the data config YAML."""
        from . import data as D
        assert self.data_cfg is not None, "load_dataset needs --data <manifest root> with the --config-yaml file in it"
        self.datasets[split] = D.TripletDatasetCreator.from_tsv(
            self.args.data, self.data_cfg, split, self.tgt_dict, self.source_dictionary if self.TRIPLET else None,
            D.build_tokenizer(self.data_cfg.pre_tokenizer), D.build_bpe(self.data_cfg.bpe_tokenizer),
            D.build_bpe(self.data_cfg.src_bpe_tokenizer) if self.TRIPLET else None, is_train_split=split.startswith("train"),
            epoch=epoch, seed=getattr(self.args, "seed", 1), normalize=getattr(self.args, "normalize", False),
            sample_rate=getattr(self.args, "sample_rate", 16000), triplet=self.TRIPLET)
        return self.datasets[split]

    # ---- typed input: the lines are audio paths (speech_to_text.py:140-154, triplet.py:173-188, :234-241) ----------------------
    def build_tokenizer(self, args):
        from . import data as D
        assert self.data_cfg is not None, "typed input needs --data <manifest root> with the --config-yaml file in it"
        return D.build_tokenizer(self.data_cfg.pre_tokenizer)

    def build_bpe(self, args):
        from . import data as D
        assert self.data_cfg is not None, "typed input needs --data <manifest root> with the --config-yaml file in it"
        return D.build_bpe(self.data_cfg.bpe_tokenizer)

    def get_interactive_tokens_and_lengths(self, lines, encode_fn):
        """(the paths, per path what the dataset's loader will count for it): waveform samples with use_audio_input, filter-bank
        frames of a .wav on the device fbank route, rows of a stored feature matrix.  A missing file raises FileNotFoundError, an
        unreadable or non-PCM one ValueError."""
        from . import data as D
        from . import fbank as FB
        assert self.data_cfg is not None, "typed input needs --data <manifest root> with the --config-yaml file in it"
        wave, rate = self.data_cfg.use_audio_input, getattr(self.args, "sample_rate", 16000)
        n_frames = []
        for p in lines:
            if not wave and D.fbank_audio_entry(p) is not None:
                n_frames.append(FB.num_frames(len(D.get_fbank_audio(p, rate))))
            else:
                n_frames.append(int(D.get_features_or_waveform(p, need_waveform=wave, sample_rate=rate).shape[0]))
        return lines, n_frames

    def build_dataset_for_inference(self, src_tokens, src_lengths, **kwargs):
        from . import data as D
        cls = D.TripletDataset if self.TRIPLET else D.SpeechToTextDataset
        return cls("interactive", False, self.data_cfg, list(src_tokens), list(src_lengths))

    def build_model(self, args):
        if self.data_cfg is not None:  # speech_to_text.py:119-122
            args.input_feat_per_channel = self.data_cfg.input_feat_per_channel
            args.input_channels = self.data_cfg.input_channels
        return super().build_model(args)

    @property
    def target_dictionary(self):
        return self.tgt_dict

    @property
    def source_dictionary(self):
        return None


@register_task("triplet")
class TripletTask(SpeechToTextTask):
    """tasks/triplet.py:23-241 — audio + source text + target text triplets; joint dictionary."""

    @staticmethod
    def add_args(parser):
        SpeechToTextTask.add_args(parser)
        parser.add_argument("--dump-feature-to-file", type=str, default=None)
        parser.add_argument("--sample-rate", type=int, default=16000)

    TRIPLET = True

    def __init__(self, args, tgt_dict=None, src_dict=None, data_cfg=None):
        super().__init__(args, tgt_dict, data_cfg)
        if src_dict is None and self.data_cfg is not None and getattr(args, "data", None) and \
                os.path.isfile(os.path.join(args.data, self.data_cfg.src_vocab_filename)):
            src_dict = Dictionary.load(os.path.join(args.data, self.data_cfg.src_vocab_filename))  # triplet.py:80-95
        self.src_dict = src_dict if src_dict is not None else self.tgt_dict

    @property
    def source_dictionary(self):
        return self.src_dict


def synthetic_sample(dictionary, batch_size, audio_lengths, target_lengths, src_text_lengths=None, seed=1, device="cpu",
                     sort=True):
    """A collater-shaped batch (triplet_dataset.py:165-235) of seeded synthetic data (SURVEY §8d "Synthetic inputs")."""
    g = torch.Generator().manual_seed(seed)
    V, pad, eos = len(dictionary), dictionary.pad(), dictionary.eos()
    order = sorted(range(batch_size), key=lambda i: -audio_lengths[i]) if sort else list(range(batch_size))
    audio_lengths = [audio_lengths[i] for i in order]
    target_lengths = [target_lengths[i] for i in order]
    smax = max(audio_lengths)
    audio = torch.zeros(batch_size, smax)
    for i, s in enumerate(audio_lengths):
        audio[i, :s] = 0.1 * torch.randn(s, generator=g)
    tgt = [torch.cat([torch.randint(4, V, (u,), generator=g), torch.tensor([eos])]) for u in target_lengths]
    sample = {
        "id": torch.arange(batch_size),
        "net_input": {
            "src_tokens": audio.to(device),
            "src_lengths": torch.tensor(audio_lengths, dtype=torch.long, device=device),
            "prev_output_tokens": collate_tokens(tgt, pad, eos, move_eos_to_beginning=True).to(device),
            "mask": False,
        },
        "target": collate_tokens(tgt, pad, eos).to(device),
        "target_lengths": torch.tensor([len(t) for t in tgt], device=device),
        "ntokens": int(sum(len(t) for t in tgt)),
        "nsentences": batch_size,
    }
    if src_text_lengths is not None:
        src_text_lengths = [src_text_lengths[i] for i in order]
        src = [torch.cat([torch.randint(4, V, (l,), generator=g), torch.tensor([eos])]) for l in src_text_lengths]
        sample["src_text"] = collate_tokens(src, pad, eos).to(device)
        sample["src_text_lengths"] = torch.tensor([len(s) for s in src], device=device)
    return sample


def eval_bool(x, default=False):
    """utils.eval_bool: --left-pad-source / --left-pad-target arrive as the strings "True" / "False"."""
    if x is None:
        return default
    if isinstance(x, bool):
        return x
    if str(x) in ("True", "False"):
        return str(x) == "True"
    raise ValueError("expected True or False, got %r" % (x,))


@register_task("translation")
class TranslationTask(FairseqTask):
    """tasks/translation.py:164-475 — parallel text from a binarised directory (indexed_dataset.py, language_pair_dataset.py), and BLEU
    during validation (--eval-bleu, bleu.py).  The MT pre-training stage of the Chimera recipe (chimera/scripts/train-en2any-MT.sh)."""

    @staticmethod
    def add_args(parser):
        """translation.py:187-243, with the two dataset options the reference keeps among its common ones."""
        parser.add_argument("data", help="path to the binarised data directory")
        parser.add_argument("-s", "--source-lang", default=None, metavar="SRC", help="source language")
        parser.add_argument("-t", "--target-lang", default=None, metavar="TARGET", help="target language")
        parser.add_argument("--load-alignments", action="store_true", help="(not built)")
        parser.add_argument("--left-pad-source", default="True", type=str, metavar="BOOL", help="pad the source on the left")
        parser.add_argument("--left-pad-target", default="False", type=str, metavar="BOOL", help="pad the target on the left")
        parser.add_argument("--max-source-positions", default=1024, type=int, metavar="N")
        parser.add_argument("--max-target-positions", default=1024, type=int, metavar="N")
        parser.add_argument("--upsample-primary", default=1, type=int, help="(values other than 1 are not built)")
        parser.add_argument("--truncate-source", action="store_true", default=False, help="(not built)")
        parser.add_argument("--num-batch-buckets", default=0, type=int, metavar="N", help="(values above 0 are not built)")
        parser.add_argument("--dataset-impl", default=None, metavar="FORMAT", help="mmap (the other implementations are not built)")
        parser.add_argument("--required-seq-len-multiple", default=1, type=int, metavar="N", help="pad the batch widths to a multiple of N")
        parser.add_argument("--eval-bleu", action="store_true", help="evaluation with BLEU scores")
        parser.add_argument("--eval-bleu-detok", type=str, default="space", help="detokenize before computing BLEU: space (off) or moses")
        parser.add_argument("--eval-bleu-detok-args", type=str, metavar="JSON", help="args for building the detokenizer, if needed")
        parser.add_argument("--eval-bleu-bpe", type=str, metavar="BPE", default=None, help="sentencepiece")
        parser.add_argument("--eval-bleu-bpe-path", type=str, metavar="BPE", help="the sentencepiece model")
        parser.add_argument("--eval-tokenized-bleu", action="store_true", default=False, help="compute tokenized BLEU (what this build always does)")
        parser.add_argument("--eval-bleu-remove-bpe", nargs="?", const="@@ ", default=None, help="remove BPE before computing BLEU")
        parser.add_argument("--eval-bleu-args", type=str, metavar="JSON", help='generation args for BLEU scoring, e.g. \'{"beam": 4, "lenpen": 0.6}\'')
        parser.add_argument("--eval-bleu-print-samples", action="store_true", help="print sample generations during validation")
        parser.add_argument("--normalize", action="store_true")

    def __init__(self, args, src_dict, tgt_dict):
        super().__init__(args)
        self.src_dict, self.tgt_dict = src_dict, tgt_dict
        self.datasets = {}

    @classmethod
    def setup_task(cls, args, **kwargs):
        """translation.py:250-285."""
        args.left_pad_source = eval_bool(getattr(args, "left_pad_source", "True"), True)
        args.left_pad_target = eval_bool(getattr(args, "left_pad_target", "False"), False)
        data = getattr(args, "data", None)
        if not data:  # a checkpoint whose data directory is not reachable (checkpoint_utils.load_model_ensemble_and_task): ids only
            d = Dictionary.synthetic(getattr(args, "synthetic_vocab_size", 10000))
            return cls(args, d, d)
        from . import language_pair_dataset as P
        paths = P.split_paths(data)
        if len(paths) > 1:
            raise NotImplementedError("several colon-separated data paths (%d given) are not built: the round-robin over data shards of "
                                      "the reference's translation task; pass one directory" % len(paths))
        if getattr(args, "source_lang", None) is None or getattr(args, "target_lang", None) is None:
            args.source_lang, args.target_lang = P.infer_language_pair(paths[0])
        if args.source_lang is None or args.target_lang is None:
            raise Exception("Could not infer language pair, please provide it explicitly")
        src_dict = Dictionary.load(os.path.join(paths[0], "dict.{}.txt".format(args.source_lang)))
        tgt_dict = Dictionary.load(os.path.join(paths[0], "dict.{}.txt".format(args.target_lang)))
        assert src_dict.pad() == tgt_dict.pad()
        assert src_dict.eos() == tgt_dict.eos()
        assert src_dict.unk() == tgt_dict.unk()
        return cls(args, src_dict, tgt_dict)

    def load_dataset(self, split, epoch=1, combine=False, **kwargs):
        """translation.py:287-322.  The split's route of batch assembly (device-resident corpus or host collater) is decided here."""
        from . import language_pair_dataset as P
        a = self.args
        ds = P.load_langpair_dataset(
            a.data, split, a.source_lang, self.src_dict, a.target_lang, self.tgt_dict, combine=combine,
            dataset_impl=getattr(a, "dataset_impl", None), upsample_primary=getattr(a, "upsample_primary", 1),
            left_pad_source=a.left_pad_source, left_pad_target=a.left_pad_target,
            max_source_positions=getattr(a, "max_source_positions", 1024), max_target_positions=getattr(a, "max_target_positions", 1024),
            load_alignments=getattr(a, "load_alignments", False), truncate_source=getattr(a, "truncate_source", False),
            num_buckets=getattr(a, "num_batch_buckets", 0), shuffle=(split != "test"),
            pad_to_multiple=getattr(a, "required_seq_len_multiple", 1))
        ds.enable_resident()
        self.datasets[split] = ds
        return ds

    def build_dataset_for_inference(self, src_tokens, src_lengths, constraints=None):
        """translation.py:324-331: the typed sentences as a pair dataset without targets, with the task's padding sides.  (The batch's
        constraints are packed by the driver, per batch, in the batch's row order: no `constraints` member of the dataset.)"""
        from . import language_pair_dataset as P
        return P.LanguagePairDataset(src_tokens, src_lengths, self.source_dictionary, tgt_dict=self.target_dictionary,
                                     left_pad_source=self.args.left_pad_source, left_pad_target=self.args.left_pad_target)

    def build_model(self, args):
        """translation.py:333-362: with --eval-bleu also the detokeniser, the BPE and the generator of --eval-bleu-args."""
        import json
        import logging
        from argparse import Namespace

        from . import bleu as B
        model = super().build_model(args)
        if getattr(args, "eval_bleu", False):
            log = logging.getLogger(__name__)
            assert getattr(args, "eval_bleu_detok", None) is not None, \
                "--eval-bleu-detok is required if using --eval-bleu; try --eval-bleu-detok=moses (or --eval-bleu-detok=space to disable detokenization)"
            detok_args = json.loads(getattr(args, "eval_bleu_detok_args", None) or "{}")
            self.tokenizer = B.build_detokenizer(args.eval_bleu_detok, log, **detok_args)
            self.bpe = None
            if getattr(args, "eval_bleu_bpe", None) is not None:
                from . import data as D
                self.bpe = D.build_bpe({"bpe": args.eval_bleu_bpe, "sentencepiece_model": getattr(args, "eval_bleu_bpe_path", None)})
            if not getattr(args, "eval_tokenized_bleu", False):
                B.note_once(log, "13a", "--eval-bleu: sacrebleu's 13a tokeniser is not available in this build; BLEU is counted on whitespace "
                            "tokens (as under --eval-tokenized-bleu) and compares between runs of this build only")
            gen_args = json.loads(getattr(args, "eval_bleu_args", None) or "{}")
            self.sequence_generator = self.build_generator([model], Namespace(**gen_args))
        return model

    def decode_for_bleu(self, toks, escape_unk=False):
        """translation.py:436-451: ids -> text: the dictionary's string without the BPE marker, then the BPE's and the detokeniser's
        decode.  The unknown token prints as one word that cannot match between hypothesis and reference."""
        s = self.tgt_dict.string(toks.tolist() if torch.is_tensor(toks) else toks, getattr(self.args, "eval_bleu_remove_bpe", None),
                                 extra_symbols_to_ignore=(self.tgt_dict.bos(),),
                                 unk_string=("UNKNOWNTOKENINREF" if escape_unk else "UNKNOWNTOKENINHYP"))
        if getattr(self, "bpe", None) is not None:
            s = self.bpe.decode(s)
        if getattr(self, "tokenizer", None) is not None:
            s = self.tokenizer.decode(s)
        return s

    def bleu_strings(self, hyp_tokens, target):
        """(hypothesis strings, reference strings) of a batch: hyp_tokens a list of id sequences, target the padded [B, T] batch."""
        pad = self.tgt_dict.pad()
        hyps = [self.decode_for_bleu(h) for h in hyp_tokens]
        refs = [self.decode_for_bleu([t for t in row if t != pad], escape_unk=True) for row in target.tolist()]
        return hyps, refs

    def valid_step(self, sample, model, criterion):
        """translation.py:364-376: the criterion's log plus the batch's BLEU statistics (summed over batches and ranks by cli.validate)."""
        loss, sample_size, logging_output = super().valid_step(sample, model, criterion)
        if getattr(self.args, "eval_bleu", False):
            from . import bleu as B
            gen_out = self.inference_step(self.sequence_generator, [model], sample, prefix_tokens=None)
            hyps, refs = self.bleu_strings([g[0]["tokens"].tolist() for g in gen_out], sample["target"].cpu())
            if getattr(self.args, "eval_bleu_print_samples", False):
                import logging
                logging.getLogger(__name__).info("example hypothesis: " + hyps[0])
                logging.getLogger(__name__).info("example reference: " + refs[0])
            logging_output = dict(logging_output)
            logging_output.update(B.corpus_stats(hyps, refs))
        return loss, sample_size, logging_output

    def derived_metrics(self, summed):
        """`bleu` from the summed statistics (translation.py:378-417)."""
        from . import bleu as B
        return B.derived_bleu(summed) if getattr(self.args, "eval_bleu", False) else {}

    def max_positions(self):
        return (getattr(self.args, "max_source_positions", 1024), getattr(self.args, "max_target_positions", 1024))

    @property
    def source_dictionary(self):
        return self.src_dict

    @property
    def target_dictionary(self):
        return self.tgt_dict


@register_task("audio_pretraining")
class AudioPretrainingTask(FairseqTask):
    """tasks/audio_pretraining.py:36-167 with --labels: fine-tuning wav2vec2 on transcripts (criterion ctc, arch wav2vec_ctc).
    <data>/<split>.tsv is the wav2vec manifest, <data>/<split>.<labels> holds one label line per utterance and
    <data>/dict.<labels>.txt the target dictionary.  Without --labels and with --criterion wav2vec it pre-trains wav2vec2 on the manifest alone (cropped batches)."""

    @staticmethod
    def add_args(parser):
        parser.add_argument("data", help="path to data directory")
        parser.add_argument("--sample-rate", default=16000, type=int)
        parser.add_argument("--normalize", action="store_true", help="if set, normalizes input to have 0 mean and unit variance")
        parser.add_argument("--max-sample-size", default=None, type=int)
        parser.add_argument("--min-sample-size", default=None, type=int)
        parser.add_argument("--enable-padding", action="store_true", help="pad shorter samples instead of cropping")
        parser.add_argument("--labels", type=str, default=None, help="extension of the label file to load, if any")

    def __init__(self, args, source_dictionary=None, target_dictionary=None):
        super().__init__(args)
        self._target_dictionary, self._source_dictionary = target_dictionary, source_dictionary
        self.is_ctc = getattr(args, "criterion", None) == "ctc"
        self.datasets = {}

    @classmethod
    def setup_task(cls, args, **kwargs):
        if not getattr(args, "labels", None):
            if getattr(args, "criterion", None) != "wav2vec":
                raise NotImplementedError("wav2vec2 pre-training is not built: the audio_pretraining task needs --labels (CTC fine-tuning)"
                                          " — or --criterion wav2vec, which pre-trains")
            if getattr(args, "enable_padding", False):
                raise NotImplementedError("--enable-padding is not built for wav2vec2 pre-training: batches are cropped to their shortest utterance")
            return cls(args)
        target_dictionary = kwargs.pop("target_dictionary", None)
        if target_dictionary is None:
            target_dictionary = Dictionary.load(os.path.join(args.data, "dict.%s.txt" % args.labels))
        return cls(args, target_dictionary=target_dictionary)

    def load_dataset(self, split, **kwargs):
        from . import data as D
        if not getattr(self.args, "labels", None):  # pre-training: the manifest alone, every batch cropped to its shortest utterance
            self.datasets[split] = D.AudioLabelDataset(
                os.path.join(self.args.data, "%s.tsv" % split), getattr(self.args, "sample_rate", 16000), None, 0, None,
                max_sample_size=self.args.max_sample_size, min_length=self.args.min_sample_size, pad=False, normalize=self.args.normalize)
            return self.datasets[split]
        with open(os.path.join(self.args.data, "%s.%s" % (split, self.args.labels)), "r") as f:
            labels = [line for line in f]
        d = self.target_dictionary
        self.datasets[split] = D.AudioLabelDataset(
            os.path.join(self.args.data, "%s.tsv" % split), getattr(self.args, "sample_rate", 16000), labels, d.pad(),
            D.LabelEncoder(d), max_sample_size=self.args.max_sample_size, min_length=self.args.min_sample_size, pad=self.args.labels is not None or self.args.enable_padding, normalize=self.args.normalize)
        return self.datasets[split]

    @property
    def source_dictionary(self):
        return self._source_dictionary

    @property
    def target_dictionary(self):
        return self._target_dictionary

    def max_positions(self):
        import sys
        return sys.maxsize, sys.maxsize


@register_task("language_modeling")
class LanguageModelingTask(FairseqTask):
    """tasks/language_modeling.py:96-328 — a left-to-right language model on a binarised monolingual corpus (indexed_dataset.py,
    monolingual_dataset.py): `<data>/dict.txt`, `<data>/<split>.{bin,idx}`.  Trains the model `fairseq_generate.py --lm-path` fuses
    and fairseq_eval_lm.py scores.  Refused by name: what a fusion LM does not use."""
    BREAK_MODES = ("none", "complete", "complete_doc", "eos")
    # (args attribute, the flag to name, the value that is built)
    _REFUSED = (("output_dictionary_size", "--output-dictionary-size", -1), ("self_target", "--self-target", False),
                ("past_target", "--past-target", False), ("add_bos_token", "--add-bos-token", False),
                ("shorten_method", "--shorten-method", "none"))

    @staticmethod
    def add_args(parser):
        """language_modeling.py:40-93, with the dataset option the reference keeps among its common ones."""
        parser.add_argument("data", help="path to the binarised data directory")
        parser.add_argument("--sample-break-mode", default="none", choices=list(LanguageModelingTask.BREAK_MODES),
                            help="none: blocks of --tokens-per-sample tokens; complete: whole sentences up to that many tokens; "
                            "complete_doc: the same within documents (blank lines separate them); eos: one sentence per block")
        parser.add_argument("--tokens-per-sample", default=1024, type=int, help="max number of tokens per sample for LM dataset")
        parser.add_argument("--output-dictionary-size", default=-1, type=int, help="(not built)")
        parser.add_argument("--self-target", action="store_true", help="(not built)")
        parser.add_argument("--future-target", action="store_true", help="include future target (what this build always does)")
        parser.add_argument("--past-target", action="store_true", help="(not built)")
        parser.add_argument("--add-bos-token", action="store_true", help="(not built)")
        parser.add_argument("--max-target-positions", default=None, type=int, metavar="N", help="max number of tokens in the target sequence")
        parser.add_argument("--shorten-method", default="none", help="(values other than none are not built)")
        parser.add_argument("--shorten-data-split-list", default="")
        parser.add_argument("--dataset-impl", default=None, metavar="FORMAT", help="mmap (the other implementations are not built)")

    def __init__(self, args, dictionary):
        super().__init__(args)
        self.dictionary = dictionary
        self.targets = ["future"]
        self.datasets = {}

    @classmethod
    def check_args(cls, args):
        for attr, flag, built in cls._REFUSED:
            v = getattr(args, attr, built)
            if v is None or v == built or (attr == "output_dictionary_size" and v < 0):
                continue
            raise NotImplementedError("language_modeling: %s%s is not built: the model predicts the next token over the whole "
                                      "dictionary from the tokens before it" % (flag, "" if v is True else " %s" % v))
        if getattr(args, "exclude_self_target", True) is False:  # (an old checkpoint's spelling of --self-target)
            raise NotImplementedError("language_modeling: --self-target is not built")
        mode = getattr(args, "sample_break_mode", "none") or "none"
        if mode not in cls.BREAK_MODES:
            raise ValueError("--sample-break-mode %r: one of %s" % (mode, ", ".join(cls.BREAK_MODES)))
        from . import indexed_dataset as ID
        ID.check_dataset_impl(getattr(args, "dataset_impl", None))

    @classmethod
    def setup_task(cls, args, **kwargs):
        """language_modeling.py:135-175."""
        cls.check_args(args)
        dictionary = kwargs.pop("dictionary", None)
        data = getattr(args, "data", None)
        if dictionary is None and not data:  # a checkpoint whose data directory is not reachable: ids only
            dictionary = Dictionary.synthetic(getattr(args, "synthetic_vocab_size", 10000))
        if dictionary is None:
            from . import language_pair_dataset as P
            paths = P.split_paths(data)
            if len(paths) > 1:
                raise NotImplementedError("several colon-separated data paths (%d given) are not built: the round-robin over data "
                                          "shards of the reference's language_modeling task; pass one directory" % len(paths))
            dictionary = Dictionary.load(os.path.join(paths[0], "dict.txt"))
        return cls(args, dictionary)

    def load_dataset(self, split, epoch=1, combine=False, **kwargs):
        """language_modeling.py:188-241: split -> indexed dataset -> token blocks -> MonolingualDataset.  The split's route of batch
        assembly (device-resident corpus or host collater) is decided here."""
        from . import indexed_dataset as ID
        from . import monolingual_dataset as M
        a = self.args
        prefix = os.path.join(a.data, split)
        if not ID.dataset_exists(prefix):
            if os.path.exists(prefix + ".txt"):
                raise NotImplementedError("%s.txt: the `raw` dataset implementation is not built; binarise with --dataset-impl mmap" % prefix)
            raise FileNotFoundError("Dataset not found: {} ({})".format(split, prefix))
        if ID.dataset_exists(prefix + "1"):
            raise NotImplementedError("%s1: sharded splits (train, train1, ...) are not built; binarise the corpus as one split" % prefix)
        corpus = ID.MMapIndexedDataset(prefix)
        blocks = M.TokenBlockDataset(corpus, corpus.sizes, getattr(a, "tokens_per_sample", 1024), pad=self.dictionary.pad(),
                                     eos=self.dictionary.eos(), break_mode=getattr(a, "sample_break_mode", "none"), include_targets=True)
        ds = M.MonolingualDataset(blocks, blocks.sizes, self.dictionary, shuffle=True)
        ds.enable_resident()
        self.datasets[split] = ds
        return ds

    def build_model(self, args):
        """:177-186."""
        model = super().build_model(args)
        for target in self.targets:
            if target not in model.supported_targets:
                raise ValueError("Unsupported language modeling target: {}".format(target))
        return model

    def build_dataset_for_inference(self, src_tokens, src_lengths, **kwargs):
        """language_modeling.py:246-289: typed prompts, each prefixed with eos and right-padded (monolingual_dataset.PromptDataset)."""
        from . import monolingual_dataset as M
        return M.PromptDataset(src_tokens, src_lengths, self.source_dictionary)

    def inference_step(self, generator, models, sample, prefix_tokens=None, constraints=None):
        """language_modeling.py:291-315: the generator does not read src_tokens of a decoder-only model; the prompt batch becomes
        prefix_tokens, without its leading eos column (the token every hypothesis starts from)."""
        with torch.no_grad():
            bos_token = self.source_dictionary.eos()  # (--add-bos-token is refused by check_args)
            if constraints is not None:
                raise NotImplementedError("Constrained decoding with the language_modeling task is not supported")
            if prefix_tokens is None and sample["net_input"]["src_tokens"].nelement():
                prefix_tokens = sample["net_input"]["src_tokens"]
                if prefix_tokens[:, 0].eq(bos_token).all():
                    prefix_tokens = prefix_tokens[:, 1:]
                if prefix_tokens.size(1) == 0:  # a batch of empty prompts: nothing is forced
                    prefix_tokens = None
            return generator.generate(models, sample, prefix_tokens=prefix_tokens, bos_token=bos_token)

    def max_positions(self):
        """The target limit: --max-target-positions, else --tokens-per-sample (what the model is built with)."""
        v = getattr(self.args, "max_target_positions", None)
        return v if v is not None else getattr(self.args, "tokens_per_sample", 1024)

    @property
    def source_dictionary(self):
        return self.dictionary

    @property
    def target_dictionary(self):
        return self.dictionary
