#!/usr/bin/env python3
"""examples/speech_recognition/infer.py for the MI355X-native build: transcribe a subset with a wav2vec_ctc checkpoint (chimera-st_amd/cli.py infer_main).

  python fairseq_infer.py <data> --task audio_pretraining --labels ltr --path ckpt.pt --gen-subset dev --w2l-decoder beam --beam 50 --results-path out
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    importlib.import_module("chimera-st_amd.cli").infer_main()
