#!/usr/bin/env python3
"""fairseq-eval-lm for the MI355X-native build: the perplexity of a language model on a binarised split (chimera-st_amd/cli.py eval_lm_main).

  python fairseq_eval_lm.py <data> --path lm.pt --gen-subset valid --max-tokens 4096 --sample-break-mode eos
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    importlib.import_module("chimera-st_amd.cli").eval_lm_main()
