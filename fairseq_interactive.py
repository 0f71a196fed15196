#!/usr/bin/env python3
"""fairseq-interactive entry point of this build (chimera/scripts/interactive-en2any-ST.sh calls `fairseq-interactive <data> --task triplet
--config-yaml config_wave.yaml --path ...`): type audio paths, sentences or language-model prompts, read H-/D-/P- lines."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    importlib.import_module("chimera-st_amd.cli").interactive_main()
