"""Harness-side stand-in for `torchaudio` (absent from this image) so that the REAL reference dataset code can take its
filter-bank route (fairseq/data/audio/audio_utils.py:80-93, _get_torchaudio_fbank) when fbank goldens are generated.  Only
torchaudio.compliance.kaldi.fbank exists, and it delegates to tests/fbank_ref.py: the fixtures it feeds pin the reference's glue
around the call (scaling, transforms, draws, padding, order), not the filter-bank numerics.  Never imported by the product or
by tests."""
