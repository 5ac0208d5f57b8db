"""samples_per_image is validated before any device work: the ValueError needs no GPU."""
import pytest
import torch

import helpers
from vsrcap import _lib, synth


@pytest.mark.parametrize("bad", [0, -1, _lib.MAX_BEAM + 1])
def test_samples_per_image_out_of_range_raises_before_the_device_is_touched(bad):
    cfg = dict(V=61, B=3, R0=6, R=7, D=128, L=3, T=7, E=32, H=48, A=16)
    m = helpers.build_model(cfg, helpers.weights_for(cfg), "cpu")
    det, ctrl = helpers.decode_inputs(cfg, 12)
    with pytest.raises(ValueError, match="samples_per_image"):
        m.sample_rl(det, ctrl, samples_per_image=bad)


def test_max_beam_matches_the_header():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vsrcap.h")).read()
    assert int(re.search(r"#define VSR_MAX_BEAM (\d+)", text).group(1)) == _lib.MAX_BEAM
