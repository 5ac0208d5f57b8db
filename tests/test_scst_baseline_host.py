"""The host side of sample_rl(..., greedy_baseline=True), without a GPU: the argument check that precedes any engine, and the row layout
of vsrcap/baseline_rows.py held to the rule include/vsrcap.h states for vsr_sample_rows_baseline."""
import pytest
import torch

import helpers
from vsrcap import _lib, baseline_rows


def test_samples_plus_the_baseline_row_must_fit_the_beam_workspace():
    cfg = dict(V=20, B=2, R0=3, R=3, D=16, L=2, T=4, E=8, H=8, A=8)
    m = helpers.build_model(cfg, helpers.weights_for(cfg), "cpu")
    det, ctrl = helpers.decode_inputs(cfg, 1)
    with pytest.raises(ValueError, match="samples_per_image") as e:
        m.sample_rl(det, ctrl, samples_per_image=_lib.MAX_BEAM, greedy_baseline=True)
    assert "greedy_baseline" in str(e.value)
    assert m._eng is None, "an engine was created before the arguments were checked"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", range(1, 8))
def test_row_map_is_a_bijection_in_repeat_interleave_order(K, B):
    rows = [baseline_rows.decoder_row(r, K) for r in range((K + 1) * B)]
    assert len(set(rows)) == len(rows)
    assert sorted(i for kind, i in rows if kind == "baseline") == list(range(B))
    assert sorted(i for kind, i in rows if kind == "sample") == list(range(B * K))
    assert {kind for kind, _ in rows} == {"baseline", "sample"}
    # K + 1 adjacent rows per image, the baseline first; sample j of image b at b K + j: the order of repeat_interleave(K)
    image_of_sample = torch.arange(B).repeat_interleave(K).tolist()
    for b in range(B):
        assert rows[b * (K + 1)] == ("baseline", b)
        for j in range(K):
            kind, i = rows[b * (K + 1) + 1 + j]
            assert (kind, i) == ("sample", b * K + j) and image_of_sample[i] == b
    assert baseline_rows.output_rows(B, K) == (B * K, B)
    # the form the kernels use (csrc/kernels.h, sample_row)
    assert all(i == r - r // (K + 1) - 1 for r, (kind, i) in enumerate(rows) if kind == "sample")


def test_row_map_rejects_what_is_no_row():
    for row, K in ((0, 0), (-1, 3)):
        with pytest.raises(ValueError):
            baseline_rows.decoder_row(row, K)
