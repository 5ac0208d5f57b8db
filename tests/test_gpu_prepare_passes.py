"""The streaming passes of vsr_prepare() (csrc/kernels.h: k_rowmask with two row sets per launch, k_compact_count / k_compact_write,
k_pool with eight rows' loads in flight, k_slab_reduce_scatter with four elements per thread) on the sizes where their loops change shape.

Inputs are NON-NEGATIVE, as the reference's post-ReLU features are: a row's sum is then zero iff the row is zero, whatever the order
of the adds, and numpy is a valid yardstick for the mask.

  * the row mask through the library's exported entry (engine.row_mask -> vsr_row_mask): 1, 4k + 1 and 4k + 3 rows (blocks take four
    rows); D = 256 (one load per lane), 2048 (eight), 2304 (nine); all rows zero, all rows valid, exactly one valid row - with the
    only non-zero element of a valid row in the first and the last lane of the first, a middle and the last load in turn.
  * the compacted list and its count through prepare + decode: the ids are the CPU oracle's on those sizes and patterns, and a batch
    decodes to the same ids after the rows of each slot's tail (everything behind its first row: valid rows and padding) changed
    places, which moves every padding row and so every entry of the list.  With and without a caller's rows bound.
Reference ops: models/controllable_captioning.py:126-128 (pooled descriptor), :159 (row mask)."""
import numpy as np
import pytest
import torch

import helpers
from vsrcap import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAVOURS = ("f16x2", "f32x3", "f32")
DS = (256, 2048, 2304)
ROWS = (1, 9, 11)                # 1, 4k + 1, 4k + 3


def _cfg(D, **kw):
    return dict(dict(V=50, B=1, R0=7, R=3, D=D, L=3, T=4, E=64, H=64, A=32), **kw)


@pytest.fixture(scope="module")
def engine():
    cfg = _cfg(256)
    return helpers.build_model(cfg, helpers.weights_for(cfg), DEV)._engine(torch.device(DEV))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", ROWS)
def test_row_mask_sizes_and_patterns(engine, n, D):
    # the element of lane l's k-th load: column 256 k + 4 l + e
    cols = sorted({c for c in (0, 3, 252, 255, 256, 1023, 1792, 2047, 2048, 2051, D - 4, D - 1) if c < D})
    dense = synth.make_detections(1, n, D, seed=3, min_valid=n)[0]
    assert (dense >= 0).all() and (dense.sum(-1) != 0).all()
    cases = {"all rows zero": np.zeros((n, D), np.float32), "all rows valid (dense)": dense}
    for i, c in enumerate(cols):
        x = np.zeros((n, D), np.float32)
        x[:, c] = 1e-30                                   # (tiny but normal: a sum that is not zero)
        cases["all rows valid (column %d)" % c] = x
        y = np.zeros((n, D), np.float32)
        y[(i * 5) % n, c] = 0.5
        cases["one valid row (row %d, column %d)" % ((i * 5) % n, c)] = y
    for name, x in cases.items():
        got = engine.row_mask(torch.from_numpy(x).to(DEV)).cpu().numpy()
        want = (x.astype(np.float64).sum(-1) != 0).astype(np.float32)
        np.testing.assert_array_equal(got, want, err_msg="%s, %d rows, D = %d" % (name, n, D))


def _regions(B, L, R, D, pattern, seed):
    """(B, L, R, D) >= 0 and its number of non-zero rows"""
    if pattern == "zero":
        x = np.zeros((B, L, R, D), np.float32)
    elif pattern == "valid":
        x = synth.make_detections(B * L, R, D, seed=seed, min_valid=R).reshape(B, L, R, D)
    elif pattern == "one":
        x = np.zeros((B, L, R, D), np.float32)
        x[B - 1, L - 1, R // 2] = synth.make_detections(1, 1, D, seed=seed, min_valid=1)[0, 0]
    else:
        x = synth.make_ctrl(B, L, R, D, seed=seed)
    return x, int((x.sum(-1) != 0).sum())


def _decode(m, det, ctrl):
    with torch.no_grad():
        w, g = m.test(det, ctrl)
        (bw, bg), _ = m.beam_search((det, ctrl), [3, -1], 3, 1)
    return [t.cpu() for t in (w, g, bw, bg)]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("D", DS)
def test_compacted_rows_through_prepare_and_decode(D, flavour):
    import vsr_oracle as vo
    cfg = _cfg(D)
    w = helpers.weights_for(cfg)
    m = helpers.build_model(cfg, w, DEV).set_compute_dtype(flavour)
    o = vo.Oracle(w, cfg["T"], 2, as_written=False)
    # region rows B x L x R = 1, 9, 11 (+ 15 for the tail permutation); detection rows B x 7 = 7, 21
    for (B, L, R) in ((1, 1, 1), (1, 3, 3), (1, 1, 11)):
        det = torch.from_numpy(synth.make_detections(B, cfg["R0"], D, seed=5))
        for pattern in ("zero", "valid", "one"):
            x, valid = _regions(B, L, R, D, pattern, seed=9)
            ctrl = torch.from_numpy(x)
            ow, og = o.test(det, ctrl)
            for bound in (None, valid if valid > 0 else B * L * R):
                m.set_valid_rows_bound(bound)
                got = _decode(m, det.to(DEV), ctrl.to(DEV))
                what = "%s rows of %d x %d x %d, D = %d, bound %s" % (pattern, B, L, R, D, bound)
                assert torch.equal(got[0], ow) and torch.equal(got[1], og), what
            m.set_valid_rows_bound(None)
    B, L, R = 3, 1, 5
    det = torch.from_numpy(synth.make_detections(B, cfg["R0"], D, seed=6))
    x, valid = _regions(B, L, R, D, "mixed", seed=6)
    assert 0 < valid < B * L * R
    y = np.ascontiguousarray(np.concatenate([x[:, :, :1], x[:, :, :0:-1]], axis=2))      # the tail behind each slot's first row, reversed
    assert ((x.sum(-1) != 0) != (y.sum(-1) != 0)).any()
    for bound in (None, valid):
        m.set_valid_rows_bound(bound)
        a = _decode(m, det.to(DEV), torch.from_numpy(x).to(DEV))
        b = _decode(m, det.to(DEV), torch.from_numpy(y).to(DEV))
        for name, s, t in zip(("greedy words", "greedy gates", "beam words", "beam gates"), a, b):
            assert torch.equal(s, t), "%s change with the places of the padding rows (D = %d, bound %s)" % (name, D, bound)
    m.set_valid_rows_bound(None)
