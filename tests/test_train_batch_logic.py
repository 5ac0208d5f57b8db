"""The training-batch builder on the CPU.  Two links of one chain:
  1. the numpy yardsticks of vsrcap.trainbatch (ssp_train_batch, sinkhorn_train_items) reproduce, exactly, what the REFERENCE's own loops
     made of the seeded inputs of tests/golden/g18_train_batch.npz (tests/golden/make_golden_train_batch.py executed them);
  2. csrc/train_batch_logic.h - the statement the kernels run - equals the yardsticks exactly: tools/train_batch_host.cpp is built with the
     host compiler into a temp dir and driven on the fixture, on the named corners and on 2000 seeded random cases
     (tests/train_batch_ref.py)."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import train_batch_ref as tr
from vsrcap import trainbatch as tb

N_RANDOM = 2000


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which(os.environ.get("CXX", "c++")) is None and shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    spec = importlib.util.spec_from_file_location("vsr_build", os.path.join(ROOT, "vsr-guided-cic_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build_train_batch_tool(out=str(tmp_path_factory.mktemp("tb") / "train_batch_host"), force=True)


def test_yardsticks_reproduce_the_reference_fixture():
    meta, g, c = tr.fixture_case()
    verbs, det, gt = tb.ssp_train_batch(c.control_verb, c.det_seqs_v, c.det_seqs_sr, c.gt_seqs_v, c.gt_seqs_sr)
    assert len(verbs) == meta["n_seqs"] == 14
    for got, key in ((verbs, "ref_verbs"), (det, "ref_det_roles"), (gt, "ref_gt_roles")):
        assert got.shape == g[key].shape
        np.testing.assert_array_equal(got, g[key], err_msg=key)
    gather, t, gl, keys = tb.sinkhorn_train_items(c.control_verb, c.det_seqs_v, c.det_seqs_sr, c.idx_list, n_sink=meta["n_sink"])
    ref = tr.fixture_items(meta, g)
    assert sorted(map(tuple, keys.tolist())) == sorted(ref) and len(keys) == 21
    for q, key in enumerate(map(tuple, keys.tolist())):
        for got, want, what in zip((gather[q], t[q], gl[q]), ref[key], ("gather", "tr_locs", "gt_locs")):
            assert got.shape == want.shape and (what == "gather" or got.dtype == want.dtype == np.float32)
            np.testing.assert_array_equal(got, want, err_msg="%s %s" % (key, what))
    assert keys.tolist() == sorted(keys.tolist())                 # the order of the reference's loops: captions, verb columns, ascending role
    assert (tr.caption_status(**c.annotations()) == 0).all()


def test_special_cases_are_what_they_say():
    by = {c.name: (c, c.expected()) for c in tr.special_cases()}
    c, e = by["truncation"]
    assert e["status"].tolist() == [tb.TRUNCATED] and e["counts"].tolist() == [1, 1, tb.TRUNCATED, 0]
    assert e["item_gather"][0].tolist() == [0, 1, 3] and e["tr_locs"][0].tolist() == [0.0, 1.0, 3.0] and e["gt_locs"][0].tolist() == [2.0, 1.0, 0.0]
    for name in ("role_26_det", "role_26_gt"):
        c, e = by[name]
        assert e["status"].tolist() == [0, tb.BAD_ROLE, 0] and e["counts"].tolist() == [2, 2, tb.BAD_ROLE, 0]
        assert e["verbs"].tolist()[:3] == [61, 63, 0] and e["item_key"][:2, 0].tolist() == [0, 2] and e["item_gather"][1, 0] == 2 * tr.L
    c, e = by["negative_verb"]
    assert e["status"].tolist() == [0, 0, tb.BAD_VERB] and e["counts"].tolist() == [2, 2, tb.BAD_VERB, 0]
    c, e = by["idx_10_stable_tie"]
    assert e["status"].tolist() == [tb.BAD_IDX] and e["gt_locs"][0].tolist() == [1.0, 0.0, 10.0, 10.0] and e["tr_locs"][0].tolist() == [0.0, 1.0, 10.0, 10.0]
    c, e = by["max_items_minus_one"]
    assert e["counts"].tolist() == [3, 2, 0, 1] and e["item_gather"].shape == (2, 10) and e["item_key"][:, 0].tolist() == [0, 1]
    c, e = by["all_inactive"]
    assert e["counts"].tolist() == [0, 0, 0, 0] and not e["verbs"].any() and (e["item_gather"] == -1).all()
    assert not by["no_gt"][1]["gt_roles"].any() and by["no_gt"][1]["counts"].tolist() == [3, 3, 0, 0]
    assert by["no_idx"][1]["counts"].tolist() == [3, 0, 0, 0] and by["no_idx"][1]["gt_roles"][0].tolist()[:4] == [1, 2, 3, 0]
    c, e = by["gate_and_lg1"]
    assert e["det_roles"][0].tolist() == list(range(1, 11)) and e["gt_roles"][0].tolist() == [9] + [0] * 9 and e["counts"].tolist() == [1, 0, 0, 0]


def test_host_tool_equals_the_yardsticks_on_fixture_and_corners(tool):
    cases = [tr.fixture_case()[2]] + tr.special_cases()
    for c, got in zip(cases, tr.run_tool(tool, cases)):
        tr.check(c, c.expected(), got)


def test_host_tool_equals_the_yardsticks_on_random_cases(tool):
    rng = np.random.RandomState(20261)
    cases = [tr.random_case(rng) for _ in range(N_RANDOM)]
    exps = [c.expected() for c in cases]
    assert N_RANDOM >= 2000
    # the generator reaches every corner it is meant to (counted on the yardsticks' side, so a silent change of the generator fails here)
    bit = lambda b: sum(int(e["counts"][2]) & b != 0 for e in exps)
    assert bit(tb.TRUNCATED) > 20 and bit(tb.BAD_ROLE) > 20 and bit(tb.BAD_VERB) > 5 and bit(tb.BAD_IDX) > 5, [bit(b) for b in (4, 8, 32, 64)]
    assert sum(int(e["counts"][3] > 0) for e in exps) > 20 and sum(int(e["counts"][0] == 0) for e in exps) > 20
    assert sum(int(np.count_nonzero(r) == 10) for e in exps for r in e["det_roles"]) > 5
    assert {(c.MV, c.n_sink, c.Lg) for c in cases if c.gt_seqs_v is not None} >= {(mv, k, lg) for mv in (1, 3, 8) for k in (2, 10, 16) for lg in (1, 10, 13)}
    assert {c.MS - c.MV for c in cases} == {0, 1}
    for c, e, got in zip(cases, exps, tr.run_tool(tool, cases)):
        tr.check(c, e, got)


def test_limits_fail_loudly(tool):
    for Lx, Lg, MV, n_sink in ((9, 10, 1, 10), (10, 10, 9, 10), (10, 10, 1, 1), (10, 10, 1, 17), (10, 0, 1, 10)):
        head = "1\n1 %d %d %d %d %d %d 0 1 1\n" % (Lx, Lg, MV, MV, n_sink, tr.N_VERBS)
        res = subprocess.run([tool], input=head + "0 " * 400, capture_output=True, text=True, timeout=60)
        assert res.returncode == 3 and "limits" in res.stderr
