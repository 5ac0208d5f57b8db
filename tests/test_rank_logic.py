"""csrc/rank_logic.h (the integer logic the ranking kernels run, one statement for host and device) against the Python of
vsrcap.evalbatch on the CPU: tools/rank_logic_host.cpp is built with the host compiler into a temp dir and driven on the cases the issue
names plus seeded random ones, with the networks' decisions injected (tests/rank_ref.py).  Everything must be exactly equal."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rank_ref as rr

N_RANDOM = 2400


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("vsr_build", os.path.join(ROOT, "vsr-guided-cic_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build_rank_tool(out=str(tmp_path_factory.mktemp("rank") / "rank_logic_host"), force=True)


def run_tool(tool, cases, exps):
    lines = [str(len(cases))]
    for c, e in zip(cases, exps):
        lines.append("%d %d %d %d %d %d %d" % (c.N, rr.L, c.MV, c.MS, c.n_sink, rr.N_VERBS, c.max_items))
        for a in (c.control_verb, c.det_seqs_v, c.det_seqs_sr, e["pred"], e["assign"]):
            lines.append(" ".join(map(str, np.asarray(a).reshape(-1).tolist())))
    res = subprocess.run([tool], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert len(out) == len(cases)
    got = []
    for c, line in zip(cases, out):
        v = np.array(line.split(), dtype=np.int64)
        S, Q = c.S, c.qcap
        cuts = np.cumsum([S, S * rr.L, 1, Q * c.n_sink, c.N * rr.L, c.N])
        assert len(v) == cuts[-1]
        jv, jr, ni, g, rank, st = np.split(v, cuts[:-1])
        got.append(dict(job_verbs=jv, job_roles=jr.reshape(S, rr.L), n_items=int(ni[0]), gather=g.reshape(Q, c.n_sink), rank=rank.reshape(c.N, rr.L), status=st))
    return got


def check(cases, exps, got):
    for c, e, g in zip(cases, exps, got):
        for k in ("job_verbs", "job_roles", "n_items", "gather", "status", "rank"):
            np.testing.assert_array_equal(g[k], e[k], err_msg="%s: %s" % (c.name, k))


def test_special_cases_are_what_they_say_and_match(tool):
    cases = rr.special_cases()
    rng = np.random.RandomState(0)
    stats = {c.name: dict(out_of_order=0, long=0, duplicate=0) for c in cases}
    exps = [rr.expected(c, rng, stats[c.name]) for c in cases]
    by = {c.name: (c, e) for c, e in zip(cases, exps)}
    assert by["n1_mv1"][1]["rank"][0].tolist()[:4] != [-1] * 4 and by["n1_mv1"][1]["n_items"] == 1
    assert by["no_match"][1]["status"].tolist() == [0, rr.NO_JOB, 0]
    assert (by["v_0_w"][1]["job_verbs"] != 0).tolist() == [True, False, False]
    c, e = by["two_columns_gate"]
    assert np.count_nonzero(e["job_roles"][0]) == 10 and len(np.unique(c.det_seqs_sr[0][c.det_seqs_v[0] == 21])) > 10      # the gate closed
    assert e["gather"][0, :2].tolist() == [0, 0] and stats["two_columns_gate"]["duplicate"]                               # slot 0 twice in one list
    c, e = by["more_than_n_sink"]
    assert (c.det_seqs_sr[0, :, 0] == 2).sum() == 6 > c.n_sink and (e["gather"][0] >= 0).all()
    assert stats["longer_than_L"]["long"] == 1
    assert stats["out_of_order"]["out_of_order"] == 1
    c, e = by["max_items_minus_one"]
    assert e["n_items"] == c.max_items + 1 and e["status"].tolist() == [0, 0, rr.ITEM_OVERFLOW] and (e["rank"][2] == -1).all() and (e["rank"][:2, 0] >= 0).all()
    check(cases, exps, run_tool(tool, cases, exps))


def test_random_cases_match(tool):
    rng = np.random.RandomState(20260)
    stats = dict(out_of_order=0, long=0, duplicate=0)
    cases = [rr.random_case(rng) for _ in range(N_RANDOM)]
    exps = [rr.expected(c, rng, stats) for c in cases]
    assert N_RANDOM >= 2000
    # the generator reaches every corner it is meant to (counted on the Python side, so a silent change of the generator fails here)
    assert stats["out_of_order"] > 20 and stats["long"] > 20 and stats["duplicate"] > 20, stats
    assert sum(int((e["status"] & rr.ITEM_OVERFLOW).any()) for e in exps) > 20
    assert sum(int((e["status"] & rr.NO_JOB).any()) for e in exps) > 20
    assert sum(int(np.count_nonzero(e["job_roles"][s]) == 10) for e in exps for s in range(len(e["job_roles"]))) > 5
    check(cases, exps, run_tool(tool, cases, exps))


def test_limits_fail_loudly(tool):
    c = rr.special_cases()[0]
    for L, MV, n_sink in ((9, 1, 10), (10, 9, 10), (10, 1, 1), (10, 1, 17)):
        head = "1\n1 %d %d %d %d %d 0\n" % (L, MV, MV, n_sink, rr.N_VERBS)
        res = subprocess.run([tool], input=head + "0 " * 400, capture_output=True, text=True, timeout=60)
        assert res.returncode == 3 and "limits" in res.stderr
