"""csrc/step_gemms.h, slab placement of the step launches (the *_slabs layouts, place_slabs, plan_s56, slab_floats), on the CPU:
tools/step_slabs_host.hip is built into a temp dir; it plans and places every launch of DESIGN.md's layout table on a GemmState of 256 CUs,
in the exact flavour and in f32x3.  The table's rules are restated here in closed form - which problems share a slab array, its width, the
count rule, the area and what precedes the group there - and held against what the tool printed, address for address and count for count."""
import importlib.util
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

DIMS = (dict(H=48, A=16, D=128, E=32, V=61), dict(H=64, A=32, D=64, E=32, V=56), dict(H=256, A=512, D=2048, E=64, V=4104),
        dict(H=1000, A=512, D=2048, E=1000, V=10000),
        # on the default knobs the split composition of S5 / S6 fits pre1's 8 slabs at every shape above: from H = 416 on (13 k-tiles of 32)
        # some launches' stream-K ranges (the rows-16 kernel's, M <= 40, in the exact flavour) are short enough that it does not, and both
        # launches are planned again
        dict(H=416, A=16, D=64, E=32, V=56))
# the environment of tests/test_gpu_configs.py's last kernel-variant case: shorter ranges, so that its decodes at the real dims reach the re-plan
SHORT_RANGES = dict(VSR_GEMM_SLOTS_SMALL="4096", VSR_GEMM_SLOTS_R16="2048", VSR_GEMM_MIN_ITERS="4")
MS = (1, 13, 16, 100, 128, 129, 193, 500, 800)
FLAVOURS = (("exact", 0), ("f32x3", 1))
MAX_SLABS = 8
LAUNCH, TIGHT = "launch", "tight"


def table(name, nprob, d, h2_first, ns_h1):
    """The layout table: the groups of a launch as (problems, width, count rule, area, floats that precede the group's area)"""
    H, A, D, V = d["H"], d["A"], d["D"], d["V"]
    rest = lambda k: list(range(k, nprob))
    if name in ("vproj", "cache_chunk", "train_xproj") or name.startswith("S1_"):
        return [(rest(0), 6 * H, LAUNCH, 0, 0)]
    if name == "vproj2":
        return [([0], 4 * H, LAUNCH, 0, 0)]
    if name == "att_va":
        return [([0], A, LAUNCH, 0, 0)]
    if name == "S2":
        return [([0, 1], H + A, LAUNCH, 0, 0), ([2, 3], D + A, LAUNCH, 0, 0)]
    if name.startswith("train_S5"):
        return [([0], 4 * H, LAUNCH, 0, 0), ([1], A, LAUNCH, 0, 0)]
    if name.startswith("S5_"):       # scratch | ga_slabs | pre1
        return [([0], 4 * H, TIGHT, 0, 0), ([1], A, TIGHT, 1, 0), (rest(2), 6 * H, TIGHT, 2, 0)]
    if name.startswith("S6_"):       # scratch | pre1 behind the ns_h1 slabs of S5
        return [([0], V, TIGHT, 0, 0), (rest(1), 6 * H, TIGHT, 1, ns_h1)]
    if name == "train_vocab":
        return [([0], V, LAUNCH, 0, 0)]
    if name == "bwd1":
        return [([0], H + D, LAUNCH, 0, 0), ([1], H, LAUNCH, 0, 0), ([2], H, LAUNCH, 0, 0)]
    if name == "bwd2":
        return [([0], H, LAUNCH, 0, 0), ([1], H, LAUNCH, 0, 0)]
    if name in ("bwd3", "bwd3_none"):
        return [(rest(0)[:1], H, LAUNCH, 0, 0), (rest(1), H, LAUNCH, 0, 0)]
    raise AssertionError(name)


def nprob_of(name, h2_first, img_second, replan):
    """problems per launch: a problem of the LSTM1 list without a k segment does not exist (the shift-gate block has no h1 part)"""
    l1_state = 3 if h2_first else 2          # h2 | h1 parts: the third problem only through its h2 columns
    fixed = {"vproj": 3, "vproj2": 1, "att_va": 1, "cache_chunk": 3, "train_xproj": 3, "S1_none": 0, "S1_x": 3, "S1_rec": l1_state, "S1_all": 3, "S2": 4,
             "train_vocab": 1, "bwd1": 3, "bwd2": 2, "bwd3": 2 if h2_first else 1, "bwd3_none": 0}
    if name in fixed:
        return fixed[name]
    if name.startswith("train_S5"):
        return 2
    mode = int(name[-1])
    split = mode == 2 and h2_first and not replan
    if name.startswith("S5_"):
        return 4 if split else 2
    return 1 if mode == 0 else 1 + (3 if split else l1_state)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("vsr_build", os.path.join(ROOT, "vsr-guided-cic_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build_step_slabs_tool(out=str(tmp_path_factory.mktemp("step_slabs") / "step_slabs_host"), force=True)


def run(tool, d, M, h2_first, img_second, x3, knobs=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VSR_")}          # (the tool reads the routing knobs, as vsr_create does)
    env.update(knobs or {})
    res = subprocess.run([tool] + [str(v) for v in (d["H"], d["A"], d["D"], d["E"], d["V"], M, h2_first, img_second, x3, 1)], capture_output=True, text=True,
                         timeout=60, env=env)
    assert res.returncode == 0, res.stderr
    launches, pre1 = [], None
    for line in res.stdout.splitlines():
        w = line.split()
        kv = lambda ws: {ws[i]: int(ws[i + 1]) for i in range(0, len(ws), 2)}
        if w[0] == "launch":
            launches.append(dict(name=w[1], **kv(w[2:]), probs=[], views=[], areas={}, refused=[], accepted=[], pre1=pre1))
            pre1 = None
        elif w[0] == "pre1":
            pre1 = kv(w[1:])
        elif w[0] == "prob":
            launches[-1]["probs"].append(kv(w[2:]))
        elif w[0] == "view":
            launches[-1]["views"].append(kv(w[2:]))
        elif w[0] == "area":
            launches[-1]["areas"][int(w[1])] = kv(w[2:])
        elif w[0] == "refused":
            launches[-1]["refused"].append(line[len("refused "):])
        elif w[0] == "accepted":
            launches[-1]["accepted"].append(line)
        else:
            raise AssertionError(line)
    return launches


@pytest.fixture(scope="module")
def cases(tool):
    """every dims set x M x flag pair x flavour, run once"""
    out = []
    for (di, d), M, h2_first, img_second, (fl, x3) in itertools.product(enumerate(DIMS), MS, (0, 1), (0, 1), FLAVOURS):
        out.append(dict(di=di, d=d, M=M, h2_first=h2_first, img_second=img_second, flavour=fl, launches=run(tool, d, M, h2_first, img_second, x3)))
    for M in (13, 24, 40, 120):               # the rows of that GPU case's greedy and beam-5 decodes, exact flavour
        out.append(dict(di=3, d=DIMS[3], M=M, h2_first=1, img_second=0, flavour="exact, short ranges", launches=run(tool, DIMS[3], M, 1, 0, 0, SHORT_RANGES)))
    return out


def where(c, l):
    return f"{l['name']} dims {c['di']} M {c['M']} h2_first {c['h2_first']} img_second {c['img_second']} {c['flavour']}"


def test_every_launch_is_placed_as_the_table_says(cases):
    for c in cases:
        d, M = c["d"], c["M"]
        names = [l["name"] for l in c["launches"]]
        assert ("vproj2" in names) == bool(c["img_second"]) and len(names) == len(set(names)) == 28 + c["img_second"]
        for l in c["launches"]:
            at = where(c, l)
            m = min(M, 512) if l["name"] == "cache_chunk" else M
            assert l["nprob"] == nprob_of(l["name"], c["h2_first"], c["img_second"], l["replan"]) == len(l["probs"]), at
            assert 1 <= l["ns"] <= MAX_SLABS or l["nprob"] == 0, at
            ns_h1 = l["pre1"]["ns_h1"] if l["pre1"] else 0
            groups = table(l["name"], l["nprob"], d, c["h2_first"], ns_h1)
            assert len(groups) == len(l["views"]), at
            end = {}                             # per area: where the next group begins
            for (probs, width, rule, area, before), v in zip(groups, l["views"]):
                n = 0 if not probs else (l["ns"] if rule == LAUNCH else max(l["probs"][i]["tight"] for i in probs))
                base = end.get(area, before * m * 6 * d["H"])
                assert v == dict(area=area, off=base, n=n, stride=m * width), at
                col = 0
                for i in probs:
                    p = l["probs"][i]
                    # a consumer's count is the count of every problem of its group; columns are consecutive from 0
                    assert (p["area"], p["off"], p["ldc"], p["stride"], p["nslab"]) == (area, base + col, width, m * width, n), at
                    # 16-byte alignment is kept wherever the area's base has it - for dims in multiples of 4 (vsr_create refuses others) and a
                    # V group that begins its area, as here; a group behind an odd number of rows of a width that is no multiple of 4 would
                    # lose it (the tile kernels then store scalars: vec_ok), in the parent's hand-written placement as well
                    assert p["tight"] <= n and p["off"] % 4 == 0, at
                    col += p["N"]
                assert col <= width, at
                end[area] = base + n * m * width  # packed: disjoint, nothing between the groups of an area
            for area, a in l["areas"].items():
                width = sum(g[1] for g in groups if g[3] == area)
                before = max([g[4] for g in groups if g[3] == area] + [0]) * m * 6 * d["H"]
                assert a["cap"] == m * width * MAX_SLABS - before, at              # what the workspace functions size the area with
                assert a["used"] == end.get(area, before) - before <= a["cap"], at


def test_s5_and_s6_share_pre1_and_the_replan_is_reached(cases):
    replans, counts = [], set()
    for c in cases:
        by = {l["name"]: l for l in c["launches"]}
        for l in c["launches"]:
            counts.update(v["n"] for v in l["views"])
        for with_h2, mode in itertools.product((0, 1), (0, 1, 2)):
            s5, s6 = by[f"S5_h2{with_h2}_mode{mode}"], by[f"S6_h2{with_h2}_mode{mode}"]
            at = where(c, s6)
            p = s6["pre1"]
            assert s5["replan"] == s6["replan"] and s5["views"][2]["n"] == p["ns_h1"], at
            assert p["ns_h1"] + p["ns_pre1"] <= MAX_SLABS or p["ns_h1"] == 0, at
            assert p["nblk6"] == (0 if mode == 0 else (6 if c["h2_first"] else 5)), at
            if s6["nprob"] > 1:
                # the next step's LSTM1 kernel reads ns_h1 + ns_pre1 slabs of ONE array: S6's begin where S5's end
                assert s6["views"][1] == dict(area=1, off=p["ns_h1"] * s5["views"][2]["stride"], n=p["ns_pre1"], stride=s5["views"][2]["stride"]), at
            if s5["replan"]:
                assert mode == 2 and c["h2_first"] and s5["nprob"] == 2 and p["ns_h1"] == 0, at
                replans.append(at)
            elif mode == 2 and c["h2_first"]:
                assert s5["nprob"] == 4 and p["ns_h1"] >= 1, at
    print(f"{len(replans)} cases reach the re-plan (ns_h1 + ns_pre1 > {MAX_SLABS}):")
    for r in replans:
        print("  " + r)
    print("slab counts seen:", sorted(counts))
    assert replans, "no case reached the re-plan of S5 / S6"
    assert counts == set(range(0, MAX_SLABS + 1))       # (0: the launches that are not made)


def test_an_area_one_float_too_small_is_refused_by_name(cases):
    for c in cases:
        for l in c["launches"]:
            at = where(c, l)
            holding = [a for a in l["areas"].values() if a["used"] > 0]
            assert not l["accepted"] and len(l["refused"]) == len(holding), at
            assert all(r.startswith(l["name"] + ": slab group ") and " ends at " in r for r in l["refused"]), at
            assert (l["nprob"] == 0) == (not holding), at
