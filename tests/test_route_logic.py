"""csrc/gemm_route.h on the CPU: the flavour rule (GemmState::flavour() and its predicates) and the registry of operand images
(OperandImages) as GemmBuilder::finish() reads them.  tools/route_host.hip is built into a temp dir; it drives a bare GemmState through
the registry calls of the entry points and routes one-segment launches of N = 4096 on it.  Three things are held:

(a) the predicate table, against the conjunctions of the three switches that the readers spelt out themselves before the rule had one
    owner (each written out below with the line it stood on);
(b) every launch and lookup of tests/golden/route_script.txt, against tests/golden/route_expected.txt: the output of the same script and
    the same tool body on the separate vectors and six lookup functions the registry replaced (profiles/r32_a_operand_images.md says how it
    was recorded);
(c) that the script reaches what it is there for: every kernel, both stale flags, every flavour and the two mixed switch states."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("vsr_build", os.path.join(ROOT, "vsr-guided-cic_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build_route_tool(out=str(tmp_path_factory.mktemp("route") / "route_host"), force=True)


def run(tool, script):
    res = subprocess.run([tool], input=script, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    return res.stdout


def fields(text):
    return {k: v for k, v in re.findall(r"(\w+)=(\S+)", text)}


@pytest.fixture(scope="module")
def table(tool):
    rows = []
    for line in run(tool, "table\n").splitlines():
        state, derived = line.split(" : ")
        assert state.startswith("state ")
        rows.append(({k: int(v) for k, v in fields(state).items()}, fields(derived)))
    return rows


def test_predicates_are_the_conjunctions_their_readers_spelt(table):
    assert len(table) == 8 * 2 * 2 and len({tuple(sorted(s.items())) for s, _ in table}) == 32
    for s, d in table:
        bf16_on, h2_on, x3_on, gemm_tile, h2_aimg = bool(s["bf16"]), bool(s["h2"]), bool(s["x3"]), s["tile"], bool(s["aimg"])
        want = {
            # gemm_route.h:239 finish() `h->bf16_on && ...`; train.inc.h:276 trans_dst and :1065 `h->bf16_on ? map16(..)`; vsrcap.hip:938
            # run_step `h->bf16_on && h->bf16_a16`; products.h:98 `!st.bf16_on`
            "bf16": bf16_on,
            # vsrcap.hip:1256 vsr_step `h->h2_on && !h->bf16_on && h->x3_on`
            "f16x2": h2_on and not bf16_on and x3_on,
            # gemm_route.h:265 finish() `h->h2_on && h->x3_on && k.gemm_tile == 0`; train.inc.h:1037 the backward's h2b has the same three
            # terms and `!h->bf16_on` (held below)
            "routes_f16x2": h2_on and x3_on and gemm_tile == 0,
            # train.inc.h:176 carve_train and gemm_route.h:299 finish() `h->h2_on && !h->bf16_on`
            "train_h2_images": h2_on and not bf16_on,
            # vsrcap.hip:937 run_step and train.inc.h:367 train_a_images `h->h2_on && !h->bf16_on && h->x3_on && h->gk.h2_aimg`
            "writes_h2_a_images": h2_on and not bf16_on and x3_on and h2_aimg,
            # vsrcap.hip:733 prepare_impl `h->h2_on`; train.inc.h:348, :388 the stash of what it measured
            "measures_h2_bounds": h2_on,
            # vsrcap.hip:647 vsr_adam_step `h->h2_on || h->bf16_on`
            "has_weight_images": h2_on or bf16_on,
        }
        assert {k: bool(int(d[k])) for k in want} == want, s
        # train.inc.h:1037: `h->h2_on && h->x3_on && h->gk.gemm_tile == 0 && !h->bf16_on` is now routes_f16x2() && !bf16()
        assert (bool(int(d["routes_f16x2"])) and not bool(int(d["bf16"]))) == (h2_on and x3_on and gemm_tile == 0 and not bf16_on)
        # the flavour: bf16 is offered first; f16x2 only together with x3_on; the knobs do not enter
        assert d["flavour"] == ("bf16" if bf16_on else "f32" if not x3_on else "f16x2" if h2_on else "f32x3"), s


@pytest.fixture(scope="module")
def routed(tool):
    with open(os.path.join(GOLDEN, "route_script.txt")) as f:
        return run(tool, f.read())


def test_launches_and_lookups_are_those_of_the_separate_vectors(routed):
    with open(os.path.join(GOLDEN, "route_expected.txt")) as f:
        want = f.read()
    got, want = routed.splitlines(), want.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    assert len(got) == len(want)


def test_the_script_reaches_what_it_is_for(routed, table):
    flavour_of = {(s["bf16"], s["h2"], s["x3"]): d["flavour"] for s, d in table}
    launches = [fields(line) for line in routed.splitlines() if line.startswith("launch ")]
    looks = [line for line in routed.splitlines() if line.startswith("look ")]
    assert len(launches) >= 20 and looks
    assert {l["kernel"] for l in launches} == {"F32", "F32_R16", "BF16W", "X3", "X3S", "H2", "H2S", "H2A", "B16A"}
    assert any(l["stale_w"] == "1" for l in launches) and any(l["stale_h2"] == "1" for l in launches)
    states = {(int(l["bf16"]), int(l["h2"]), int(l["x3"])) for l in launches}
    assert {flavour_of[s] for s in states} == {"f32", "f32x3", "f16x2", "bf16"}
    assert (1, 1, 1) in states and (0, 1, 0) in states            # both images on; h2_on with x3_on off
    # an address inside a weight AND inside a (stale) training range: the lookups prefer the weight's images, of either kind
    assert any(l.startswith("look w1+") and " h2=h2w+" in l and " slot=1 " in l and l.endswith("only_h2=1") for l in looks)
    assert any(l.startswith("look w1+") and " bf16=b16w+" in l and " only_bf16=1 " in l for l in looks)
    # an A operand inside a training range is not rewritten (the A lookup ignores those ranges) and the launch takes H2, not H2A
    assert any(l["kernel"] == "H2" and l["A"].startswith("t0+") for l in launches)
    # a W window that does not begin on a whole 8-element group of its range falls to f32x3 with fp32 operands
    assert any(l["kernel"] == "X3" and l["h2"] == "1" and l["W"] == "w0+16" for l in launches)
    # a_image_only keeps a short launch off the streaming kernel
    assert any(l["kernel"] == "H2A" and l["M"] == "65" for l in launches)
