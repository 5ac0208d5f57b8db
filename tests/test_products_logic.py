"""csrc/products.h, the planning half of the dense-product path (plan_products), on the CPU: tools/products_host.hip is built into a temp
dir and asked to plan launches on a GemmState of 256 CUs, in the exact flavour (x3_on = false, the ordering models') and in f32x3.  What is
held: what is refused, when a launch is written in place, and how the slabs of the others are placed in the scratch.  The slab counts are
those of the planners (gemm_grouped.h) at the commit that introduced this path."""
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

FLAVOURS = (("exact", 0), ("f32x3", 1))
BIG = 10_000_000


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("vsr_build", os.path.join(ROOT, "vsr-guided-cic_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build_products_tool(out=str(tmp_path_factory.mktemp("products") / "products_host"), force=True)


def seg(K, lda=None, ldw=None, a_off=0, a_img=0):
    return (K, K if lda is None else lda, K if ldw is None else ldw, a_off, a_img)


def prod(M, N, segs, in_place=1, bias=0, keep=0, relu_y=0, ldo=0):
    return dict(M=M, N=N, segs=segs, in_place=in_place, bias=bias, keep=keep, relu_y=relu_y, ldo=ldo)


def plan(tool, x3, prods, scratch=BIG, h2=0):
    words = [x3, h2, scratch, len(prods)]
    for p in prods:
        words += [p["M"], p["N"], len(p["segs"]), p["in_place"], p["bias"], p["keep"], p["relu_y"], p["ldo"]]
        for s in p["segs"]:
            words += list(s)
    res = subprocess.run([tool], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    line = res.stdout.strip()
    assert "\n" not in line
    if line.startswith("refused "):
        return dict(refused=line[len("refused "):])
    head, *rest = line.split(" | ")
    h = head.split()
    assert h[0] == "ok" and len(rest) == len(prods)
    out = dict(refused=None, ns=int(h[2]), in_place=bool(int(h[4])), prods=[])
    for r in rest:
        w = r.split()
        d = {w[i]: w[i + 1] for i in range(0, len(w), 2)}
        out["prods"].append(dict(c_is_out=bool(int(d["c_is_out"])), ldc=int(d["ldc"]), stride=int(d["stride"]), nslab=int(d["nslab"]), off=int(d["off"]),
                                 finish=d["finish"]))
    return out


@pytest.mark.parametrize("name,x3", FLAVOURS)
def test_one_slab_is_written_in_place(tool, name, x3):
    r = plan(tool, x3, [prod(3, 8, [seg(16)], ldo=12)])
    assert r["refused"] is None and r["ns"] == 1 and r["in_place"]
    assert r["prods"] == [dict(c_is_out=True, ldc=12, stride=0, nslab=1, off=0, finish="none")]
    # compact destination: ldo 0 = N
    assert plan(tool, x3, [prod(3, 8, [seg(16)])])["prods"][0]["ldc"] == 8
    # not allowed in place: one slab through the scratch and the plain finish
    r = plan(tool, x3, [prod(3, 8, [seg(16)], in_place=0)])
    assert r["ns"] == 1 and not r["in_place"]
    assert r["prods"] == [dict(c_is_out=False, ldc=8, stride=24, nslab=1, off=0, finish="k_prod_finish<false,FIN_NONE>")]
    # two products, one of which does not allow it: neither is in place
    r = plan(tool, x3, [prod(3, 8, [seg(16)]), prod(3, 8, [seg(16)], in_place=0)])
    assert r["ns"] == 1 and not r["in_place"] and [p["off"] for p in r["prods"]] == [0, 24]


@pytest.mark.parametrize("name,x3", FLAVOURS)
def test_refusals(tool, name, x3):
    ok = prod(3, 8, [seg(16)])
    assert plan(tool, x3, [ok])["refused"] is None
    assert "in-place" in plan(tool, x3, [prod(3, 8, [seg(16)], bias=1)])["refused"]
    assert plan(tool, x3, [prod(3, 8, [seg(16)], in_place=0, bias=1)])["prods"][0]["finish"] == "k_prod_finish<true,FIN_NONE>"
    assert "keep or relu_y" in plan(tool, x3, [prod(3, 8, [seg(16)], in_place=0, keep=1, relu_y=1)])["refused"]
    assert plan(tool, x3, [prod(3, 8, [seg(16)], in_place=0, keep=1)])["prods"][0]["finish"] == "k_prod_finish<true,FIN_KEEP>"
    assert plan(tool, x3, [prod(3, 8, [seg(16)], in_place=0, relu_y=1)])["prods"][0]["finish"] == "k_prod_finish<true,FIN_RELU_Y>"
    assert "16-byte" in plan(tool, x3, [prod(3, 8, [seg(16, lda=6)])])["refused"]
    assert "16-byte" in plan(tool, x3, [prod(3, 8, [seg(16, a_off=4)])])["refused"]
    assert plan(tool, x3, [prod(3, 8, [seg(16, a_off=16)])])["refused"] is None
    assert plan(tool, x3, [ok] * 4)["refused"] is None
    assert "products in one launch" in plan(tool, x3, [ok] * 5)["refused"]
    assert "products in one launch" in plan(tool, x3, [])["refused"]
    # an A operand that exists only as an fp16-pair image needs the all-DMA kernel, which a state without the f16x2 flavour never routes to
    assert "all-DMA" in plan(tool, x3, [prod(3, 8, [seg(16, a_img=1)])], h2=0)["refused"]


@pytest.mark.parametrize("name,x3,tight", [("exact", 0, [8, 2]), ("f32x3", 1, [8, 1])])
def test_slabs_are_placed_compactly_in_the_order_given(tool, name, x3, tight):
    prods = [prod(64, 64, [seg(4096)]), prod(64, 64, [seg(64)])]
    r = plan(tool, x3, prods)
    assert r["refused"] is None and r["ns"] == 8 and not r["in_place"]
    assert [p["nslab"] for p in r["prods"]] == tight
    end = 0
    for p, q in zip(prods, r["prods"]):
        assert not q["c_is_out"] and q["ldc"] == p["N"] and q["stride"] == p["M"] * p["N"] and q["finish"] == "k_prod_finish<false,FIN_NONE>"
        assert q["off"] == end                       # consecutive: disjoint, nothing between them
        end += p["M"] * p["N"] * q["nslab"]
    assert end == 64 * 64 * sum(tight) <= BIG
    assert plan(tool, x3, prods, scratch=end)["refused"] is None
    assert "scratch too small" in plan(tool, x3, prods, scratch=end - 1)["refused"]
    # the other order: the regions follow the products
    r = plan(tool, x3, prods[::-1])
    assert [p["nslab"] for p in r["prods"]] == tight[::-1] and [p["off"] for p in r["prods"]] == [0, 64 * 64 * tight[1]]


@pytest.mark.parametrize("name,x3,ns", [("exact", 0, 4), ("f32x3", 1, 6)])
def test_split_tiles_take_the_slab_path_even_when_in_place_is_allowed(tool, name, x3, ns):
    r = plan(tool, x3, [prod(256, 160, [seg(584)], in_place=1, ldo=200)])
    assert r["refused"] is None and r["ns"] == ns and not r["in_place"]
    assert r["prods"] == [dict(c_is_out=False, ldc=160, stride=256 * 160, nslab=ns, off=0, finish="k_prod_finish<false,FIN_NONE>")]
    assert "scratch too small" in plan(tool, x3, [prod(256, 160, [seg(584)])], scratch=256 * 160 * ns - 1)["refused"]
