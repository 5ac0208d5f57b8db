"""The kernels that turn logits into ids, on their own: tools/select_check launches k_vocab, k_select_beam<K> and k_backtrack on inputs
it builds itself (no library handle, no weights) and compares every output with a plain host reference.  All inputs are multiples of
1/8 of small magnitude, so every fp32 sum is exact, the ties are exactly the designed ones and no row is excluded: ids, parents,
gates, slots, masks and the copied floats must match bit for bit, log-probs within 2e-5 of an fp64 log-sum-exp.

vocab: V = 37 .. 12292 (256 / 512 threads, 16-byte and scalar loads, LDS row and global re-read) x K = 1..8 x 1..8 slabs, with rows
built to reach each candidate regime of the top-K tail (wave 0 alone, block rounds over the candidate list, full-row fallback) under
both threshold constructions, tie groups that include id 0 and id V - 1, VM_FULL / VM_FORCED / the gs row rule and the verb branch;
the tool itself fails when its inputs did not reach a required crossing.  beam: K = beam = 1..8, t = 0 and t > 0, cross-beam ties,
frozen streams.  backtrack: T in {1, 5, 20}, beam in {1, 5, 8}, out_size in {1, beam}, ties in seq, optional outputs null."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "select_check")


@pytest.mark.parametrize("group", ["vocab", "beam", "backtrack"])
def test_selection_kernels_against_host_reference(group):
    if not os.path.exists(TOOL):
        pytest.skip("tools/select_check not built (python vsr-guided-cic_amd/build.py --tool, or __graft_entry__.build())")
    r = subprocess.run([TOOL, group], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    failed = [ln for ln in lines if ln.endswith("FAIL") or ln.startswith("    ") or ln.startswith("HIP error")]     # (a failed case prints what was wrong above its line)
    report = "\n".join(failed[:40] + lines[-3:]) + r.stderr[-2000:]
    m = re.search(r"^(\d+) of (\d+) cases failed$", lines[-1] if lines else "")
    assert r.returncode == 0 and m and int(m.group(1)) == 0 and int(m.group(2)) > 0, report
