"""tests/grad_compare.py on the CPU: the fp32 oracle stands in for the device, and four planted defects of the kind the routes of
tests/test_gpu_grad_routes.py can have must fail compare() at margin 16.  Each defect also states whether the project's older check
alone (2e-3 of max |ref|) would have let it pass: that is what the fp64 comparison adds, and that nothing it sees was hidden before.

The shape is the smallest with a decoder row 128: B = 129, everything else as the row ladder's base."""
import pytest
import torch
import torch.nn.functional as F

import grad_compare as gc
import helpers
from vsrcap import synth

CFG = dict(V=56, B=129, R0=6, R=6, D=64, L=3, T=3, E=32, H=64, A=32)
SEED = 23


@pytest.fixture(scope="module")
def case():
    w = helpers.weights_for(CFG, gains={k: 1.0 for k in synth.DEFAULT_GAINS})
    det, ctrl_seq, caps, gts = helpers.train_inputs(CFG, SEED)
    kw = dict(caps=caps, ctrl_seq=ctrl_seq)
    ref, yard = (gc.oracle_grads(w, CFG["T"], det, dt, gc.xe_loss_fn(caps, gts), **kw) for dt in (torch.float64, torch.float32))
    return dict(w=w, det=det, ctrl_seq=ctrl_seq, caps=caps, gts=gts, ref=ref, yard=yard)


def _planted(case, **changed):
    got = {k: v.clone() for k, v in case["yard"]["grads"].items()}
    got.update(changed)
    return got


def _verdicts(case, got, label):
    """(fails compare at margin 16, passes the older 2e-3-of-max check alone)"""
    old = not gc.over_ceiling(got, case["ref"]["grads"], 2e-3)
    try:
        gc.compare(got, case["ref"]["grads"], case["yard"]["grads"], label=label)
        return False, old
    except AssertionError as e:
        print(str(e).splitlines()[1].strip() if "\n" in str(e) else str(e))
        return True, old


def _slice_ratio(case, got, k):
    """metric (b) of one tensor over its yardstick, as compare() forms it"""
    b = gc.metrics(got[k], case["ref"]["grads"][k])[1]
    return b / max(gc.metrics(case["yard"]["grads"][k], case["ref"]["grads"][k])[1], gc.ULP_FLOOR / gc.MARGIN)


def test_oracle_grads_returns_fp64_and_the_fp32_run_is_close(case):
    ref, yard = case["ref"], case["yard"]
    assert len(ref["grads"]) == 28 and all(v.dtype == torch.float64 for v in yard["grads"].values())
    assert ref["logp_words"].shape == (CFG["B"], CFG["T"], CFG["V"]) and ref["logp_gates"].shape == (CFG["B"], CFG["T"], 2)
    gc.check_outputs(yard["loss"], yard["logp_words"], yard["logp_gates"], ref, "fp32 oracle")
    worst = max(gc.metrics(yard["grads"][k], ref["grads"][k])[0] for k in ref["grads"])
    print("fp32 oracle against fp64: worst max error / max |ref| %.2e" % worst)
    assert worst < 1e-5                                   # 24-bit arithmetic: two decades under the 2e-3 ceiling


def test_the_yardstick_passes_against_itself(case):
    worst = gc.compare(case["yard"]["grads"], case["ref"]["grads"], case["yard"]["grads"], label="fp32 oracle")
    assert worst["a"][0] == pytest.approx(1.0) and worst["b"][0] == pytest.approx(1.0)


def test_planted_bf16_block_in_lstm1_weight_ih(case):
    """one 16 x 16 block of lstm_cell_1.weight_ih's gradient recomputed from bf16-rounded values: every element of it moves by up to
    2^-9 of ITSELF, so the older check (2e-3 of the tensor's max) cannot see it"""
    g = case["yard"]["grads"]["lstm_cell_1.weight_ih"].clone()
    g[64:80, 32:48] = g[64:80, 32:48].float().bfloat16().double()
    assert not torch.equal(g, case["yard"]["grads"]["lstm_cell_1.weight_ih"])
    got = _planted(case, **{"lstm_cell_1.weight_ih": g})
    fails, old = _verdicts(case, got, "bf16 block")
    assert fails and old
    assert _slice_ratio(case, got, "lstm_cell_1.weight_ih") > gc.MARGIN       # the slice-wise metric sees it on its own


def test_planted_decoder_row_128_left_out_of_every_batch_sum(case):
    """rows 0 .. 127 only, the loss still divided as for 129 rows.  The older check sees this one too: an embedding row that only
    decoder row 128 reads loses its whole gradient"""
    caps, gts = case["caps"], case["gts"]
    n_cap, n_gate = caps[:, 1:].numel(), int((gts != -1).sum())

    def first_rows(n):
        def loss_fn(lw, lg):
            cap = F.nll_loss(lw[:, :-1].reshape(-1, CFG["V"]), caps[:n, 1:].reshape(-1), reduction="sum") / n_cap
            gate = F.nll_loss(lg.reshape(-1, 2), gts[:n].reshape(-1).long(), ignore_index=-1, reduction="sum") / n_gate
            return cap + 4 * gate
        return gc.oracle_grads(case["w"], CFG["T"], case["det"][:n], torch.float32, loss_fn, caps=caps[:n],
                               ctrl_seq=case["ctrl_seq"][:n])["grads"]
    fails, _ = _verdicts(case, first_rows(129), "all 129 rows, sums divided by hand")         # the construction itself is sound
    assert not fails
    fails, old = _verdicts(case, first_rows(128), "row 128 dropped")
    assert fails and not old


def test_planted_column_of_att_va_scaled(case):
    """one column of att_va.weight's gradient x 1.001: 1e-3 of the column's own elements, under the older ceiling by construction"""
    g = case["yard"]["grads"]["att_va.weight"].clone()
    g[:, 17] *= 1.001
    got = _planted(case, **{"att_va.weight": g})
    fails, old = _verdicts(case, got, "att_va column x 1.001")
    assert fails and old
    assert _slice_ratio(case, got, "att_va.weight") > gc.MARGIN               # the slice-wise metric sees it on its own


def test_planted_embedding_row_counts_one_occurrence_only(case):
    """the gradient of one embedding row whose id the batch reads more than once keeps its first occurrence only (a segmented sum
    that drops its tail): every later occurrence reads a copy of the row appended to the table, so autograd keeps them apart.
    Half of a row's gradient is missing, so the older check sees this one too"""
    caps, V = case["caps"], CFG["V"]
    counts = torch.bincount(caps.reshape(-1), minlength=V)
    v = int(torch.where(counts >= 2, counts, counts.max() + 1).argmin())
    where = (caps == v).nonzero()
    assert len(where) >= 2
    moved = caps.clone()
    for b, t in where[1:].tolist():
        moved[b, t] = V
    w = dict(case["w"])
    w["embed.weight"] = torch.cat([torch.as_tensor(w["embed.weight"]), torch.as_tensor(w["embed.weight"][v:v + 1])], 0)
    got = gc.oracle_grads(w, CFG["T"], case["det"], torch.float32, gc.xe_loss_fn(caps, case["gts"]), caps=moved, ctrl_seq=case["ctrl_seq"])
    e = case["yard"]["grads"]["embed.weight"].clone()
    total = got["grads"]["embed.weight"][v] + got["grads"]["embed.weight"][V]
    assert float((total - e[v]).abs().max()) <= 1e-5 * float(e[v].abs().max())         # the copy splits the row's gradient, no more
    e[v] = got["grads"]["embed.weight"][v]
    fails, old = _verdicts(case, _planted(case, **{"embed.weight": e}), "embedding row %d, 1 of %d occurrences" % (v, len(where)))
    assert fails and not old
