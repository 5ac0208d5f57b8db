"""The ordering models' training batches built on the device: vsr_train_batch_plan / vsr_gather_rows through SspEngine and
vsrcap.trainbatch.build_device, held exactly to the reference's own outputs (tests/golden/g18_train_batch.npz) and to the numpy yardsticks
of vsrcap.trainbatch on the cases of tests/train_batch_ref.py (the ones tests/test_train_batch_logic.py runs through the host tool); the
losses of a device-built batch must have the bits of the same models fed the yardsticks' arrays."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
import train_batch_ref as tr
from vsrcap import synth, trainbatch as tb

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = tr.L
N_RANDOM = 200


def _np(x):
    return None if x is None else x.cpu().numpy()


def build(case, seqs_perm=None):
    return tb.build_device(DEV, seqs_perm=seqs_perm, n_sink=case.n_sink, n_verbs=tr.N_VERBS, max_items=case.max_items, **case.annotations())


def plan(case, device_inputs=False):
    ann = case.annotations()
    if device_inputs:
        ann = {k: None if v is None else torch.from_numpy(v.astype(np.int32)).to(DEV) for k, v in ann.items()}
    return tb._engine(DEV).train_batch_plan(n_sink=case.n_sink, n_verbs=tr.N_VERBS, max_items=case.max_items, **ann)


def check_case(case):
    """the padded tables of the plan call and the sliced tensors of build_device against host_tables"""
    exp = case.expected()
    tr.check(case, exp, {k: _np(v) for k, v in plan(case).items()})
    b = build(case)
    S, Q = (int(x) for x in exp["counts"][:2])
    assert (b.n_seqs, b.n_items, b.status_or, b.n_dropped) == tuple(int(x) for x in exp["counts"])
    assert b.verbs.dtype == torch.int64 and tuple(b.verbs.shape) == (S, 1) and b.det_roles.dtype == torch.int32
    sliced = dict(verbs=b.verbs[:, 0], det_roles=b.det_roles, gt_roles=b.gt_roles, item_gather=b.item_gather, tr_locs=b.tr_locs, gt_locs=b.gt_locs, item_key=b.item_key,
                  status=b.status)
    want = dict(exp, **{k: exp[k][:S] for k in ("verbs", "det_roles", "gt_roles")}, **{k: exp[k][:Q] for k in ("item_gather", "tr_locs", "gt_locs", "item_key")})
    tr.check(case, want, dict({k: _np(v) for k, v in sliced.items()}, counts=exp["counts"]))
    return b


def _models():
    from models import S_SSP, SinkhornNet
    meta, _ = load_golden("g11_ssp")
    w, ws = synth.make_ssp_weights(meta["seed"], meta["n_verbs"]), synth.make_sinkhorn_weights(meta["seed"])
    m = S_SSP()
    sd = m.state_dict()
    alias = {"encoder.sr_embed_layer.weight": "sr_embed_layer.weight", "decoder.embed_layer.weight": "sr_embed_layer.weight",
             "encoder.v_embed_layer.weight": "v_embed_layer.weight"}
    for k in sd:
        kk = alias.get(k, k)
        if kk in w:
            sd[k] = torch.from_numpy(w[kk])
    m.load_state_dict(sd)
    sh = SinkhornNet(10, 20, 0.1)
    sh.load_state_dict({k: torch.from_numpy(v) for k, v in ws.items()})
    return m.to(DEV).eval(), sh.to(DEV).eval()


def _train_case(N, MV, seed):
    """a loader batch of N captions with gt = the det rows in their ground-truth positions, and its feature rows (N, L, 2352)"""
    cv, dv, dsr, feats = synth.make_rank_batch(N, MV, seed)
    rng = np.random.RandomState(seed)
    idx = np.stack([rng.permutation(L) for _ in range(N)])
    gv, gsr = np.zeros_like(dv), np.zeros_like(dsr)
    for n in range(N):
        gv[n, idx[n]], gsr[n, idx[n]] = dv[n], dsr[n]
    return tr.Case(cv, dv, dsr, gv, gsr, idx, name="train"), feats


def _loss_and_grads(model, loss_fn):
    model.zero_grad(set_to_none=True)
    loss = loss_fn()
    assert loss.dim() == 0
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert grads
    return loss.detach().clone(), grads


def _same_bits(a, b):
    la, ga = a
    lb, gb = b
    assert la.view(torch.int32).item() == lb.view(torch.int32).item(), (la.item(), lb.item())
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), k


def test_fixture_of_the_reference_loops_exactly():
    """build_device on the fixture's annotations equals what the reference's loops made of them; seq at D = 8 through its distinct rows"""
    meta, g, c = tr.fixture_case()
    b = build(c, seqs_perm=torch.from_numpy(g["seqs_perm"]).to(DEV))
    assert (b.n_seqs, b.n_items, b.status_or, b.n_dropped) == (meta["n_seqs"], meta["n_items"], 0, 0) and not b.status.any()
    for got, key in ((b.verbs[:, 0], "ref_verbs"), (b.det_roles, "ref_det_roles"), (b.gt_roles, "ref_gt_roles")):
        assert tuple(got.shape) == g[key].shape
        np.testing.assert_array_equal(_np(got), g[key], err_msg=key)
    ref = tr.fixture_items(meta, g)
    keys = [tuple(k) for k in _np(b.item_key).tolist()]
    assert sorted(keys) == sorted(ref) and keys == sorted(keys)
    order = [list(map(tuple, g["ref_keys"].tolist())).index(k) for k in
             [(n // meta["n_caps"], n % meta["n_caps"], int(g["control_verb"][n, v]), sr) for n, v, sr in keys]]
    for got, key in ((b.seq, "ref_sr_perm"), (b.tr_locs, "ref_tr_locs"), (b.gt_locs, "ref_gt_locs")):
        assert got.dtype == torch.float32 and tuple(got.shape) == g[key].shape
        np.testing.assert_array_equal(_np(got), g[key][order], err_msg=key)
    np.testing.assert_array_equal(_np(b.item_gather), np.stack([ref[k][0] for k in keys]))


def test_seq_rows_at_2352_equal_index_select():
    _, g, c = tr.fixture_case()
    rows = torch.from_numpy(synth.hash_u01(c.N * L * 2352, 5, 3).astype(np.float32).reshape(c.N * L, 2352)).to(DEV)
    b = build(c, seqs_perm=rows.view(c.N, L, 2352))
    gather = torch.from_numpy(tb.sinkhorn_train_items(c.control_verb, c.det_seqs_v, c.det_seqs_sr, c.idx_list, c.n_sink)[0]).to(DEV)
    want = rows.index_select(0, gather.clamp(min=0).reshape(-1)).view(gather.size(0), c.n_sink, 2352) * (gather >= 0).unsqueeze(-1)
    assert (gather < 0).any() and tuple(b.seq.shape) == (21, 10, 2352)
    assert torch.equal(b.seq, want)


def test_named_corners_equal_the_yardsticks():
    by = {}
    for c in tr.special_cases():
        by[c.name] = check_case(c)
    assert by["all_inactive"].verbs.shape == (0, 1) and by["all_inactive"].tr_locs.shape == (0, 10) and by["no_idx"].tr_locs is None and by["no_gt"].gt_roles is None
    eng = tb._engine(DEV)
    z = lambda *s: np.zeros(s, np.int64)
    for kw in (dict(control_verb=z(1, 9), det_seqs_v=z(1, L, 9), det_seqs_sr=z(1, L, 9)), dict(control_verb=z(1, 2), det_seqs_v=z(1, 9, 2), det_seqs_sr=z(1, 9, 2)),
               dict(control_verb=z(1, 2), det_seqs_v=z(1, L, 2), det_seqs_sr=z(1, L, 2), idx_list=z(1, L), n_sink=17),
               dict(control_verb=z(1, 2), det_seqs_v=z(1, L, 2), det_seqs_sr=z(1, L, 2), idx_list=z(1, L), n_sink=1)):
        with pytest.raises(RuntimeError, match="limits"):
            eng.train_batch_plan(n_verbs=tr.N_VERBS, **kw)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        eng.gather_rows(torch.zeros(4, 6, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))


def test_random_cases_equal_the_yardsticks():
    """200 of the seeded cases of the CPU test (same generator, same seed), plus one of S = 320 job slots: the scan of k_tb_compact carries
    over a chunk of 256"""
    rng = np.random.RandomState(20261)
    cases = [tr.random_case(rng) for _ in range(N_RANDOM)] + [tr.random_case(rng, N=40, MV=8, n_sink=10)]
    assert cases[-1].N * cases[-1].MV > 256 and cases[-1].expected()["counts"][0] > 20
    for c in cases:
        check_case(c)


def test_ssp_loss_has_the_bits_of_the_yardstick_batch():
    ssp, _ = _models()
    c, _ = _train_case(4, 3, 3)
    verbs, det, gt = tb.ssp_train_batch(c.control_verb, c.det_seqs_v, c.det_seqs_sr, c.gt_seqs_v, c.gt_seqs_sr)
    assert len(verbs) >= 4
    b = tb.build_device(DEV, n_verbs=ssp.v_embed_layer.weight.shape[0], **c.annotations())
    assert b.n_seqs == len(verbs) and b.status_or == 0
    dev = lambda x: torch.from_numpy(x).to(DEV)
    want = _loss_and_grads(ssp, lambda: ssp(dev(verbs).unsqueeze(1), dev(det), dev(gt)))
    got = _loss_and_grads(ssp, lambda: tb.ssp_loss(ssp, b))
    _same_bits(got, want)


def test_sinkhorn_loss_has_the_bits_of_the_yardstick_items():
    _, sh = _models()
    c, feats = _train_case(2, 3, 3)
    gather, t, gl, _ = tb.sinkhorn_train_items(c.control_verb, c.det_seqs_v, c.det_seqs_sr, c.idx_list, 10)
    assert 1 <= len(gather) <= 8
    feats = torch.from_numpy(feats).to(DEV)
    b = tb.build_device(DEV, seqs_perm=feats, n_verbs=tr.N_VERBS, **c.annotations())
    assert b.n_items == len(gather)
    g = torch.from_numpy(gather).to(DEV)
    seq = (feats.reshape(-1, 2352)[g.clamp(min=0)] * (g >= 0).unsqueeze(-1)).contiguous()
    dev = lambda x: torch.from_numpy(x).to(DEV)
    want = _loss_and_grads(sh, lambda: sh.loc_loss(seq, dev(t), dev(gl), scale=1.0 / 2))
    got = _loss_and_grads(sh, lambda: tb.sinkhorn_loss(sh, b, 2))
    _same_bits(got, want)


def test_a_batch_without_an_active_job_trains_nothing():
    c = [c for c in tr.special_cases() if c.name == "all_inactive"][0]
    b = build(c, seqs_perm=torch.zeros(c.N, L, 2352, device=DEV))
    assert b.n_seqs == 0 and b.n_items == 0 and tuple(b.seq.shape) == (0, 10, 2352)

    class Boom:
        def __call__(self, *a, **k):
            raise AssertionError("a forward was launched")
        loc_loss = __call__
    assert tb.ssp_loss(Boom(), b) is None and tb.sinkhorn_loss(Boom(), b, 3) is None


def test_plan_call_is_free_of_synchronisation_and_build_device_reads_back_once():
    """Under torch.cuda.set_sync_debug_mode("error") SspEngine's two calls complete on device-resident inputs; under "warn" build_device
    reports exactly one synchronising operation: the read-back of counts.  (The mode sees torch-level synchronisation only; the library
    has none in these calls by construction: launches on the caller's stream, no read-back, no allocation.)"""
    c, feats = _train_case(4, 3, 3)
    rows = torch.from_numpy(feats).to(DEV).reshape(-1, 2352)
    ann = {k: torch.from_numpy(v.astype(np.int32)).to(DEV) for k, v in c.annotations().items()}
    eng = tb._engine(DEV)
    exp = c.expected()
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                               # noqa: BLE001
        pytest.skip("torch.cuda.set_sync_debug_mode is not supported by this torch build on ROCm: %s" % e)
    try:
        t = eng.train_batch_plan(n_sink=10, n_verbs=tr.N_VERBS, **ann)
        seq = eng.gather_rows(rows, t["item_gather"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    tr.check(c, exp, {k: _np(v) for k, v in t.items()})
    assert tuple(seq.shape) == (4 * 3 * L, 10, 2352) and not seq[int(exp["counts"][1]):].any()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            b = tb.build_device(DEV, seqs_perm=rows.view(4, L, 2352), n_verbs=tr.N_VERBS, **ann)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, syncs
    assert b.n_items == int(exp["counts"][1]) and torch.equal(b.seq, seq[:b.n_items])


def test_two_calls_write_identical_bytes():
    rng = np.random.RandomState(5)
    c = tr.random_case(rng, N=12, MV=3, n_sink=10)
    assert c.idx_list is not None and c.gt_seqs_v is not None
    eng = tb._engine(DEV)
    rows = torch.from_numpy(synth.hash_u01(c.N * L * 2352, 9, 1).astype(np.float32).reshape(c.N * L, 2352)).to(DEV)
    outs = []
    for fill in (0x00, 0xFF):
        junk = torch.full((8 << 20,), fill, dtype=torch.uint8, device=DEV)         # what the allocator hands out next holds another pattern each time
        del junk
        t = plan(c, device_inputs=True)
        if t["item_gather"] is not None:
            t["seq"] = eng.gather_rows(rows, t["item_gather"])
        outs.append({k: v.clone() for k, v in t.items() if v is not None})
    assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]) >= 5
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)), k
