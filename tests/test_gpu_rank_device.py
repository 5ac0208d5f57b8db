"""The eval loop's caption ranking on the device: vsr_rank_plan / vsr_rank_finish / vsr_rank_captions through
SspEngine, evalbatch.rank_captions_device, regions.reorder_slots_device and evalbatch.beam_search_v_ranked.

The integer stages are held exactly to the Python of vsrcap.evalbatch with injected decisions (tests/rank_ref.py, the cases of
tests/test_rank_logic.py); the whole call is held to the reference's per-caption flow re-enacted with the fp64 oracle networks under the
margin rule of tests/test_gpu_ssp.py::test_rank_captions_equals_the_per_caption_reference_flow (same generator, same weights, re-stated
here).  Counted on the CPU from the oracles alone: N = 40, MV = 3, RandomState(3): 19 of 40 captions decided by a margin > 1e-4, 80 jobs,
109 Sinkhorn items; N = 40, MV = 4, RandomState(5): 24 of 40, 104 jobs, 110 items; N = 12 (MV = 3, RandomState(3)): 4 of 12."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import helpers
import rank_ref as rr
import ssp_oracle as so
from vsrcap import evalbatch, regions, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = 10


def _weights():
    meta, _ = load_golden("g11_ssp")
    return meta, synth.make_ssp_weights(meta["seed"], meta["n_verbs"]), synth.make_sinkhorn_weights(meta["seed"])


def _models():
    from models import S_SSP, SinkhornNet
    meta, w, ws = _weights()
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


make_batch = synth.make_rank_batch          # the generator of tests/test_gpu_ssp.py's rank_captions test, kept in one place


def reference_flow(N, MV, seed):
    """the reference's loop structure, one caption at a time, on the fp64 oracle networks (CPU only): the batch, per caption its final
    rank (`want`) and whether every decision behind it is separated by more than 1e-4 (`safe`), the job and item counts"""
    from vsrcap.evalbatch import verb_rank_merge
    _, w, ws = _weights()
    o_ssp, o_sh = so.SSPOracle(w, dtype=torch.float64), so.SinkhornOracle(ws, dtype=torch.float64)
    control_verb, det_seqs_v, det_seqs_sr, feats = make_batch(N, MV, seed)
    want, safe, n_jobs, n_items = [], [], 0, 0
    for n in range(N):
        verb_ranks, margin = [], float('inf')
        for verb in control_verb[n]:
            if verb == 0:
                break
            roles = np.zeros(L, dtype=np.int64)
            find_sr, sr_find, need = 0, {}, set()
            for j in range(L):
                for k in range(MV):
                    if verb == det_seqs_v[n, j, k] and find_sr < 10:
                        sr = int(det_seqs_sr[n, j, k])
                        if sr not in sr_find:
                            sr_find[sr] = [j]; roles[find_sr] = sr; find_sr += 1
                        else:
                            sr_find[sr].append(j); need.add(sr)
            if find_sr == 0:
                continue
            n_jobs += 1
            with torch.no_grad():
                pred, _, mg = o_ssp.generate(np.array([verb]), roles[None], return_margin=True)
            margin = min(margin, float(mg[0]))
            sr_rank = {}
            for sr in need:
                n_items += 1
                item = np.zeros((1, 10, 2352), dtype=np.float64)
                for j, loc in enumerate(sr_find[sr]):
                    item[0, j] = feats[n, loc]
                with torch.no_grad():
                    tr_item = o_sh.forward(torch.from_numpy(item))
                    a = o_sh.assign(tr_item)[0]
                margin = min(margin, so.assignment_gap(tr_item[0].numpy(), len(sr_find[sr])))
                if sum(int(a[i]) >= len(sr_find[sr]) for i in range(len(sr_find[sr]))) >= 2:
                    margin = 0.0      # two filled rows paired with (identical) padding columns: their order is the solver's tie-break
                sr_rank[sr] = so.reorder_from_assignment(a, sr_find[sr])
            vr = []
            for sr in pred[0].numpy():
                if sr == 0:
                    break
                vr += list(sr_rank[int(sr)]) if len(sr_find[int(sr)]) != 1 else sr_find[int(sr)]
            verb_ranks.append(vr)
        final = verb_ranks[0] if verb_ranks else []
        for other in verb_ranks[1:]:
            final = verb_rank_merge(final, other)
        want.append([int(v) for v in final])
        safe.append(margin > 1e-4)
    return dict(control_verb=control_verb, det_seqs_v=det_seqs_v, det_seqs_sr=det_seqs_sr, feats=feats, want=want, safe=safe, n_jobs=n_jobs, n_items=n_items)


def _row(fr):
    fr = list(fr)[:L]
    return fr + [-1] * (L - len(fr))


@pytest.fixture(scope="module")
def nets():
    return _models()


@pytest.fixture(scope="module")
def flow40():
    """N = 40, MV = 3, RandomState(3): the oracle flow (computed once) and the device path's answer at the default max_items"""
    return reference_flow(40, 3, 3)


@pytest.fixture(scope="module")
def ranked40(nets, flow40):
    f = flow40
    with torch.no_grad():
        rank, status = evalbatch.rank_captions_device(nets[0], nets[1], f["control_verb"], f["det_seqs_v"], f["det_seqs_sr"], torch.from_numpy(f["feats"]).to(DEV))
    return rank.cpu().numpy(), status.cpu().numpy()


def test_plan_and_finish_with_injected_decisions_are_exact():
    """vsr_rank_plan -> random valid pred / assign -> vsr_rank_finish against the Python helper: every caption of the CPU test's special
    cases plus 40 random captions in one batch; job_verbs / job_roles / item_gather must equal the host loop's"""
    from vsrcap.ssp import SspEngine
    eng = SspEngine(DEV)
    rng = np.random.RandomState(11)
    cases = rr.special_cases() + [rr.random_case(rng, N=40, MV=3, n_sink=10), rr.random_case(rng, N=5, MV=8, n_sink=16),
                                 rr.random_case(rng, N=40, MV=8, n_sink=10)]          # S = 320 job slots: the scan of k_rank_items carries over a chunk of 256
    for c in cases:
        e = rr.expected(c, rng)
        plan, job_verbs, job_roles, gather = eng.rank_plan(c.control_verb, c.det_seqs_v, c.det_seqs_sr, n_sink=c.n_sink, n_verbs=rr.N_VERBS, max_items=c.max_items)
        np.testing.assert_array_equal(job_verbs.cpu().numpy(), e["job_verbs"], err_msg=c.name)
        np.testing.assert_array_equal(job_roles.cpu().numpy(), e["job_roles"], err_msg=c.name)
        np.testing.assert_array_equal(gather.cpu().numpy(), e["gather"], err_msg=c.name)
        rank, status = eng.rank_finish(plan, torch.from_numpy(e["pred"]).to(DEV), torch.from_numpy(e["assign"]).to(DEV), c.N, c.MV, max_items=c.max_items)
        np.testing.assert_array_equal(status.cpu().numpy(), e["status"], err_msg=c.name)
        np.testing.assert_array_equal(rank.cpu().numpy(), e["rank"], err_msg=c.name)
    with pytest.raises(RuntimeError, match="limits"):
        eng.rank_plan(np.zeros((1, 9), np.int64), np.zeros((1, L, 9), np.int64), np.zeros((1, L, 9), np.int64), n_sink=10, n_verbs=rr.N_VERBS)
    with pytest.raises(RuntimeError, match="limits"):
        eng.rank_plan(np.zeros((1, 2), np.int64), np.zeros((1, 9, 2), np.int64), np.zeros((1, 9, 2), np.int64), n_sink=10, n_verbs=rr.N_VERBS)
    with pytest.raises(RuntimeError, match="the plan was written for"):       # the kernel indexes assign with the plan's item bound
        eng.rank_finish(plan, torch.from_numpy(e["pred"]).to(DEV), torch.from_numpy(e["assign"][:7]).to(DEV), c.N, c.MV, max_items=7)
    with pytest.raises(RuntimeError, match="ONE engine"):
        eng.rank_captions(np.zeros((1, 2), np.int64), np.zeros((1, L, 2), np.int64), np.zeros((1, L, 2), np.int64), torch.zeros(1, L, 2352, device=DEV))


def test_whole_call_equals_the_per_caption_reference_flow(flow40, ranked40):
    """rank_captions_device against the reference's per-caption flow on the fp64 oracles: a caption whose every decision is separated by
    more than 1e-4 and that pairs no two filled rows with padding columns must match exactly; at least 15 of the 40 are such."""
    f, (rank, status) = flow40, ranked40
    print("safe %d of 40, jobs %d, items %d" % (sum(f["safe"]), f["n_jobs"], f["n_items"]))
    assert sum(f["safe"]) >= 15, f["safe"]
    assert (status == 0).all(), status
    for n in range(40):
        if f["safe"][n]:
            assert rank[n].tolist() == _row(f["want"][n]), (n, rank[n].tolist(), f["want"][n])
    assert ((rank >= 0).sum(1) > 3).any() and rank.min() >= -1 and rank.max() < L


def test_max_items_bound_and_overflow(nets, flow40, ranked40):
    """max_items equal to the batch's item count gives the default's ranks; one less sets bit 2 on exactly the captions that own the dropped
    (last) item and leaves every other row as it was"""
    f, (rank, status) = flow40, ranked40
    case = rr.Case(f["control_verb"], f["det_seqs_v"], f["det_seqs_sr"])
    jobs = rr.host_jobs(case)
    items, _ = rr.host_items(case, jobs)
    assert len(items) == f["n_items"] and len(jobs) == f["n_jobs"]
    feats = torch.from_numpy(f["feats"]).to(DEV)
    with torch.no_grad():
        r_eq, s_eq = evalbatch.rank_captions_device(nets[0], nets[1], f["control_verb"], f["det_seqs_v"], f["det_seqs_sr"], feats, max_items=len(items))
        r_lo, s_lo = evalbatch.rank_captions_device(nets[0], nets[1], f["control_verb"], f["det_seqs_v"], f["det_seqs_sr"], feats, max_items=len(items) - 1)
    np.testing.assert_array_equal(s_eq.cpu().numpy(), status)
    np.testing.assert_array_equal(r_eq.cpu().numpy(), rank)
    owner = jobs[items[-1][0]][0]
    want_status = np.zeros(40, np.int64)
    want_status[owner] = rr.ITEM_OVERFLOW
    np.testing.assert_array_equal(s_lo.cpu().numpy(), want_status)
    r_lo = r_lo.cpu().numpy()
    assert (r_lo[owner] == -1).all()
    keep = np.arange(40) != owner
    np.testing.assert_array_equal(r_lo[keep], rank[keep])


def test_status_bits(nets):
    """a caption with no job, one with role id 26 and one with a verb beyond the verb table each set their own bit and nothing else; the
    rows of the other captions are those of the same batch without the three defects (same shapes, same launches)"""
    cv, dv, dsr, feats = make_batch(6, 3, 9)
    feats = torch.from_numpy(feats).to(DEV)
    n_verbs = nets[0].v_embed_layer.weight.shape[0]

    def run(cv, dv, dsr):
        with torch.no_grad():
            r, s = evalbatch.rank_captions_device(nets[0], nets[1], cv, dv, dsr, feats)
        return r.cpu().numpy(), s.cpu().numpy()
    base_r, base_s = run(cv, dv, dsr)
    assert (base_s == 0).all()
    cv2, dv2, dsr2 = cv.copy(), dv.copy(), dsr.copy()
    dv2[1] = 0                                                           # caption 1: no slot carries any of its verbs
    first = np.argwhere(dv2[3] == cv2[3, 0])[0]
    dsr2[3, first[0], first[1]] = 26                                     # caption 3: a matched role id one past the table
    old = cv2[4, 0]
    cv2[4, 0] = n_verbs                                                  # caption 4: a verb one past the verb table (and below 10000)
    dv2[4][dv2[4] == old] = n_verbs
    assert n_verbs < 10000
    r, s = run(cv2, dv2, dsr2)
    assert s.tolist() == [0, rr.NO_JOB, 0, rr.BAD_ROLE, rr.BAD_VERB, 0]
    for n in (1, 3, 4):
        assert (r[n] == -1).all()
    for n in (0, 2, 5):
        np.testing.assert_array_equal(r[n], base_r[n])


def test_beam_search_v_ranked_equals_indexed_with_the_rank_copied_back(nets):
    """plumbing: beam_search_v_ranked == beam_search_v_indexed given the device rank tensor as lists (4 images x 3 captions, beam 3)"""
    meta, _ = load_golden("g3_beam_small")
    cfg = dict(meta["cfg"], L=L)             # the small config with its 5 slots per caption raised to S-SSP's 10 (L belongs to the inputs, not to the weights)
    m = helpers.build_model(cfg, helpers.weights_for(cfg, wseed=meta.get("wseed", 0)), DEV, bos=meta["bos"], verb_table=meta["verb_table"])
    n_img, caps = 4, 3
    N = n_img * caps
    det = torch.from_numpy(synth.make_detections(n_img, cfg["R0"], cfg["D"], seed=33)).to(DEV)
    idx = torch.from_numpy(synth.make_slot_indices(N, cfg["L"], cfg["R"], cfg["R0"], seed=33)).to(DEV)
    row_img = torch.arange(N, dtype=torch.int32, device=DEV) // caps
    cv, dv, dsr, feats = make_batch(N, 3, 3)
    feats = torch.from_numpy(feats).to(DEV)
    rng = np.random.RandomState(4)
    verb_list = np.where(rng.rand(N, L) > 0.7, rng.randint(0, meta["nv"], size=(N, L)), -1).astype(np.float64)
    with torch.no_grad():
        (w_r, g_r), _, status = evalbatch.beam_search_v_ranked(m, nets[0], nets[1], det, det, idx, row_img, cv, dv, dsr, feats, verb_list, meta["eos"], beam_size=3)
        rank, status2 = evalbatch.rank_captions_device(nets[0], nets[1], cv, dv, dsr, feats)
        lists = [[int(x) for x in row if x >= 0] for row in rank.cpu().numpy()]
        (w_i, g_i), _ = evalbatch.beam_search_v_indexed(m, det, det, idx, row_img, lists, verb_list, meta["eos"], beam_size=3)
    assert (status.cpu().numpy() == 0).all() and (status2.cpu().numpy() == 0).all() and any(len(r) > 3 for r in lists)
    np.testing.assert_array_equal(w_r.cpu().numpy(), w_i.cpu().numpy())
    np.testing.assert_array_equal(g_r.cpu().numpy(), g_i.cpu().numpy())
    # reorder_slots_device is reorder_slots' launch: same slots, same verbs, from the same rank
    eng = m._engine(torch.device(DEV))
    reg = regions.IndexedRegions(det, idx, row_img)
    a, va = regions.reorder_slots_device(eng, reg, rank, torch.from_numpy(verb_list).to(DEV))
    b, vb = regions.reorder_slots(eng, reg, lists, verb_list)
    np.testing.assert_array_equal(a.slot_idx.cpu().numpy(), b.slot_idx.cpu().numpy())
    np.testing.assert_array_equal(va.cpu().numpy(), vb.cpu().numpy())
    with pytest.raises(ValueError):
        regions.reorder_slots_device(eng, reg, rank.long(), verb_list)


def test_repeatable_and_free_of_torch_level_synchronisation(nets, flow40, ranked40):
    """Two calls return bit-identical rank / status, and with device-resident inputs the call completes under
    torch.cuda.set_sync_debug_mode("error").  That mode sees torch-level synchronisation only (.cpu(), .item(), blocking copies); the
    library has none in these calls by construction (launches on the caller's stream, no read-back, no allocation)."""
    f, (rank, status) = flow40, ranked40
    cv, dv, dsr = (torch.from_numpy(f[k].astype(np.int32)).to(DEV) for k in ("control_verb", "det_seqs_v", "det_seqs_sr"))
    feats = torch.from_numpy(f["feats"]).to(DEV)
    with torch.no_grad():
        r2, s2 = evalbatch.rank_captions_device(nets[0], nets[1], cv, dv, dsr, feats)
    np.testing.assert_array_equal(r2.cpu().numpy(), rank)
    np.testing.assert_array_equal(s2.cpu().numpy(), status)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                               # noqa: BLE001
        pytest.skip("torch.cuda.set_sync_debug_mode is not supported by this torch build on ROCm: %s" % e)
    try:
        with torch.no_grad():
            r3, s3 = evalbatch.rank_captions_device(nets[0], nets[1], cv, dv, dsr, feats)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    np.testing.assert_array_equal(r3.cpu().numpy(), rank)
    np.testing.assert_array_equal(s3.cpu().numpy(), status)
