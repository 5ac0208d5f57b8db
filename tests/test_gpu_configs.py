"""GPU parity at the sizes BASELINE.json's configs name (everything through the reference-shaped class -> ctypes -> C ABI):
  configs[3]  XE step at batch 100, full dims (coco_scripts/train.py:103-113)        vs golden g1_xe_b100 (reference)
  configs[4]  SCST on 500 rows = 100 images x 5 samples (train.py:151-178)            vs golden g9_scst_500 (reference)
  fresh seeds (no arg-max margin search) at full size, greedy + beam-5                vs golden g10_fresh (reference)
  index-list regions == dense regions at the headline shapes
  step_v single-step vector with verb-forced rows (controllable_captioning.py:192-297) vs golden g6_step_v (reference)
and the input-contract / robustness cases the round-1 review asked for.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
import helpers
import vsr_oracle as vo
from vsrcap import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(meta, gains=None, table=None):
    cfg = meta["cfg"]
    w = helpers.weights_for(cfg, gains=gains, wseed=meta.get("wseed", 0))
    return helpers.build_model(cfg, w, DEV, bos=meta["bos"], verb_table=table), w


# ------------------------------------------------------------------ configs[3]: XE at batch 100, full size, fp32
def test_xe_step_batch100_full_size_vs_reference():
    """loss within 1e-4 (north star) and all 28 gradient norms within 2e-3 of the reference's autograd at B = 100."""
    meta, g = load_golden("g1_xe_b100")
    cfg = meta["cfg"]
    assert cfg["B"] == 100 and cfg["H"] == 1000 and cfg["V"] == 10000 and cfg["D"] == 2048
    m, _ = _model(meta, gains=meta["gains"])
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, meta["seed"])
    m.train()
    m.zero_grad()
    out, gate = m((det.to(DEV),), (caps.to(DEV), ctrl_seq.to(DEV)))
    loss, lc, lg = vo.xe_loss(out, gate, caps.to(DEV), gts.to(DEV))       # train.py:106-110 arithmetic (tests may use the oracle module)
    loss.backward()
    assert abs(loss.item() - g["losses"][0]) < 1e-4, (loss.item(), g["losses"])
    assert abs(lc.item() - g["losses"][1]) < 1e-4 and abs(lg.item() - g["losses"][2]) < 1e-4
    o, gt_ = out.detach().cpu(), gate.detach().cpu()
    np.testing.assert_allclose(gt_.numpy(), g["gate"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(o[:, :-1].gather(2, caps[:, 1:, None])[:, :, 0].numpy(), g["out_at_target"], atol=2e-5, rtol=0)
    np.testing.assert_array_equal(o.argmax(-1).numpy(), g["out_argmax"])
    grads = {k: p.grad for k, p in m.named_parameters()}
    gn = np.array([float(grads[k].double().norm()) for k in meta["param_order"]])
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=2e-3, atol=1e-8)
    gs = np.array([float(grads[k].double().sum()) for k in meta["param_order"]])
    np.testing.assert_allclose(gs, g["grad_sum"], rtol=5e-3, atol=5e-5)


def test_backward_is_bitwise_deterministic():
    """two forward+backward passes over the same batch give identical bits for all 28 gradients (no float atomics:
    the embedding gradient is a sorted segmented sum)."""
    meta, _ = load_golden("g1_xe_wide")
    cfg = meta["cfg"]
    m, _ = _model(meta, gains=meta["gains"])
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, meta["seed"])
    caps[:, 3] = caps[0, 3]            # repeated word ids inside the batch: several rows add into one embedding row
    caps[1] = caps[0]
    m.train()
    runs = []
    for _ in range(2):
        m.zero_grad()
        out, gate = m((det.to(DEV),), (caps.to(DEV), ctrl_seq.to(DEV)))
        vo.xe_loss(out, gate, caps.to(DEV), gts.to(DEV))[0].backward()
        runs.append({k: p.grad.clone() for k, p in m.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# ------------------------------------------------------------------ configs[4]: SCST on 500 rows
def test_scst_500_rows_replay_and_slice_gradients_vs_reference():
    """sample_rl on 100 images x 5 samples: (1) replaying the reference's 500 x 20 draws reproduces its log-probs to 1e-4;
    (2) the SCST backward on all 500 rows, with a non-zero advantage on rows 0..39 only, equals 40/500 x the reference's
    autograd gradients of the 40-row slice (rows are independent; train.py:174-175 averages over the batch)."""
    meta, g = load_golden("g9_scst_500")
    cfg = meta["cfg"]
    m, _ = _model(meta)
    det, ctrl = helpers.decode_inputs(cfg, meta["seed"])
    rep, n = meta["n_rep"], meta["n_slice"]
    det5 = det.repeat_interleave(rep, 0).contiguous().to(DEV)
    ctrl5 = ctrl.repeat_interleave(rep, 0).contiguous().to(DEV)
    assert det5.size(0) == 500
    fw, fg = torch.from_numpy(g["words"].astype(np.int64)), torch.from_numpy(g["gates"].astype(np.int64))
    with torch.no_grad():
        (sw, sg), (lw, lg) = m.sample_rl(det5, ctrl5, forced=(fw, fg))
    np.testing.assert_array_equal(sw.cpu().numpy(), fw.numpy())
    np.testing.assert_allclose(lw.cpu().numpy(), g["lp_w"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(lg.cpu().numpy(), g["lp_g"], atol=1e-4, rtol=0)
    # gradient path at 500 rows
    m.train()
    m.zero_grad()
    (_, _), (lw, lg) = m.sample_rl(det5, ctrl5, forced=(fw, fg))
    assert lw.requires_grad and lg.requires_grad
    reward = torch.zeros(500)
    base = torch.zeros(500)
    reward[:n] = torch.from_numpy(synth.hash_u01(n, *meta["reward_hash"]).astype(np.float32))
    base[:n] = torch.from_numpy(synth.hash_u01(n, *meta["baseline_hash"]).astype(np.float32))
    loss = vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV))
    loss.backward()
    scale = n / 500.0
    assert abs(loss.item() - scale * g["slice_loss"][0]) < 1e-4
    grads = {k: p.grad for k, p in m.named_parameters()}
    gn = np.array([float(grads[k].double().norm()) for k in meta["param_order"]])
    np.testing.assert_allclose(gn, scale * g["slice_grad_norm"], rtol=3e-3, atol=1e-9)


# ------------------------------------------------------------------ fresh seeds, no margin search
def test_fresh_seed_decode_full_size_vs_reference():
    """2 fresh seeds x 48 images at the headline dims: greedy rows whose fp64 arg-max margins are >= 1e-4 (words) /
    2e-3 (gates) and beam-5 rows on which the reference (fp32) and the fp64 oracle agree must match the reference's
    tokens exactly; the remaining rows are numerically ambiguous for any fp32 implementation and are reported."""
    meta, g = load_golden("g10_fresh")
    cfg = meta["cfg"]
    m, _ = _model(meta)
    report = []
    for seed in meta["seeds"]:
        det, ctrl = helpers.decode_inputs(cfg, seed)
        with torch.no_grad():
            gw, gg = m.test(det.to(DEV), ctrl.to(DEV))
            (bw, bg), _ = m.beam_search((det.to(DEV), ctrl.to(DEV)), meta["eos"], 5, 1)
        gw, gg, bw, bg = (x.cpu().numpy() for x in (gw, gg, bw, bg))
        marg = g["margins_%d" % seed]
        solid_g = (marg[:, :, 0].min(1) >= 1e-4) & (marg[:, :, 1].min(1) >= 2e-3) & g["greedy_agree64_%d" % seed].astype(bool)
        same_g = (gw == g["greedy_words_%d" % seed]).all(1) & (gg == g["greedy_gates_%d" % seed]).all(1)
        solid_b = g["beam_agree64_%d" % seed].astype(bool)
        same_b = (bw == g["beam_words_%d" % seed]).all(1) & (bg == g["beam_gates_%d" % seed]).all(1)
        report.append("seed %d: greedy %d/%d rows equal (%d solid), beam-5 %d/%d rows equal (%d solid)" %
                      (seed, same_g.sum(), len(same_g), solid_g.sum(), same_b.sum(), len(same_b), solid_b.sum()))
        assert same_g[solid_g].all(), "greedy mismatch on well-separated rows %s" % np.nonzero(~same_g & solid_g)[0]
        assert same_b[solid_b].all(), "beam-5 mismatch on rows the reference and fp64 agree on %s" % np.nonzero(~same_b & solid_b)[0]
        assert solid_g.mean() >= 0.8 and solid_b.mean() >= 0.8, "fixture lost its discriminating power"
        assert same_g.mean() >= 0.9 and same_b.mean() >= 0.9
    print("\n".join(report))


# ------------------------------------------------------------------ index lists == dense tensor at the headline shapes
def test_indexed_equals_dense_decode_full_size():
    from vsrcap.regions import IndexedRegions
    cfg = dict(V=10000, B=100, R0=36, R=36, D=2048, L=10, T=20, E=1000, H=1000, A=512)
    w = helpers.weights_for(cfg)
    m = helpers.build_model(cfg, w, DEV)
    det = torch.from_numpy(synth.make_detections(cfg["B"], cfg["R0"], cfg["D"], seed=77, min_valid=cfg["R0"])).to(DEV)
    idx = torch.from_numpy(synth.make_slot_indices(cfg["B"], cfg["L"], cfg["R"], cfg["R0"], seed=77)).to(DEV)
    reg = IndexedRegions(det, idx)
    dense = reg.dense().contiguous()
    with torch.no_grad():
        gi = m.test(det, reg)
        gd = m.test(det, dense)
        (bi, _) = m.beam_search((det, reg), [3, -1], 5, 1)
        (bd, _) = m.beam_search((det, dense), [3, -1], 5, 1)
    assert torch.equal(gi[0], gd[0]) and torch.equal(gi[1], gd[1])
    assert torch.equal(bi[0], bd[0]) and torch.equal(bi[1], bd[1])
    assert len(torch.unique(bd[0])) > 50


def test_indexed_prepare_with_bank_much_larger_than_the_slot_list():
    """n_img * Rb >> B * L * R: the hoisted att_va runs over the bank rows, whose split-K slabs must fit the workspace
    (round-1 advisor finding: they were sized by the slot entries only)."""
    from vsrcap.regions import IndexedRegions
    cfg = dict(V=120, B=16, R0=8, R=4, D=256, L=4, T=6, E=32, H=48, A=512)
    Rb = 100
    w = helpers.weights_for(cfg)
    m = helpers.build_model(cfg, w, DEV)
    det = torch.from_numpy(synth.make_detections(cfg["B"], cfg["R0"], cfg["D"], seed=3)).to(DEV)
    bank = torch.from_numpy(synth.make_detections(cfg["B"], Rb, cfg["D"], seed=4, min_valid=Rb)).to(DEV)
    idx = torch.from_numpy(synth.make_slot_indices(cfg["B"], cfg["L"], cfg["R"], Rb, seed=5)).to(DEV)
    reg = IndexedRegions(bank, idx)
    sentinel = torch.full((1 << 20,), 7.0, device=DEV)        # neighbours in the caching allocator: must stay untouched
    with torch.no_grad():
        (bi, _) = m.beam_search((det, reg), [3, -1], 3, 1)
        (bd, _) = m.beam_search((det, reg.dense().contiguous()), [3, -1], 3, 1)
    assert torch.equal(bi[0], bd[0]) and torch.equal(bi[1], bd[1])
    assert bool((sentinel == 7.0).all())


# ------------------------------------------------------------------ step_v single step
def test_step_v_single_step_vector():
    meta, g = load_golden("g6_step_v")
    cfg = meta["cfg"]
    m, _ = _model(meta, table=meta["verb_table"])
    det, ctrl = helpers.decode_inputs(cfg, meta["seed"])
    B, H = cfg["B"], cfg["H"]
    st = [torch.from_numpy((synth.hash_u01(B * H, 50 + i, 9).reshape(B, H) - 0.5).astype(np.float32)).to(DEV) for i in range(4)]
    k0 = torch.tensor(meta["k0"], device=DEV)
    prev = (torch.tensor(meta["prev_w"], device=DEV), torch.tensor(meta["prev_g"], device=DEV))
    verbs = torch.tensor(meta["verbs"], dtype=torch.float64, device=DEV)        # eval_coco.py:240 hands float64
    for flag in (False, True):
        with torch.no_grad():
            (lw, lg), (s1, s2, k1) = m.step_v(meta["t"], ((st[0], st[1]), (st[2], st[3]), k0), prev,
                                              (det.to(DEV), ctrl.to(DEV), verbs), None, mode="feedback", gt=flag)
        np.testing.assert_array_equal(k1.cpu().numpy(), g["k_gt%d" % flag])
        want_w, want_g = g["logp_w_gt%d" % flag], g["logp_g_gt%d" % flag]
        forced = (want_w == 0).sum(1) == 1
        assert forced.sum() == 3                                    # three verb-forced rows, one free row
        np.testing.assert_array_equal(lw.cpu().numpy()[forced], want_w[forced])        # exactly 0 / -1e6
        np.testing.assert_array_equal(lg.cpu().numpy()[forced], want_g[forced])        # exactly [-1e3, 0]
        np.testing.assert_allclose(lw.cpu().numpy()[~forced], want_w[~forced], atol=2e-5, rtol=0)
        np.testing.assert_allclose(lg.cpu().numpy()[~forced], want_g[~forced], atol=2e-5, rtol=0)
        np.testing.assert_allclose(s2[0].cpu().numpy(), g["h2_gt%d" % flag], atol=5e-6, rtol=0)


def test_greedy_with_verbs_equals_beam1_step_v():
    """test() with a third static runs the greedy loop over step_v: identical to beam_search_v with beam_size 1."""
    meta, _ = load_golden("g3_beam_small")
    cfg = meta["cfg"]
    m, _ = _model(meta, table=meta["verb_table"])
    det, ctrl = helpers.decode_inputs(cfg, meta["seed"])
    verbs = torch.from_numpy(synth.make_verbs(cfg["B"], cfg["L"], meta["nv"], seed=meta["seed"], p=meta["verb_p"])).to(DEV)
    with torch.no_grad():
        gw, gg = m._run_greedy((det.to(DEV), ctrl.to(DEV), verbs))
        (bw, bg), _ = m.beam_search_v((det.to(DEV), ctrl.to(DEV), verbs), meta["eos"], 1, 1, gt=False)
    assert torch.equal(gw, bw) and torch.equal(gg, bg)
    with pytest.raises(RuntimeError):
        m.beam_search_v((det.to(DEV), ctrl.to(DEV), verbs[:, :-1].contiguous()), meta["eos"], 3, 1)      # (B, L) contract


# ------------------------------------------------------------------ freeze branch: tokens, not only scores
def test_freeze_branch_tokens_and_logprobs():
    """eos on BOTH streams (CaptioningModel.py:143-150): frozen hypotheses emit word 0 / keep their score.  Tokens, gates,
    returned per-slot log-probs and final scores against the oracle (top-1 and runner-up)."""
    meta, _ = load_golden("g3_beam_small")
    cfg = meta["cfg"]
    m, w = _model(meta)
    o = vo.Oracle(w, cfg["T"], 2, as_written=False)
    det, ctrl = helpers.decode_inputs(cfg, meta["seed"])
    with torch.no_grad():
        gw, gg = o.test(det, ctrl)
    hit = 0
    for row, t in ((0, 2), (1, 4), (2, 1)):
        eos = [int(gw[row, t]), int(gg[row, t])]
        with torch.no_grad():
            (ow, og), (olw, olg), osc = o.beam_search(det, ctrl, eos, 3, 2, return_scores=True)
            eng = m._engine(torch.device(DEV))
            B = eng.prepare(det.to(DEV), ctrl.to(DEV), 3, m._weights_version())
            (w_, g_), (lw, lg), sc = eng.beam(B, torch.device(DEV), 3, 2, eos[0], eos[1])
        np.testing.assert_allclose(sc.cpu().numpy(), osc.numpy(), atol=1e-4, rtol=0)
        # Frozen hypotheses: every candidate of a frozen beam keeps the beam's score for word 0 with either gate, so the top-2
        # scores of such a row tie exactly and only differ in the gates AFTER the freeze (torch.sort breaks that tie
        # arbitrarily in the reference).  Well defined and compared: the top-1 WORDS of every row, the gates up to and
        # including the freezing step, and everything (gates, per-slot log-probs) on rows without a tie.
        sep = ((osc[:, 0] - osc[:, 1]).abs() > 1e-3).numpy()
        got_w, got_g = w_.cpu().numpy()[:, 0], g_.cpu().numpy()[:, 0]
        np.testing.assert_array_equal(got_w, ow.numpy()[:, 0])
        np.testing.assert_array_equal(got_g[sep], og.numpy()[sep, 0])
        np.testing.assert_allclose(lw.cpu().numpy()[sep, 0], olw.numpy()[sep, 0], atol=2e-4, rtol=0)
        np.testing.assert_allclose(lg.cpu().numpy()[sep, 0], olg.numpy()[sep, 0], atol=2e-4, rtol=0)
        both = (ow[:, 0] == eos[0]) & (og[:, 0] == eos[1])
        first = both.float().argmax(1)
        for b in range(cfg["B"]):
            if both[b].any() and first[b] + 1 < cfg["T"]:
                f = int(first[b])
                np.testing.assert_array_equal(got_g[b, :f + 1], og.numpy()[b, 0, :f + 1])
                frozen = bool((ow[b, 0, f + 1:] == 0).all())          # a frozen hypothesis keeps emitting word 0
                hit += int(frozen)
                if frozen:
                    assert (got_w[b, f + 1:] == 0).all()
    assert hit > 0, "no hypothesis was frozen: the test lost its subject"


# ------------------------------------------------------------------ input contracts (advisor findings)
# (two forwards then a backward of the first: raised in rounds 1-5, works since round 6 - tests/test_gpu_live_forwards.py)


def test_teacher_forcing_with_more_slots_than_steps():
    """forward() only needs ctrl_seq.size(1) >= captions.size(1) (CaptioningModel.py:30-32: step t reads slot t)."""
    cfg = dict(V=61, B=3, R0=6, R=5, D=128, L=9, T=9, E=32, H=48, A=16)
    w = helpers.weights_for(cfg)
    m = helpers.build_model(cfg, w, DEV)
    o = vo.Oracle(w, cfg["T"], 2, as_written=False)
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, 5)
    caps6 = caps[:, :6].contiguous()
    with torch.no_grad():
        oo, og = o.forward(det, caps6, ctrl_seq)
        out, gate = m((det.to(DEV),), (caps6.to(DEV), ctrl_seq.to(DEV)))
    assert out.shape == (3, 6, 61)
    np.testing.assert_allclose(out.cpu().numpy(), oo.numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(gate.cpu().numpy(), og.numpy(), atol=2e-4, rtol=0)
    m.train()
    m.zero_grad()
    out, gate = m((det.to(DEV),), (caps6.to(DEV), ctrl_seq.to(DEV)))
    vo.xe_loss(out, gate, caps6.to(DEV), gts[:, :6].to(DEV))[0].backward()
    for k in o.p:
        o.p[k].requires_grad_(True)
    oo, og = o.forward(det, caps6, ctrl_seq)
    vo.xe_loss(oo, og, caps6, gts[:, :6])[0].backward()
    for k, p in m.named_parameters():
        r = o.p[k].grad
        assert (p.grad.cpu() - r).abs().max().item() <= 2e-3 * (r.abs().max().item() + 1e-12) + 1e-9, k


def test_out_of_range_ids_are_clamped_and_reported():
    meta, _ = load_golden("g1_xe_small")
    cfg = meta["cfg"]
    m, _ = _model(meta, gains=meta["gains"])
    det, ctrl_seq, caps, _ = helpers.train_inputs(cfg, meta["seed"])
    bad = caps.clone()
    bad[0, 1] = -1                      # a padding id
    bad[2, 3] = cfg["V"] + 5            # beyond the vocabulary
    eng = m._engine(torch.device(DEV))
    eng.check_ids = True
    with torch.no_grad():
        with pytest.raises(IndexError, match="2 word"):
            m((det.to(DEV),), (bad.to(DEV), ctrl_seq.to(DEV)))
        out, _ = m((det.to(DEV),), (caps.to(DEV), ctrl_seq.to(DEV)))       # the counter was reset; clean ids pass
    assert torch.isfinite(out).all()


def test_prepare_cache_invalidation():
    """prepare() is skipped on an unchanged (data_ptr, _version) key; a .data write is invisible to it until invalidate_cache()."""
    meta, _ = load_golden("g3_beam_small")
    cfg = meta["cfg"]
    m, _ = _model(meta)
    det, ctrl = helpers.decode_inputs(cfg, meta["seed"])
    d, c = det.to(DEV), ctrl.to(DEV)
    d2, c2 = helpers.decode_inputs(cfg, meta["seed"] + 1)
    with torch.no_grad():
        a = m.test(d, c)
        want = m.test(d2.to(DEV), c2.to(DEV))
        m.test(d, c)
        d.data.copy_(d2)                 # no version bump
        c.data.copy_(c2)
        m.invalidate_cache()
        b = m.test(d, c)
    assert torch.equal(b[0], want[0]) and not torch.equal(a[0], b[0])


# ------------------------------------------------------------------ every GEMM kernel variant keeps token parity
@pytest.mark.parametrize("env", [dict(VSR_GEMM_TILE="64"), dict(VSR_GEMM_TILE="12864"), dict(VSR_GEMM_TILE="128"),
                                 dict(VSR_GEMM_R16_MAX="0"), dict(VSR_GEMM_R16_MAX="256"), dict(VSR_GEMM_R16_MAX="512"),
                                 dict(VSR_GEMM_SLOTS="384", VSR_GEMM_MIN_ITERS="4"),
                                 # round 6: the launch compositions / plans that are NOT the default stay token-exact too
                                 dict(VSR_SPLIT_PRE1="0"), dict(VSR_ATTEND_PARTS="1"), dict(VSR_XCD_GROUPS="1"),
                                 dict(VSR_H2_ALIGNED_MIN_SMALL="4"),
                                 # stream-K ranges so short that the split composition of S5 / S6 does not fit pre1's 8 slabs in the exact-fp32
                                 # flavour (3-4 slabs for the h1 pair + 8 for the h2 part at all three shapes): run_step falls back to round 5's
                                 dict(VSR_GEMM_SLOTS_SMALL="4096", VSR_GEMM_SLOTS_R16="2048", VSR_GEMM_MIN_ITERS="4")])
def test_gemm_kernel_variants_keep_token_parity(env, monkeypatch):
    """The tile / kernel overrides read by vsr_create (64x64, 128x64, 128x128 tiles of the 32x32x2 kernel; the rows-16
    16x16x4 kernel up to 0 / 256 / 512 rows; other stream-K grids) change the summation order, never the tokens: greedy on
    40 rows and beam-5 on 24 rows of the 256-sample reference fixture, plus the shard-sized batch of 13."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    meta, g = load_golden("g2_greedy")
    _, gb = load_golden("g3_beam")
    m, _ = _model(meta)                                  # a fresh model -> a fresh handle that reads the environment
    det, ctrl = helpers.decode_inputs(meta["cfg"], meta["seed"], n=40)
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    with torch.no_grad():
        w, gate = m.test(det, ctrl)
        w13, g13 = m.test(det[:13].contiguous(), ctrl[:13].contiguous())
        (bw, bg), _ = m.beam_search((det[:24].contiguous(), ctrl[:24].contiguous()), meta["eos"], 5, 1)
    np.testing.assert_array_equal(w.cpu().numpy(), g["words"][:40].astype(np.int64))
    np.testing.assert_array_equal(gate.cpu().numpy(), g["gates"][:40].astype(np.int64))
    np.testing.assert_array_equal(w13.cpu().numpy(), g["words"][:13].astype(np.int64))
    np.testing.assert_array_equal(g13.cpu().numpy(), g["gates"][:13].astype(np.int64))
    solid = gb["agree64"][:24].astype(bool)
    same = (bw.cpu().numpy() == gb["words"][:24]).all(1) & (bg.cpu().numpy() == gb["gates"][:24]).all(1)
    assert same[solid].all()
