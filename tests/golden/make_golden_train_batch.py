"""Golden vectors for the ordering models' training batches: outputs of the REFERENCE's own loops on seeded inputs.

    python tests/golden/make_golden_train_batch.py          (build container only: reads /root/reference)

The two training scripts cannot be imported (they parse arguments, open datasets and train at import time), so the loop bodies that
build the batches are taken out of the files at run time, located by their first and last statements, and executed as they stand on
torch tensors:
  coco_scripts/train_region_sort.py   from `index = 0` to the `index += 1` line           -> batch_verb, batch_det_sr, batch_gt_sr
  coco_scripts/train_sinkhorn.py      from `for i in range(detections.size(0))` up to the `tr_matrix = sinkhorn_net(` line, with a stub
                                      sinkhorn_net that records this_sr_perm, tr_locs, gt_locs_ and the key (i, idx, verb, sr) per call
Only inputs and outputs are stored (g18_train_batch.npz); nothing of the reference's text is.

Inputs: 3 images x 3 caption rows, L = Lg = 10, MV = 3, MS = 4, idx_list a permutation of range(10) per caption, feature rows of D = 8
(vis 4, txt 2, pos 2), every row distinct and non-zero, so that the stored this_sr_perm identifies the gathered slots.  The corners
the device path must get right are built in by hand and asserted below on the reference's own outputs."""
import json
import os
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
N_IMG, N_CAPS, L, MV, MS, SINK = 3, 3, 10, 3, 4, 10


def block(path, first, last):
    lines = open(os.path.join(REF, path)).read().split("\n")
    a = [i for i, l in enumerate(lines) if l.strip().startswith(first)][0]
    b = [i for i, l in enumerate(lines) if i > a and l.strip().startswith(last)][0]
    return compile(textwrap.dedent("\n".join(lines[a:b + 1])), "%s:%d-%d" % (path, a + 1, b + 1), "exec")


def make_inputs():
    rng = np.random.RandomState(18)
    N = N_IMG * N_CAPS
    cv = np.zeros((N, MV), np.int64)
    dv = np.zeros((N, L, MV), np.int64)
    dsr = np.zeros((N, L, MS), np.int64)
    # 0: no verb at all; its slots still carry a verb of another caption
    dv[0, :3, 0], dsr[0, :3, 0] = 40, [1, 2, 1]
    # 1: [v, 0, w]: w is never a job although it matches
    cv[1] = [41, 0, 42]
    dv[1, :4, 0], dsr[1, :4, 0] = 41, [3, 1, 3, 2]
    dv[1, :4, 2], dsr[1, :4, 2] = 42, [5, 5, 6, 6]
    # 2: the first verb matches nothing (`continue`), the two behind it are jobs
    cv[2] = [43, 44, 45]
    dv[2, 0:5, 1], dsr[2, 0:5, 1] = 44, [1, 4, 1, 4, 6]
    dv[2, 5:9, 0], dsr[2, 5:9, 0] = 45, [2, 3, 2, 7]
    # 3: one verb in columns 0 and 1 of every slot: the 10th distinct role arrives in slot 5, matches (a new role and repeats) follow
    cv[3] = [46, 0, 0]
    dv[3, :, 0:2] = 46
    dsr[3, :, 0:2] = [[1, 2], [3, 4], [5, 1], [6, 7], [8, 9], [10, 11], [1, 12], [2, 2], [13, 3], [4, 4]]
    # 4: a role seen three times and a second repeated role: the items {2, 5}
    cv[4] = [47, 48, 0]
    dv[4, :7, 0], dsr[4, :7, 0] = 47, [2, 5, 2, 5, 2, 3, 7]
    dv[4, 7:, 1], dsr[4, 7:, 1] = 48, [1, 1, 9]
    # 5: slot 3 carries the verb in two columns with one role: the slot twice in one list
    cv[5] = [49, 50, 0]
    dv[5, 3, 0], dsr[5, 3, 0] = 49, 4
    dv[5, 3, 2], dsr[5, 3, 2] = 49, 4
    dv[5, 6, 0], dsr[5, 6, 0] = 49, 8
    dv[5, :3, 1], dsr[5, :3, 1] = 50, [6, 3, 6]
    # 6: gt will have fewer roles than det; 7: gt will have a role det lacks
    cv[6] = [51, 0, 0]
    dv[6, :5, 0], dsr[6, :5, 0] = 51, [1, 2, 3, 2, 4]
    cv[7] = [52, 53, 0]
    dv[7, :4, 0], dsr[7, :4, 0] = 52, [5, 6, 5, 7]
    dv[7, 4:8, 1], dsr[7, 4:8, 1] = 53, [2, 3, 4, 3]
    # 8: three verbs, seeded noise in all columns
    cv[8] = [54, 10055, 56]
    for j in range(L):
        for k in range(MV):
            if rng.rand() < 0.7:
                dv[8, j, k], dsr[8, j, k] = cv[8, rng.randint(0, 3)], rng.randint(1, 6)
    dsr[:, :, 3] = rng.randint(1, 26, size=(N, L))                                  # the column beyond MV is never read
    idx = np.stack([rng.permutation(L) for _ in range(N)]).astype(np.int64)
    # gt: the det rows in their ground-truth positions ...
    gv, gsr = np.zeros_like(dv), np.zeros_like(dsr)
    for n in range(N):
        gv[n, idx[n]], gsr[n, idx[n]] = dv[n], dsr[n]
    gv[6][(gv[6] == 51) & (gsr[6, :, :MV] == 3)] = 0                                 # ... 6: role 3 is missing from gt
    gsr[7, :, :MV][(gv[7] == 53) & (gsr[7, :, :MV] == 4)] = 21                       # ... 7: role 21 instead of 4
    feats = np.maximum(rng.rand(N, L, 8), 0.05).astype(np.float32)
    feats[:, :, 0] = (np.arange(N * L).reshape(N, L) + 1)                            # every row distinct and non-zero
    return cv, dv, dsr, gv, gsr, idx, feats


def main():
    cv, dv, dsr, gv, gsr, idx, feats = make_inputs()
    N = N_IMG * N_CAPS
    img = lambda x: torch.from_numpy(x.reshape((N_IMG, N_CAPS) + x.shape[1:]))
    env = dict(torch=torch, device="cpu", detections=torch.zeros(N_IMG, 4, 8), control_verb=img(cv), det_seqs_v=img(dv), det_seqs_sr=img(dsr), gt_seqs_v=img(gv),
               gt_seqs_sr=img(gsr))
    exec(block("coco_scripts/train_region_sort.py", "index = 0", "index += 1"), env)
    ref_verbs, ref_det, ref_gt = (env[k].numpy() for k in ("batch_verb", "batch_det_sr", "batch_gt_sr"))

    records = []
    env = dict(torch=torch, device="cpu", detections=torch.zeros(N_IMG, 4, 8), control_verb=img(cv), det_seqs_v=img(dv), det_seqs_sr=img(dsr), gt_seqs_v=img(gv),
               gt_seqs_sr=img(gsr), idx_list=img(idx), det_seqs_vis=img(feats[..., :4]), det_seqs_txt=img(feats[..., 4:6]), det_seqs_pos=img(feats[..., 6:]),
               det_seqs_all=img(feats), sinkhorn_len=SINK)

    def sinkhorn_net(x):
        records.append(dict(perm=x[0].numpy().copy(), tr=env["tr_locs"].numpy().copy(), gt=env["gt_locs_"].numpy().copy(),
                            key=(int(env["i"]), int(env["idx"]), int(env["verb"]), int(env["sr"])), need=list(env["need_re_rank"]),
                            longest=max(len(v) for v in env["sr_find"].values())))
        return torch.zeros(SINK, SINK)
    env["sinkhorn_net"] = sinkhorn_net
    exec(block("coco_scripts/train_sinkhorn.py", "for i in range(detections.size(0))", "tr_matrix = sinkhorn_net("), env)

    # ---- the corners, asserted on the inputs and on what the reference made of them
    keys = np.array([r["key"] for r in records])
    cap = keys[:, 0] * N_CAPS + keys[:, 1]
    rows = {}                                                                       # (caption, verb) -> row of the S-SSP batch, in loop order
    for n in range(N):
        for verb in cv[n]:
            if verb == 0:
                break
            if (dv[n] == verb).any():
                rows[(n, int(verb))] = len(rows)
    assert len(rows) == len(ref_verbs) and [v for (_, v) in rows] == ref_verbs.tolist()
    assert not cv[0].any() and 0 not in [n for n, _ in rows]                                             # a caption with no verb
    assert cv[1, 1] == 0 and cv[1, 2] != 0 and (dv[1] == cv[1, 2]).any() and (1, int(cv[1, 2])) not in rows   # a zero verb in column 1, a non-zero one behind it
    assert not (dv[2] == cv[2, 0]).any() and (2, 44) in rows and (2, 45) in rows                         # a verb with no match; later columns count
    r = rows[(3, 46)]
    assert np.count_nonzero(ref_det[r]) == 10 and ref_det[r].tolist() == list(range(1, 11))              # 10 distinct roles ...
    assert (dv[3] == 46).sum() == 20 and len(np.unique(dsr[3, :, :2])) > 10                              # ... with matches after them
    it = [x for x in records if x["key"][:3] == (1, 0, 46)]
    assert [x["key"][3] for x in it] == [1] and it[0]["tr"][:3].tolist() == [0.0, 2.0, 10.0]             # a repeat behind the gate joins no list
    it = {x["key"][3]: x for x in records if x["key"][:3] == (1, 1, 47)}
    assert sorted(it) == [2, 5] and it[2]["tr"][:4].tolist() == [0.0, 2.0, 4.0, 10.0]                    # a role seen three times; two repeated roles
    it = [x for x in records if x["key"][:3] == (1, 2, 49)]
    assert len(it) == 1 and it[0]["tr"][:3].tolist() == [3.0, 3.0, 10.0] and (it[0]["perm"][0] == it[0]["perm"][1]).all()   # one slot, two columns
    r = rows[(6, 51)]
    assert np.count_nonzero(ref_gt[r]) < np.count_nonzero(ref_det[r])                                    # gt with fewer roles than det
    r = rows[(7, 53)]
    assert 21 in ref_gt[r] and 21 not in ref_det[r]                                                      # gt with a role det lacks
    assert any(len(x["need"]) >= 2 for x in records)
    for x in records:                                                                                    # the set order and the ascending order coincide
        assert x["need"] == sorted(x["need"]) and x["longest"] <= SINK                                   # no list exceeds sinkhorn_len
    for n in sorted(set(cap.tolist())):                                                                  # verbs distinct per caption: the key's verb names its column
        assert len(set(cv[n][cv[n] != 0].tolist())) == np.count_nonzero(cv[n])
    order = [(c, cv[c].tolist().index(k[2]), k[3]) for c, k in zip(cap.tolist(), keys)]
    assert order == sorted(order) and len(set(order)) == len(order)                                      # captions, verb columns, ascending role
    flat = feats.reshape(N * L, 8)
    assert len(np.unique(flat, axis=0)) == N * L and (np.abs(flat).sum(1) > 0).all()
    for n in range(N):
        assert sorted(idx[n].tolist()) == list(range(L))

    meta = dict(n_img=N_IMG, n_caps=N_CAPS, L=L, Lg=L, MV=MV, MS=MS, n_sink=SINK, D=8, seed=18, n_seqs=len(ref_verbs), n_items=len(records))
    out = dict(meta=np.array(json.dumps(meta)), control_verb=cv.astype(np.int32), det_seqs_v=dv.astype(np.int32), det_seqs_sr=dsr.astype(np.int32),
               gt_seqs_v=gv.astype(np.int32), gt_seqs_sr=gsr.astype(np.int32), idx_list=idx.astype(np.int32), seqs_perm=feats,
               ref_verbs=ref_verbs, ref_det_roles=ref_det, ref_gt_roles=ref_gt, ref_sr_perm=np.stack([r["perm"] for r in records]).astype(np.float32),
               ref_tr_locs=np.stack([r["tr"] for r in records]).astype(np.float32), ref_gt_locs=np.stack([r["gt"] for r in records]).astype(np.float32),
               ref_keys=keys.astype(np.int64))
    path = os.path.join(HERE, "g18_train_batch.npz")
    np.savez_compressed(path, **out)
    print("g18_train_batch.npz: %d sequences, %d items, %d bytes" % (len(ref_verbs), len(records), os.path.getsize(path)))


if __name__ == "__main__":
    main()
