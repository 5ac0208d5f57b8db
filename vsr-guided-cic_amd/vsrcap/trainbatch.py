"""The ordering models' training batches: the step in front of S_SSP.forward and SinkhornNet.loc_loss.

The reference builds the inputs of its two training calls with five nested Python loops over tensor elements, once per loader batch
(coco_scripts/train_region_sort.py:133-179, coco_scripts/train_sinkhorn.py:144-205 and their Flickr twins).  Here that step exists twice:

  ssp_train_batch, sinkhorn_train_items   the HOST YARDSTICKS: a plain numpy transcription of those loops - what a port of the two scripts
                                          would write, and what the device path is held to (tests/test_train_batch_logic.py,
                                          tests/test_gpu_train_batch.py), as evalbatch.rank_captions is for the eval loop
  build_device                            the same tables from two launches (vsr_train_batch_plan; logic in csrc/train_batch_logic.h), one
                                          16-byte read-back of the counts, and the items' feature rows through vsr_gather_rows

All caption rows of the loader batch are flattened to N = images x captions; a JOB is one (caption row n, verb column v).  Two orders
that the reference leaves open are fixed here: the items of a job come in ascending role id (the reference iterates a
Python set; the loss is a sum, so only its rounding depends on that order), and gt_locs comes from the STABLE argsort (torch.argsort
without stable=True promises no tie order; with idx_list values distinct and < 10 no tie is ever read)."""
import numpy as np
import torch

L = 10                       # S-SSP's sequence length: slots per caption, roles per job
PAD_LOC = 10.0               # the padding of tr_locs / gt_locs: the literal of train_sinkhorn.py:191-193, whatever n_sink is
N_VERBS_COCO = 2663          # rows of S_SSP()'s verb table (models/sort_model.py)
BAD_ROLE, BAD_VERB, TRUNCATED, BAD_IDX = 4, 8, 32, 64
DROP_CAPTION = BAD_ROLE | BAD_VERB


# ---------------------------------------------------------------------------------------------- host yardsticks
def _first_sights(verb, seqs_v, seqs_sr):
    """roles of `verb` in order of first sight under the `find < 10` gate: seqs_v (Lx, MV), seqs_sr (Lx, MS)"""
    roles, found = np.zeros(L, dtype=np.int64), []
    for j in range(seqs_v.shape[0]):
        for k in range(seqs_v.shape[1]):
            if verb == seqs_v[j, k] and len(found) < 10 and int(seqs_sr[j, k]) not in found:
                found.append(int(seqs_sr[j, k]))
                roles[len(found) - 1] = seqs_sr[j, k]
    return roles, len(found)


def ssp_train_batch(control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v, gt_seqs_sr):
    """train_region_sort.py:133-179 over N caption rows: control_verb (N, MV), det_seqs_v (N, L, MV), det_seqs_sr (N, L, MS), gt_seqs_v
    (N, Lg, MV), gt_seqs_sr (N, Lg, MS) ints -> (verbs (S,), det_roles (S, 10), gt_roles (S, 10)) int64, one row per active job."""
    control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v, gt_seqs_sr = (np.asarray(x) for x in (control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v, gt_seqs_sr))
    verbs, det_roles, gt_roles = [], [], []
    for n in range(control_verb.shape[0]):
        for verb in control_verb[n]:
            if verb == 0:
                break
            det, find_sr = _first_sights(verb, det_seqs_v[n], det_seqs_sr[n])
            gt, _ = _first_sights(verb, gt_seqs_v[n], gt_seqs_sr[n])
            if find_sr == 0:
                continue
            verbs.append(int(verb))
            det_roles.append(det)
            gt_roles.append(gt)
    return (np.array(verbs, dtype=np.int64), np.array(det_roles, dtype=np.int64).reshape(-1, L), np.array(gt_roles, dtype=np.int64).reshape(-1, L))


def sinkhorn_train_items(control_verb, det_seqs_v, det_seqs_sr, idx_list, n_sink=10):
    """train_sinkhorn.py:144-205 over N caption rows: idx_list (N, L) = the ground-truth position of each slot -> (gather (Q, n_sink) int64 =
    n L + slot or -1, tr_locs (Q, n_sink) fp32, gt_locs (Q, n_sink) fp32, keys (Q, 3) int64 = (n, verb column, role)), one item per repeated
    role of an active job, roles ascending.  A slot list longer than n_sink is cut (train_sinkhorn_flickr.py's `j >= sinkhorn_len`)."""
    control_verb, det_seqs_v, det_seqs_sr, idx_list = (np.asarray(x) for x in (control_verb, det_seqs_v, det_seqs_sr, idx_list))
    idx_list = idx_list.reshape(control_verb.shape[0], -1)
    gather, tr_locs, gt_locs, keys = [], [], [], []
    for n in range(control_verb.shape[0]):
        for v, verb in enumerate(control_verb[n]):
            if verb == 0:
                break
            find_sr, sr_find, need_re_rank = 0, {}, set()
            for j in range(det_seqs_v.shape[1]):
                for k in range(det_seqs_v.shape[2]):
                    if verb == det_seqs_v[n, j, k] and find_sr < 10:
                        sr = int(det_seqs_sr[n, j, k])
                        if sr not in sr_find:
                            sr_find[sr] = [j]
                            find_sr += 1
                        else:
                            sr_find[sr].append(j)
                            need_re_rank.add(sr)
            if find_sr == 0:
                continue
            for sr in sorted(need_re_rank):
                locs = sr_find[sr][:n_sink]
                tr = np.full(n_sink, PAD_LOC, dtype=np.float32)
                g = np.full(n_sink, PAD_LOC, dtype=np.float32)
                gt = np.full(n_sink, PAD_LOC, dtype=np.float32)
                for j, loc in enumerate(locs):
                    tr[j] = loc
                    g[j] = idx_list[n, loc]
                change = np.argsort(g, kind="stable")
                gt[:len(locs)] = change[:len(locs)]
                gather.append([n * L + loc for loc in locs] + [-1] * (n_sink - len(locs)))
                tr_locs.append(tr)
                gt_locs.append(gt)
                keys.append((n, v, sr))
    return (np.array(gather, dtype=np.int64).reshape(-1, n_sink), np.array(tr_locs, dtype=np.float32).reshape(-1, n_sink),
            np.array(gt_locs, dtype=np.float32).reshape(-1, n_sink), np.array(keys, dtype=np.int64).reshape(-1, 3))


# ---------------------------------------------------------------------------------------------- device builder
class TrainBatch:
    """What build_device returns, all on the GPU and sliced to the counts: verbs (S, 1) int64, det_roles / gt_roles (S, 10) int32 (gt_roles
    None without gt annotations); seq (Q, n_sink, D) fp32 (None without seqs_perm), item_gather (Q, n_sink) int32, tr_locs / gt_locs
    (Q, n_sink) fp32, item_key (Q, 3) int32 = (caption, verb column, role) (all None without idx_list); status (N,) int32 (a bit set: BAD_ROLE, BAD_VERB,
    TRUNCATED, BAD_IDX).  On the host: n_seqs = S, n_items = Q, status_or (the OR of all status words), n_dropped (items beyond max_items)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


_engines = {}


def _engine(device):
    from .ssp import SspEngine
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("build_device runs only on the GPU (got %s); the host yardsticks are ssp_train_batch / sinkhorn_train_items" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _engines:
        _engines[device] = SspEngine(device)
    return _engines[device]


def build_device(device, control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v=None, gt_seqs_sr=None, idx_list=None, seqs_perm=None, n_sink=10,
                 n_verbs=N_VERBS_COCO, max_items=None):
    """The two scripts' batch-building loops as one call: the annotations of N caption rows (host arrays: one non-blocking upload; or GPU
    tensors) -> a TrainBatch.  gt_seqs_v / gt_seqs_sr give gt_roles (S-SSP), idx_list (N, L) gives the Sinkhorn items, seqs_perm (N, L, D)
    fp32 on the GPU (D = 2352 for SinkhornNet) gives their feature rows.  n_verbs: rows of the verb table (S_SSP(dataset=...)
    .v_embed_layer.weight.shape[0]).

    The plan is two launches; then counts - 16 bytes - is read back.  That read is THE STEP'S SINGLE HOST SYNCHRONISATION: the S-SSP forward
    takes exactly S sequences, so S has to reach the host before it is launched.  Everything else (slicing, the row gather for the Q items
    that exist) is launches and views."""
    eng = _engine(device)
    t = eng.train_batch_plan(control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v, gt_seqs_sr, idx_list, n_sink=n_sink, n_verbs=n_verbs, max_items=max_items)
    n_seqs, n_items, status_or, n_dropped = t["counts"].tolist()                     # the one read-back
    return _finish(eng, t, seqs_perm, n_seqs, n_items, status_or, n_dropped)


def _finish(eng, t, seqs_perm, n_seqs, n_items, status_or, n_dropped):
    cut = lambda x, n: None if x is None else x[:n]
    seq = None
    if seqs_perm is not None and t["item_gather"] is not None:
        if seqs_perm.dim() != 3 or seqs_perm.size(0) != t["status"].numel() or seqs_perm.size(1) != L:
            raise RuntimeError("expected seqs_perm (%d, %d, D); got %s" % (t["status"].numel(), L, tuple(seqs_perm.shape)))
        rows = seqs_perm.reshape(seqs_perm.size(0) * L, seqs_perm.size(2))
        seq = eng.gather_rows(rows, t["item_gather"][:n_items])
    return TrainBatch(verbs=t["verbs"][:n_seqs].unsqueeze(1), det_roles=t["det_roles"][:n_seqs], gt_roles=cut(t["gt_roles"], n_seqs), seq=seq,
                      item_gather=cut(t["item_gather"], n_items), tr_locs=cut(t["tr_locs"], n_items), gt_locs=cut(t["gt_locs"], n_items),
                      item_key=cut(t["item_key"], n_items), status=t["status"], n_seqs=n_seqs, n_items=n_items, status_or=status_or, n_dropped=n_dropped)


# ---------------------------------------------------------------------------------------------- loss helpers
def ssp_loss(ssp, batch):
    """train_region_sort.py:181 on a TrainBatch: ssp(batch.verbs, batch.det_roles, batch.gt_roles), or None when the batch has no active
    job (nothing is launched)"""
    if batch.n_seqs == 0:
        return None
    if batch.gt_roles is None:
        raise RuntimeError("ssp_loss: the batch was built without gt_seqs_v / gt_seqs_sr")
    return ssp(batch.verbs, batch.det_roles, batch.gt_roles)


def sinkhorn_loss(sinkhorn, batch, batch_size):
    """train_sinkhorn.py:207-211 on a TrainBatch: the sum of the items' location losses / batch_size (the script's detections.size(0)), or
    None when the batch has no item - the reference then skips the step (`if loss != 0.`)"""
    if batch.n_items == 0:
        return None
    if batch.seq is None:
        raise RuntimeError("sinkhorn_loss: the batch was built without idx_list / seqs_perm")
    return sinkhorn.loc_loss(batch.seq, batch.tr_locs, batch.gt_locs, scale=1.0 / batch_size)
