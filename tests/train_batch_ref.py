"""Cases for the training-batch builder, shared by tests/test_train_batch_logic.py (the host tool over
csrc/train_batch_logic.h) and tests/test_gpu_train_batch.py (the kernels): the named corners, a seeded random generator, and the driver
of tools/train_batch_host.  What either must reproduce is host_tables below - the numpy yardsticks of vsrcap.trainbatch with the padding,
the counts and the status of vsr_train_batch_plan around them."""
import subprocess

import numpy as np

from conftest import load_golden
from vsrcap import trainbatch as tb

L = tb.L
N_VERBS = 2663
TABLES = ("verbs", "det_roles", "gt_roles", "item_gather", "tr_locs", "gt_locs", "item_key", "counts", "status")


def caption_status(control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v=None, gt_seqs_sr=None, idx_list=None, n_sink=10, n_verbs=N_VERBS):
    """status (N,) int64 as vsr_train_batch_plan reports it, from the yardsticks' own tables: bit 4 a det / gt role id outside [0, 26),
    8 a verb whose C remainder % 10000 lies outside [0, n_verbs) (any negative id that is no multiple of 10000 included), 32 an item cut to n_sink slots, 64 an idx_list value outside [0, 10) at a used
    slot - each judged on the caption's active jobs"""
    control_verb, det_seqs_v, det_seqs_sr = (np.asarray(x) for x in (control_verb, det_seqs_v, det_seqs_sr))
    N = control_verb.shape[0]
    status = np.zeros(N, dtype=np.int64)
    if idx_list is not None:
        idx_list = np.asarray(idx_list).reshape(N, -1)
    for n in range(N):
        one = [x[n:n + 1] for x in (control_verb, det_seqs_v, det_seqs_sr)]
        gt = [np.asarray(x)[n:n + 1] for x in (gt_seqs_v, gt_seqs_sr)] if gt_seqs_v is not None else [np.zeros((1, 1, one[1].shape[2]), np.int64), np.zeros((1, 1, one[2].shape[2]), np.int64)]
        verbs, det, g = tb.ssp_train_batch(*one, *gt)
        if ((det < 0) | (det >= 26) | (g < 0) | (g >= 26)).any():
            status[n] |= tb.BAD_ROLE
        if ((np.fmod(verbs, 10000) < 0) | (np.fmod(verbs, 10000) >= n_verbs)).any():          # the C remainder, as the kernels take it
            status[n] |= tb.BAD_VERB
        if idx_list is not None:
            full = tb.sinkhorn_train_items(*one, idx_list[n:n + 1], n_sink=L * one[1].shape[2])[0]
            gather = full[:, :n_sink]
            if (full[:, n_sink:] >= 0).any():
                status[n] |= tb.TRUNCATED
            used = idx_list[n][gather[gather >= 0]]
            if ((used < 0) | (used >= 10)).any():
                status[n] |= tb.BAD_IDX
    return status


def host_tables(control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v=None, gt_seqs_sr=None, idx_list=None, n_sink=10, n_verbs=N_VERBS, max_items=0):
    """Everything vsr_train_batch_plan writes, from the yardsticks: a dict of numpy arrays at the padded sizes - verbs (N MV,), det_roles,
    gt_roles (N MV, 10), item_gather / tr_locs / gt_locs (Q, n_sink), item_key (Q, 3), counts (4,), status (N,), with Q = max_items or
    N MV 10.  The rows and items of a caption with status bit 4 or 8 are left out; rows and items beyond the counts are zeros (-1 in
    item_gather)."""
    control_verb = np.asarray(control_verb)
    N, MV = control_verb.shape
    S, Q = N * MV, max_items if max_items > 0 else N * MV * L
    status = caption_status(control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v, gt_seqs_sr, idx_list, n_sink, n_verbs)
    keep = [n for n in range(N) if not status[n] & tb.DROP_CAPTION]
    sub = lambda x: np.asarray(x)[keep]
    out = dict(verbs=np.zeros(S, np.int64), det_roles=np.zeros((S, L), np.int64), gt_roles=np.zeros((S, L), np.int64), item_gather=np.full((Q, n_sink), -1, np.int64),
               tr_locs=np.zeros((Q, n_sink), np.float32), gt_locs=np.zeros((Q, n_sink), np.float32), item_key=np.zeros((Q, 3), np.int64), status=status)
    n_rows = n_found = 0
    if keep:
        gt = [sub(gt_seqs_v), sub(gt_seqs_sr)] if gt_seqs_v is not None else [np.zeros((len(keep), 1, MV), np.int64), np.zeros((len(keep), 1, np.asarray(det_seqs_sr).shape[2]), np.int64)]
        verbs, det, g = tb.ssp_train_batch(sub(control_verb), sub(det_seqs_v), sub(det_seqs_sr), *gt)
        n_rows = len(verbs)
        out["verbs"][:n_rows], out["det_roles"][:n_rows], out["gt_roles"][:n_rows] = verbs, det, g
        if idx_list is not None:
            gather, tr, gl, keys = tb.sinkhorn_train_items(sub(control_verb), sub(det_seqs_v), sub(det_seqs_sr), sub(np.asarray(idx_list).reshape(N, -1)), n_sink)
            n_found = len(keys)
            q = min(n_found, Q)
            if q:
                orig = np.array(keep, dtype=np.int64)[keys[:, 0]]                        # caption ids of the whole batch again
                out["item_gather"][:q] = np.where(gather >= 0, gather + (orig - keys[:, 0])[:, None] * L, -1)[:q]
                out["tr_locs"][:q], out["gt_locs"][:q] = tr[:q], gl[:q]
                out["item_key"][:q] = np.stack([orig, keys[:, 1], keys[:, 2]], 1)[:q]
    out["counts"] = np.array([n_rows, min(n_found, Q), int(np.bitwise_or.reduce(status)) if N else 0, n_found - min(n_found, Q)], dtype=np.int64)
    return out


class Case:
    def __init__(self, control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v=None, gt_seqs_sr=None, idx_list=None, n_sink=10, max_items=0, name=""):
        i64 = lambda x: None if x is None else np.asarray(x, dtype=np.int64)
        self.control_verb, self.det_seqs_v, self.det_seqs_sr, self.gt_seqs_v, self.gt_seqs_sr, self.idx_list = map(i64, (control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v,
                                                                                                                         gt_seqs_sr, idx_list))
        self.N, self.MV = self.control_verb.shape
        self.MS = self.det_seqs_sr.shape[2]
        self.Lg = self.gt_seqs_v.shape[1] if self.gt_seqs_v is not None else 0
        self.n_sink, self.max_items, self.name = n_sink, max_items, name

    @property
    def qcap(self):
        return self.max_items if self.max_items > 0 else self.N * self.MV * L

    def annotations(self):
        return dict(control_verb=self.control_verb, det_seqs_v=self.det_seqs_v, det_seqs_sr=self.det_seqs_sr, gt_seqs_v=self.gt_seqs_v, gt_seqs_sr=self.gt_seqs_sr,
                    idx_list=self.idx_list)

    def expected(self):
        return host_tables(n_sink=self.n_sink, n_verbs=N_VERBS, max_items=self.max_items, **self.annotations())


def fixture_case():
    meta, g = load_golden("g18_train_batch")
    return meta, g, Case(g["control_verb"], g["det_seqs_v"], g["det_seqs_sr"], g["gt_seqs_v"], g["gt_seqs_sr"], g["idx_list"], n_sink=meta["n_sink"], name="g18")


def fixture_items(meta, g):
    """the reference's recorded items as {(n, verb column, role): (gather row, tr_locs, gt_locs)}: the key's verb names its column (verbs are
    distinct per caption), the rows of this_sr_perm name their slots (every feature row is distinct and non-zero)"""
    flat = g["seqs_perm"].reshape(-1, meta["D"])
    row_of = {r.tobytes(): i for i, r in enumerate(flat)}
    assert len(row_of) == len(flat)
    zero = np.zeros(meta["D"], np.float32).tobytes()
    out = {}
    for key, perm, t, gl in zip(g["ref_keys"], g["ref_sr_perm"], g["ref_tr_locs"], g["ref_gt_locs"]):
        n = int(key[0]) * meta["n_caps"] + int(key[1])
        v = g["control_verb"][n].tolist().index(int(key[2]))
        out[(n, v, int(key[3]))] = (np.array([-1 if r.tobytes() == zero else row_of[r.tobytes()] for r in perm]), t, gl)
    assert len(out) == len(g["ref_keys"]) == meta["n_items"]
    return out


def _blank(N, MV, MS=None, Lg=L):
    MS = MS or MV
    return (np.zeros((N, MV), np.int64), np.zeros((N, L, MV), np.int64), np.zeros((N, L, MS), np.int64), np.zeros((N, Lg, MV), np.int64), np.zeros((N, Lg, MS), np.int64),
            np.tile(np.arange(L), (N, 1)))


def _three_captions():
    """three captions of one verb each: roles [1, 2, 1, 3] in slots 0..3 (one item per caption), gt = det"""
    cv, dv, dsr, gv, gsr, idx = _blank(3, 2)
    cv[:, 0] = [61, 62, 63]
    for n in range(3):
        dv[n, :4, 0], dsr[n, :4, 0] = cv[n, 0], [1, 2, 1, 3]
        idx[n] = np.roll(np.arange(L), n + 1)
    gv[:], gsr[:] = dv, dsr
    return cv, dv, dsr, gv, gsr, idx


def special_cases():
    """the named corners; tests/test_train_batch_logic.py asserts on the yardsticks' tables that each is what it says"""
    out = []
    cv, dv, dsr, gv, gsr, idx = _blank(1, 1)                     # a role repeated more often than N_sink: bit 32
    cv[0, 0] = 31
    dv[0, :7, 0], dsr[0, :7, 0] = 31, [2, 2, 5, 2, 2, 2, 2]
    idx[0] = [4, 2, 9, 0, 1, 3, 5, 6, 7, 8]
    out.append(Case(cv, dv, dsr, gv, gsr, idx, n_sink=3, name="truncation"))
    cv, dv, dsr, gv, gsr, idx = _three_captions()                # role id 26 in the middle caption's det: bit 4, the caption emits nothing
    dsr[1, 1, 0] = 26
    out.append(Case(cv, dv, dsr, gv, gsr, idx, name="role_26_det"))
    cv, dv, dsr, gv, gsr, idx = _three_captions()                # ... in its gt only
    gsr[1, 3, 0] = 26
    out.append(Case(cv, dv, dsr, gv, gsr, idx, name="role_26_gt"))
    cv, dv, dsr, gv, gsr, idx = _three_captions()                # a negative verb: bit 8
    cv[2, 0] = -7
    dv[2][dv[2] == 63], gv[2][gv[2] == 63] = -7, -7
    out.append(Case(cv, dv, dsr, gv, gsr, idx, name="negative_verb"))
    cv, dv, dsr, gv, gsr, idx = _blank(1, 1)                     # idx_list value 10 at a used slot: bit 64; it ties with the padding in front of it only
    cv[0, 0] = 33                                                # under the stable rule: g = [10, 3, 10, 10] -> change = [1, 0, 2, 3]
    dv[0, :2, 0], dsr[0, :2, 0] = 33, [4, 4]
    idx[0, :2] = [10, 3]
    out.append(Case(cv, dv, dsr, gv, gsr, idx, n_sink=4, name="idx_10_stable_tie"))
    cv, dv, dsr, gv, gsr, idx = _three_captions()                # max_items one below the item count (3)
    out.append(Case(cv, dv, dsr, gv, gsr, idx, max_items=2, name="max_items_minus_one"))
    cv, dv, dsr, gv, gsr, idx = _three_captions()                # no job is active: a 0 first, no verb, a verb without a match
    cv[0] = [0, 61]
    cv[1] = 0
    dv[2] = 0
    out.append(Case(cv, dv, dsr, gv, gsr, idx, name="all_inactive"))
    cv, dv, dsr, gv, gsr, idx = _three_captions()                # no gt annotations / no idx_list: the optional halves
    out.append(Case(cv, dv, dsr, None, None, idx, name="no_gt"))
    out.append(Case(cv, dv, dsr, gv, gsr, None, name="no_idx"))
    cv, dv, dsr, gv, gsr, idx = _blank(1, 2, Lg=1)               # Lg = 1; both columns of every slot carry the verb: the gate closes at slot 4
    cv[0] = [21, 22]
    dv[0, :, :] = 21
    for j in range(L):
        dsr[0, j] = [2 * j + 1, 2 * j + 2] if j < 6 else [3, 5]
    gv[0, 0], gsr[0, 0] = [21, 22], [9, 1]
    out.append(Case(cv, dv, dsr, gv, gsr, idx, name="gate_and_lg1"))
    return out


def random_case(rng, N=None, MV=None, n_sink=None):
    N = N or int(rng.randint(1, 7))
    MV = MV or int(rng.choice([1, 3, 8]))
    MS = MV + int(rng.randint(0, 2))
    n_sink = n_sink or int(rng.choice([2, 10, 16]))
    Lg = int(rng.choice([1, 10, 13]))
    cv, dv, dsr, gv, gsr, idx = _blank(N, MV, MS, Lg)
    for n in range(N):
        pool = rng.choice(np.arange(1, 60), MV, replace=False) + 10000 * rng.randint(0, 3)
        nv = int(rng.randint(0, MV + 1))
        cv[n, :nv] = pool[:nv]
        if nv >= 2 and rng.rand() < 0.15:
            cv[n, rng.randint(0, nv)] = 0                        # a hole: the verbs after it are no jobs
        if nv and rng.rand() < 0.03:
            cv[n, 0] = -cv[n, 0]                                 # (rarely) a negative verb ...
            pool[0] = cv[n, 0]
        n_roles = int(rng.choice([2, 4, 7, 14, 25 if rng.rand() < 0.9 else 27]))       # ... or role ids beyond the table
        one_verb = nv > 0 and rng.rand() < 0.2                    # every column carries the first verb: many matches, the gate closes
        for seq_v, seq_sr, rows in ((dv, dsr, L), (gv, gsr, Lg)):
            for j in range(int(rng.randint(0, rows + 1))):
                for k in range(MV):
                    if rng.rand() < 0.6:
                        seq_v[n, j, k] = pool[0 if one_verb else rng.randint(0, MV)]
                        seq_sr[n, j, k] = rng.randint(0 if rng.rand() < 0.1 else 1, n_roles + 1)
        idx[n] = rng.permutation(L)
        if rng.rand() < 0.05:
            idx[n, rng.randint(0, L)] = rng.choice([-1, 10, 11])  # (rarely) a position outside [0, 10)
    pick = rng.rand()
    case = Case(cv, dv, dsr, None if pick < 0.1 else gv, None if pick < 0.1 else gsr, None if 0.1 <= pick < 0.2 else idx, n_sink=n_sink, name="random")
    if case.idx_list is not None:
        n_items = int(case.expected()["counts"][1])
        pick = rng.rand()
        if n_items and pick < 0.15:
            case.max_items = n_items
        elif n_items > 1 and pick < 0.3:
            case.max_items = n_items - 1
    return case


def run_tool(tool, cases):
    """tools/train_batch_host on `cases` -> one dict of tables per case (TABLES)"""
    lines = [str(len(cases))]
    for c in cases:
        lines.append("%d %d %d %d %d %d %d %d %d %d" % (c.N, L, max(c.Lg, 1), c.MV, c.MS, c.n_sink, N_VERBS, c.max_items, c.gt_seqs_v is not None, c.idx_list is not None))
        for a in c.annotations().values():
            if a is not None:
                lines.append(" ".join(map(str, a.reshape(-1).tolist())))
    res = subprocess.run([tool], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert len(out) == len(cases)
    got = []
    for c, line in zip(cases, out):
        v = np.array(line.split(), dtype=np.float64)
        S, Q, K = c.N * c.MV, c.qcap, c.n_sink
        cuts = np.cumsum([S, S * L, S * L, Q * K, Q * K, Q * K, Q * 3, 4, c.N])
        assert len(v) == cuts[-1]
        parts = np.split(v, cuts[:-1])
        shapes = [(S,), (S, L), (S, L), (Q, K), (Q, K), (Q, K), (Q, 3), (4,), (c.N,)]
        got.append({k: (p.astype(np.float32) if k in ("tr_locs", "gt_locs") else p.astype(np.int64)).reshape(sh) for k, p, sh in zip(TABLES, parts, shapes)})
    return got


def check(case, exp, got):
    """every table equal, dtype-blind for the integers (array_equal on the values), fp32 against fp32 for the two float tables"""
    for k in TABLES:
        g = got[k]
        if g is None:                                            # a table the device path does not return without its annotation
            assert (k == "gt_roles" and case.gt_seqs_v is None) or (k in ("item_gather", "tr_locs", "gt_locs", "item_key") and case.idx_list is None), k
            continue
        g = np.asarray(g)
        if k in ("tr_locs", "gt_locs"):
            assert g.dtype == np.float32 and exp[k].dtype == np.float32
        assert g.shape == exp[k].shape, "%s: %s shape %s != %s" % (case.name, k, g.shape, exp[k].shape)
        np.testing.assert_array_equal(g, exp[k], err_msg="%s: %s" % (case.name, k))
