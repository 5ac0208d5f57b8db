"""The host side of the caption ranking as a reference for csrc/rank_logic.h (tests/test_rank_logic.py on the CPU,
tests/test_gpu_rank_device.py on the GPU): the bookkeeping loop of vsrcap.evalbatch.rank_captions lifted verbatim, with the two
networks' decisions INJECTED (pred per job, assign per Sinkhorn item) instead of computed, plus evalbatch.verb_rank_merge itself.
Also the case generator both tests share.

The copies mirror vsr-guided-cic_amd/vsrcap/evalbatch.py as follows (a change there must be repeated here): host_jobs = rank_captions'
job loop (:95-114, with the verb column recorded), host_items = its item loop (:120-126), host_finish = :134-155 with pred / assign
given.  Verb ids are non-negative (a negative id is invalid on the device path: status bit 8)."""
import numpy as np

from vsrcap.evalbatch import verb_rank_merge

L = 10
N_VERBS = 2663
NO_JOB, ITEM_OVERFLOW, BAD_ROLE, BAD_VERB = 1, 2, 4, 8


class Case:
    def __init__(self, control_verb, det_seqs_v, det_seqs_sr, n_sink=10, max_items=0, pred_order=None, name=""):
        self.control_verb, self.det_seqs_v, self.det_seqs_sr = (np.asarray(x, dtype=np.int64) for x in (control_verb, det_seqs_v, det_seqs_sr))
        self.N, self.MV = self.control_verb.shape
        self.MS = self.det_seqs_sr.shape[2]
        assert self.det_seqs_v.shape == (self.N, L, self.MV) and self.det_seqs_sr.shape[:2] == (self.N, L) and self.MS >= self.MV
        self.n_sink, self.max_items, self.name = n_sink, max_items, name
        self.pred_order = pred_order or {}            # {(n, v): role order} where a case needs one particular decision

    @property
    def S(self):
        return self.N * self.MV

    @property
    def qcap(self):
        return self.max_items if self.max_items > 0 else self.S * L


def host_jobs(case):
    """evalbatch.rank_captions' first loop: [(caption, verb column, verb, roles (L,), sr_find, need)] of the active jobs"""
    control_verb, det_seqs_v, det_seqs_sr = case.control_verb, case.det_seqs_v, case.det_seqs_sr
    jobs = []
    for n in range(case.N):
        for v, verb in enumerate(control_verb[n]):
            if verb == 0:
                break
            roles = np.zeros(L, dtype=np.int64)
            find_sr, sr_find, need = 0, {}, set()
            for j in range(L):
                for k in range(det_seqs_v.shape[2]):
                    if verb == det_seqs_v[n, j, k] and find_sr < 10:
                        sr = int(det_seqs_sr[n, j, k])
                        if sr not in sr_find:
                            sr_find[sr] = [j]
                            roles[find_sr] = sr
                            find_sr += 1
                        else:
                            sr_find[sr].append(j)
                            need.add(sr)
            if find_sr:
                jobs.append((n, v, int(verb), roles, sr_find, need))
    return jobs


def host_items(case, jobs):
    """its second loop: [(job index, role, locs)] and the gather rows"""
    items, gather = [], []
    SN = case.n_sink
    for ji, (n, _, _, _, sr_find, need) in enumerate(jobs):
        for sr in sorted(need):
            locs = sr_find[sr][:SN]
            items.append((ji, sr, locs))
            gather.append([n * L + loc for loc in locs] + [-1] * (SN - len(locs)))
    return items, gather


def host_finish(case, jobs, items, pred, assign, stats=None):
    """the rest of it with pred[ji] (10 role ids, 0 ends) and assign[item] (a permutation of range(N_sink)) given: N rank lists"""
    sr_rank = {}
    for (ji, sr, locs), a in zip(items, assign):
        order = np.argsort(np.array([a[i] for i in range(len(locs))]))
        sr_rank[(ji, sr)] = [locs[i] for i in order]
    ranks = [[] for _ in range(case.N)]
    for ji, (n, _, _, _, sr_find, _) in enumerate(jobs):
        verb_rank = []
        for sr in pred[ji]:
            if sr == 0:
                break
            verb_rank += sr_rank[(ji, int(sr))] if len(sr_find[int(sr)]) != 1 else sr_find[int(sr)]
        ranks[n].append(verb_rank)
    out = []
    for n in range(case.N):
        if not ranks[n]:
            out.append([])
            continue
        final = ranks[n][0]
        for other in ranks[n][1:]:
            if stats is not None:
                pos = [other.index(a) for a in final if a in other]
                stats["out_of_order"] += pos != sorted(pos)
            final = verb_rank_merge(final, other)
        if stats is not None:
            stats["long"] += len(final) > L
            stats["duplicate"] += len(set(final)) != len(final)
        out.append([int(x) for x in final])
    return out


def decide(case, jobs, items, rng):
    """random valid decisions: per job a permutation of its (non-zero) roles, per item a permutation of range(N_sink)"""
    pred = []
    for (n, v, _, roles, _, _) in jobs:
        r = [int(x) for x in roles if x != 0]
        order = case.pred_order.get((n, v)) or [r[i] for i in rng.permutation(len(r))]
        pred.append(list(order) + [0] * (L - len(order)))
    assign = [[int(x) for x in rng.permutation(case.n_sink)] for _ in items]
    return pred, assign


def expected(case, rng, stats=None):
    """everything the device path / the host tool must reproduce for `case` under decisions drawn from rng:
    dict(job_verbs (S), job_roles (S,10), n_items, gather (Qcap, N_sink), pred (S,10) and assign (Qcap, N_sink) padded, rank (N,L), status (N))"""
    jobs = host_jobs(case)
    items, gather = host_items(case, jobs)
    pred, assign = decide(case, jobs, items, rng)
    S, Q, SN = case.S, case.qcap, case.n_sink
    e = dict(job_verbs=np.zeros(S, np.int64), job_roles=np.zeros((S, L), np.int64), n_items=len(items), gather=np.full((Q, SN), -1, np.int64),
             pred=np.zeros((S, L), np.int64), assign=np.tile(np.arange(SN), (Q, 1)).astype(np.int64), status=np.zeros(case.N, np.int64),
             rank=np.full((case.N, L), -1, np.int64))
    has_job = np.zeros(case.N, bool)
    for ji, (n, v, verb, roles, sr_find, _) in enumerate(jobs):
        s = n * case.MV + v
        e["job_verbs"][s], e["job_roles"][s], e["pred"][s] = verb, roles, pred[ji]
        has_job[n] = True
        if any(sr < 0 or sr >= 26 for sr in sr_find):
            e["status"][n] |= BAD_ROLE
        if not 0 <= verb % 10000 < N_VERBS:
            e["status"][n] |= BAD_VERB
    e["status"][~has_job] |= NO_JOB
    for q, ((ji, _, _), g, a) in enumerate(zip(items, gather, assign)):
        if q < Q:
            e["gather"][q], e["assign"][q] = g, a
        else:
            e["status"][jobs[ji][0]] |= ITEM_OVERFLOW
    final = host_finish(case, jobs, items, pred, assign, stats)
    for n in range(case.N):
        if e["status"][n] == 0:
            fr = final[n][:L]
            e["rank"][n, :len(fr)] = fr
    return e


def _blank(N, MV, MS=None):
    return np.zeros((N, MV), np.int64), np.zeros((N, L, MV), np.int64), np.zeros((N, L, MS or MV), np.int64)


def special_cases():
    """the cases the issue names; each asserts (through `stats` or its own shape) that it is what it says"""
    out = []
    cv, dv, dsr = _blank(1, 1)                                   # N = 1, MV = 1
    cv[0, 0] = 7
    for j, sr in enumerate([3, 1, 3, 2]):
        dv[0, j, 0], dsr[0, j, 0] = 7, sr
    out.append(Case(cv, dv, dsr, name="n1_mv1"))
    cv, dv, dsr = _blank(3, 2)                                   # the middle caption's verb matches nothing
    cv[:, 0] = [5, 6, 7]
    for n in (0, 2):
        for j in range(3):
            dv[n, j, 0], dsr[n, j, 0] = cv[n, 0], j + 1
    dv[1, 0, 0], dsr[1, 0, 0] = 99, 4
    out.append(Case(cv, dv, dsr, name="no_match"))
    cv, dv, dsr = _blank(1, 3)                                   # control_verb = [v, 0, w]: w is never a job
    cv[0] = [11, 0, 12]
    for j in range(4):
        dv[0, j, 0], dsr[0, j, 0] = 11, 1 + j % 2
        dv[0, j, 2], dsr[0, j, 2] = 12, 5
    out.append(Case(cv, dv, dsr, name="v_0_w"))
    cv, dv, dsr = _blank(1, 2)                                   # one verb in both columns of a slot: duplicate slots, > 10 distinct roles
    cv[0] = [21, 22]
    dv[0, :, :] = 21
    dsr[0, 0] = [3, 3]
    for j in range(1, L):
        dsr[0, j] = [2 * j + 2, 2 * j + 3] if j < 6 else [4, 6]
    dv[0, 9, 1], dsr[0, 9, 1] = 22, 1
    out.append(Case(cv, dv, dsr, name="two_columns_gate"))
    cv, dv, dsr = _blank(1, 1)                                   # a role repeated more than N_sink times
    cv[0, 0] = 31
    dv[0, :7, 0] = 31
    dsr[0, :7, 0] = [2, 2, 5, 2, 2, 2, 2]
    out.append(Case(cv, dv, dsr, n_sink=3, name="more_than_n_sink"))
    cv, dv, dsr = _blank(1, 2)                                   # a merged list longer than L (both columns of six slots)
    cv[0] = [41, 42]
    dv[0, :6, :] = 41
    dsr[0, :6, 0], dsr[0, :6, 1] = 1, 2
    dv[0, 6:, 0], dsr[0, 6:, 0] = 42, [3, 4, 5, 6]
    out.append(Case(cv, dv, dsr, name="longer_than_L"))
    cv, dv, dsr = _blank(1, 2)                                   # lb's shared entries out of order: la = [0,1,2], lb = [2,5,1]
    cv[0] = [51, 52]
    for j in range(3):
        dv[0, j, 0], dsr[0, j, 0] = 51, j + 1
    for j, sr in ((2, 7), (5, 8), (1, 9)):
        dv[0, j, 1], dsr[0, j, 1] = 52, sr
    out.append(Case(cv, dv, dsr, pred_order={(0, 0): [1, 2, 3], (0, 1): [7, 8, 9]}, name="out_of_order"))
    cv, dv, dsr = _blank(3, 2)                                   # max_items one below the item count (4): the last caption's item is dropped
    cv[:, 0] = [61, 62, 63]
    cv[1, 1] = 64
    for n in range(3):
        dv[n, :4, 0], dsr[n, :4, 0] = cv[n, 0], [1, 2, 1, 3]
    dv[1, 4:7, 1], dsr[1, 4:7, 1] = 64, [5, 5, 5]
    out.append(Case(cv, dv, dsr, max_items=3, name="max_items_minus_one"))
    return out


def random_case(rng, N=None, MV=None, n_sink=None):
    N = N or int(rng.randint(1, 4))
    MV = MV or int(rng.choice([1, 2, 2, 3, 3, 4, 8]))
    MS = MV + int(rng.randint(0, 2))
    n_sink = n_sink or int(rng.choice([2, 3, 5, 10, 10, 16]))
    cv, dv, dsr = _blank(N, MV, MS)
    for n in range(N):
        pool = rng.choice(np.arange(1, 60), MV, replace=False) + 10000 * rng.randint(0, 3)
        nv = int(rng.randint(0, MV + 1))
        cv[n, :nv] = pool[:nv]
        if nv >= 2 and rng.rand() < 0.15:
            cv[n, rng.randint(0, nv)] = 0                        # a hole: the verbs after it are no jobs
        n_roles = int(rng.choice([2, 4, 7, 14, 25]))
        one_verb = nv > 0 and rng.rand() < 0.2                    # every column carries the first verb: many matches, the gate closes
        for j in range(int(rng.randint(0, L + 1))):
            for k in range(MV):
                if rng.rand() < 0.6:
                    dv[n, j, k] = pool[0 if one_verb else rng.randint(0, MV)]       # any column may carry any verb, the same one twice too
                    dsr[n, j, k] = rng.randint(0 if rng.rand() < 0.1 else 1, n_roles + 1)
    case = Case(cv, dv, dsr, n_sink=n_sink, name="random")
    n_items = len(host_items(case, host_jobs(case))[0])
    pick = rng.rand()
    if n_items and pick < 0.15:
        case.max_items = n_items
    elif n_items > 1 and pick < 0.3:
        case.max_items = n_items - 1
    return case
