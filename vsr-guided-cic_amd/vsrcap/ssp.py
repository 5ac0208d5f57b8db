"""Host driver of the ordering-model entry points of libvsrcap.so (include/vsrcap.h: vsr_ssp_*, vsr_sinkhorn_*): one
vsr_ssp object per device, weights borrowed from torch parameters, work enqueued on torch's current stream.  No fallback:
CPU tensors raise.

SinkhornNet trains through SinkhornTrainFn (one forward / one hand-written backward for all Q items of a loader batch) and
sinkhorn_loc_loss (the fused location loss of coco_scripts/train_sinkhorn.py:207-209).  S_SSP trains through SspTrainFn: the loss of
models/sort_model.py:80-103 for all S sequences of a loader batch in one forward, one hand-written backward; dropout masks are a byte
buffer (ssp_mask_layout, ssp_dropout_masks) that the forward and the backward both read.

rank_captions is the eval loop's ranking (eval_coco.py:141-221) for a loader batch as one stream of launches (vsr_rank_captions): integer
annotations in, the (N, L) rank tensor and a per-caption status out, both on the device, nothing read back; rank_plan / rank_finish are
its two integer stages on their own.  train_batch_plan / gather_rows are the training twin (vsr_train_batch_plan, vsr_gather_rows): the
same annotations in, the inputs of the two training calls out; vsrcap/trainbatch.py builds a batch from them."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s); this path has no CPU implementation" % (name, t.device))


SSP_DROPOUT_P = 0.1          # every nn.Dropout of the reference's S_SSP (sort_modules.py, transformer_modules.py: dropout_ratio=0.1)


def _ssp_layout():
    """[(field path in vsr_ssp_weights / vsr_ssp_grads, state_dict key)] of every weight the model uses, in struct order
    (decoder.*.cross_attention.* is never called, sort_modules.py:87: it is not bound and has no gradient)"""
    def layer(stack, l, pre, dec):
        out = [((stack, l, "ln%d_%s" % (i, f)), "%s.layer_norm%d.%s" % (pre, i, wb)) for i in (1, 2, 3) if i < 3 or dec
               for wb, f in (("weight", "w"), ("bias", "b"))]
        for q in "QKVO":
            out += [((stack, l, "W" + q.lower()), "%s.attention.linear_%s.weight" % (pre, q)), ((stack, l, "b" + q.lower()), "%s.attention.linear_%s.bias" % (pre, q))]
        return out + [((stack, l, "W1"), pre + ".ff_layer.w_1.weight"), ((stack, l, "b1"), pre + ".ff_layer.w_1.bias"),
                      ((stack, l, "W2"), pre + ".ff_layer.w_2.weight"), ((stack, l, "b2"), pre + ".ff_layer.w_2.bias")]
    out = [(("sr_embed",), "sr_embed_layer.weight"), (("v_embed",), "v_embed_layer.weight"),
           (("fc_w",), "encoder.fc_feat.weight"), (("fc_b",), "encoder.fc_feat.bias")]
    for l in range(3):
        out += layer("enc", l, "encoder.encoder_layers.%d" % l, False)
    out += [(("enc_ln_w",), "encoder.layer_norm.weight"), (("enc_ln_b",), "encoder.layer_norm.bias")]
    for l in range(3):
        out += layer("dec", l, "decoder.encoder_layers.%d" % l, True)
    return out + [(("dec_ln_w",), "decoder.layer_norm.weight"), (("dec_ln_b",), "decoder.layer_norm.bias"),
                  (("exp_w",), "expander_nn.weight"), (("exp_b",), "expander_nn.bias")]


SSP_LAYOUT = _ssp_layout()
SSP_PARAM_KEYS = [k for _, k in SSP_LAYOUT]


def _set_field(struct, path, value):
    for name in path[:-1]:
        struct = struct[name] if isinstance(name, int) else getattr(struct, name)
    setattr(struct, path[-1], value)


def ssp_site_shapes(S):
    """shapes of the 33 tensors nn.Dropout sees in one S_SSP.forward of S sequences, in the reference's call order (include/vsrcap.h)"""
    sh = [(S, 1, 512), (S, 10, 512)]
    for _ in range(3):
        sh += [(S, 8, 10, 10), (S, 10, 512), (S, 10, 2048), (S, 10, 512)]
    sh.append((S, 11, 512))
    for _ in range(3):
        sh += [(S, 8, 11, 11), (S, 11, 512), (S, 8, 11, 10), (S, 11, 512), (S, 11, 2048), (S, 11, 512)]
    return sh


class RankPlan:
    """what SspEngine.rank_plan wrote and rank_finish reads: the plan buffer and the shape it was written for (kept on the host, so that
    rank_finish can size-check pred / assign against the plan without reading the device)"""

    def __init__(self, buf, N, MV, n_sink, Q):
        self.buf, self.N, self.MV, self.n_sink, self.Q = buf, N, MV, n_sink, Q


class SspEngine:
    def __init__(self, device):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_ssp_create(C.byref(self.h)))
        self._ws = None
        self._keep = {}

    def __del__(self):
        try:
            if self.h:
                self.lib.vsr_ssp_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, need):
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    @staticmethod
    def _f32(sd, key):
        t = sd[key]
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError("weight %s must be a contiguous fp32 GPU tensor (got %s %s)" % (key, t.dtype, t.device))
        return t.data_ptr()

    def bind_ssp(self, sd):
        """sd: state_dict-like mapping with the reference S_SSP's keys (models/sort_model.py)."""
        w = _lib.VsrSspWeights()
        for path, key in SSP_LAYOUT:
            _set_field(w, path, self._f32(sd, key))
        w.n_verbs = sd["v_embed_layer.weight"].shape[0]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_ssp_bind(self.h, C.byref(w), None))
        self._keep["ssp"] = sd
        self.ssp_binding = object()               # a new one per bind: a tape's backward must meet the binding of its forward

    def bind_sinkhorn(self, sd, N, n_iters, tau):
        w = _lib.VsrSinkhornWeights()
        for f in _lib.SINKHORN_FIELDS:
            name, wb = f.rsplit("_", 1)
            setattr(w, f, self._f32(sd, "%s.%s" % (name, "weight" if wb == "w" else "bias")))
        w.N, w.n_iters, w.tau = int(N), int(n_iters), float(tau)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_ssp_bind(self.h, None, C.byref(w)))
        self._keep["sinkhorn"] = sd
        self.N = int(N)
        self.sinkhorn_binding = object()          # a new one per bind: a tape's backward must meet the binding of its forward

    def generate(self, verbs, roles):
        """verbs (S,) int64, roles (S,10) int (0 = padding) on the GPU -> pred (S,10) int32, logp (S,10) fp32"""
        _need_gpu(verbs, "verbs")
        _need_gpu(roles, "roles")
        verbs = verbs.to(torch.int64).contiguous()
        roles = roles.to(torch.int32).contiguous()
        S = roles.size(0)
        if roles.dim() != 2 or roles.size(1) != 10 or verbs.numel() != S:
            raise RuntimeError("expected verbs (S,) and roles (S,10); got %s and %s" % (tuple(verbs.shape), tuple(roles.shape)))
        # the reference's embeddings raise IndexError for ids outside their tables (sort_model.py:108); the kernels would clamp
        lo, hi = int(roles.min()), int(roles.max())
        if lo < 0 or hi >= 26:
            raise IndexError("semantic-role ids must lie in [0, 26) (0 = padding); got [%d, %d]" % (lo, hi))
        pred = torch.empty(S, 10, dtype=torch.int32, device=self.device)
        logp = torch.empty(S, 10, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(self.lib.vsr_ssp_workspace_bytes(S))
            _lib.check(self.lib.vsr_ssp_generate(self.h, _ptr(verbs), _ptr(roles), S, _ptr(pred), _ptr(logp), _ptr(ws), ws.numel(), self._stream()))
        return pred, logp

    def sinkhorn_assign(self, seq, want_matrix=True):
        """seq (Q,N,2352) fp32 on the GPU -> (tr (Q,N,N) or None, assign (Q,N) int32)"""
        _need_gpu(seq, "seq")
        seq = seq.float().contiguous()
        Q = seq.size(0)
        if seq.dim() != 3 or seq.size(1) != self.N or seq.size(2) != 2352:
            raise RuntimeError("expected (Q, %d, 2352) rows; got %s" % (self.N, tuple(seq.shape)))
        tr = torch.empty(Q, self.N, self.N, dtype=torch.float32, device=self.device) if want_matrix else None
        assign = torch.empty(Q, self.N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(self.lib.vsr_sinkhorn_workspace_bytes(Q, self.N))
            _lib.check(self.lib.vsr_sinkhorn_assign(self.h, _ptr(seq), Q, _ptr(tr), _ptr(assign), _ptr(ws), ws.numel(), self._stream()))
        return tr, assign

    # ---- caption ranking on the device (include/vsrcap.h: vsr_rank_*)
    RANK_L = 10

    def _upload_ints(self, xs):
        """integer arrays as contiguous int32 GPU tensors.  Host arrays travel together in ONE non-blocking upload from pinned memory;
        tensors are converted where they live."""
        if all(isinstance(x, torch.Tensor) for x in xs):
            return [x.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous() for x in xs]
        host = [x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in xs]
        stage = torch.empty(sum(h.size for h in host), dtype=torch.int32, pin_memory=True)
        view, lo = stage.numpy(), 0
        for h in host:
            view[lo:lo + h.size] = h.reshape(-1)
            lo += h.size
        dev, lo, out = stage.to(self.device, non_blocking=True), 0, []
        for h in host:
            out.append(dev[lo:lo + h.size].view(h.shape))
            lo += h.size
        return out

    def _annotations(self, control_verb, det_seqs_v, det_seqs_sr, *more):
        """the three integer arrays (and any further ones, returned after them) as contiguous int32 GPU tensors (_upload_ints).  Only
        shapes are checked: the values are judged on the device (status)."""
        cv, dv, dsr, *more = self._upload_ints([control_verb, det_seqs_v, det_seqs_sr, *more])
        if cv.dim() != 2 or dv.dim() != 3 or dsr.dim() != 3 or dv.size(0) != cv.size(0) or dv.size(2) != cv.size(1) or tuple(dsr.shape[:2]) != tuple(dv.shape[:2]) or cv.size(0) == 0:
            raise RuntimeError("expected control_verb (N, MV), det_seqs_v (N, L, MV), det_seqs_sr (N, L, MS); got %s, %s, %s"
                               % (tuple(cv.shape), tuple(dv.shape), tuple(dsr.shape)))
        return (cv, dv, dsr, *more)

    def rank_plan(self, control_verb, det_seqs_v, det_seqs_sr, n_sink=None, n_verbs=None, max_items=None):
        """the scan of vsr_rank_plan -> (plan, job_verbs (S,) int64, job_roles (S,10) int32, item_gather (max_items, n_sink) int32) with
        S = N * MV padded job slots; n_sink / n_verbs default to the bound models'"""
        cv, dv, dsr = self._annotations(control_verb, det_seqs_v, det_seqs_sr)
        N, L, MV, MS = dv.size(0), dv.size(1), dv.size(2), dsr.size(2)
        n_sink = self.N if n_sink is None else int(n_sink)
        n_verbs = self._keep["ssp"]["v_embed_layer.weight"].shape[0] if n_verbs is None else int(n_verbs)
        max_items = int(max_items or 0)
        Q = max_items if max_items > 0 else N * MV * self.RANK_L
        with torch.cuda.device(self.device):
            plan = torch.empty(max(1, self.lib.vsr_rank_plan_bytes(N, MV, max_items)), dtype=torch.uint8, device=self.device)
            job_verbs = torch.empty(N * MV, dtype=torch.int64, device=self.device)
            job_roles = torch.empty(N * MV, self.RANK_L, dtype=torch.int32, device=self.device)
            item_gather = torch.empty(Q, max(n_sink, 1), dtype=torch.int32, device=self.device)
            _lib.check(self.lib.vsr_rank_plan(_ptr(cv), _ptr(dv), _ptr(dsr), N, L, MV, MS, n_sink, n_verbs, max_items, _ptr(job_verbs), _ptr(job_roles),
                                              _ptr(item_gather), _ptr(plan), plan.numel(), self._stream()))
        return RankPlan(plan, N, MV, n_sink, Q), job_verbs, job_roles, item_gather

    def rank_finish(self, plan, pred, assign, N=None, MV=None, max_items=None):
        """vsr_rank_finish: plan as rank_plan returned it, pred (N*MV, 10) and assign (max_items, n_sink) int32 on the GPU, as generate /
        sinkhorn_assign write them (or a caller's own decisions) -> (rank (N,10) int32, status (N,) int32).  The kernel indexes assign with
        the item bound stored in the plan, so the shapes are held to the plan's own (N, MV, n_sink, max_items); N / MV / max_items, when given,
        must be the plan's."""
        if not isinstance(plan, RankPlan):
            raise RuntimeError("rank_finish: plan must be what rank_plan returned")
        Q = plan.Q if max_items is None else (int(max_items) or plan.N * plan.MV * self.RANK_L)      # 0 = the static maximum, as in rank_plan
        if (N is not None and N != plan.N) or (MV is not None and MV != plan.MV) or (max_items is not None and Q != plan.Q):
            raise RuntimeError("rank_finish: the plan was written for N %d, MV %d, max_items %d" % (plan.N, plan.MV, plan.Q))
        N, MV, Q = plan.N, plan.MV, plan.Q
        for t, name in ((plan.buf, "plan"), (pred, "pred"), (assign, "assign")):
            _need_gpu(t, name)
        pred, assign = pred.to(torch.int32).contiguous(), assign.to(torch.int32).contiguous()
        if tuple(pred.shape) != (N * MV, self.RANK_L) or tuple(assign.shape) != (Q, plan.n_sink):
            raise RuntimeError("expected pred (%d, 10) and assign (%d, %d); got %s, %s" % (N * MV, Q, plan.n_sink, tuple(pred.shape), tuple(assign.shape)))
        rank = torch.empty(N, self.RANK_L, dtype=torch.int32, device=self.device)
        status = torch.empty(N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_rank_finish(_ptr(plan.buf), plan.buf.numel(), _ptr(pred), _ptr(assign), N, self.RANK_L, MV, plan.n_sink, _ptr(rank), _ptr(status),
                                                self._stream()))
        return rank, status

    def rank_captions(self, control_verb, det_seqs_v, det_seqs_sr, seqs_perm, max_items=None):
        """vsr_rank_captions: control_verb (N, MV), det_seqs_v (N, L, MV), det_seqs_sr (N, L, MS) ints (host arrays or tensors), seqs_perm
        (N, L, 2352) fp32 on the GPU -> (rank (N, L) int32, status (N,) int32) on the GPU; nothing is read back.  status: 0 = ranked; bit 1 no
        verb of the caption matches (the host path returns [] and the reference raises), 2 an item beyond max_items, 4 a role id outside
        [0, 26), 8 a verb outside the verb table - such a caption's row is all -1.  max_items: None = the static maximum N * MV * 10."""
        if "ssp" not in self._keep or "sinkhorn" not in self._keep:
            raise RuntimeError("rank_captions needs the S_SSP and the SinkhornNet weights bound on ONE engine (bind_ssp and bind_sinkhorn)")
        _need_gpu(seqs_perm, "seqs_perm")
        cv, dv, dsr = self._annotations(control_verb, det_seqs_v, det_seqs_sr)
        N, L, MV, MS = dv.size(0), dv.size(1), dv.size(2), dsr.size(2)
        if tuple(seqs_perm.shape) != (N, L, 2352):
            raise RuntimeError("expected seqs_perm (%d, %d, 2352); got %s" % (N, L, tuple(seqs_perm.shape)))
        seqs_perm = seqs_perm.float().contiguous()
        max_items = int(max_items or 0)
        rank = torch.empty(N, L, dtype=torch.int32, device=self.device)
        status = torch.empty(N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            need = self.lib.vsr_rank_workspace_bytes(N, MV, max_items, self.N)
            ws = self._workspace(max(need, 1))
            _lib.check(self.lib.vsr_rank_captions(self.h, _ptr(cv), _ptr(dv), _ptr(dsr), N, L, MV, MS, self.N, self._keep["ssp"]["v_embed_layer.weight"].shape[0],
                                                  _ptr(seqs_perm), max_items, _ptr(rank), _ptr(status), _ptr(ws), need, self._stream()))
        return rank, status

    # ---- training batches on the device (include/vsrcap.h: vsr_train_batch_plan, vsr_gather_rows)
    def train_batch_plan(self, control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v=None, gt_seqs_sr=None, idx_list=None, n_sink=10, n_verbs=None, max_items=None):
        """vsr_train_batch_plan: the annotations (host arrays or tensors; gt_seqs_v (N, Lg, MV) / gt_seqs_sr (N, Lg, MS) and idx_list (N, L)
        optional) -> a dict of GPU tensors at their padded sizes: verbs (N MV,) int64, det_roles / gt_roles (N MV, 10) int32 (gt_roles None
        without gt), item_gather (Q, n_sink) int32, tr_locs / gt_locs (Q, n_sink) fp32, item_key (Q, 3) int32 (all four None without
        idx_list; Q = max_items or N MV 10), counts (4,) int32, status (N,) int32.  Launches only: nothing is read back."""
        if (gt_seqs_v is None) != (gt_seqs_sr is None):
            raise RuntimeError("gt_seqs_v and gt_seqs_sr go together")
        more = ([gt_seqs_v, gt_seqs_sr] if gt_seqs_v is not None else []) + ([idx_list] if idx_list is not None else [])
        cv, dv, dsr, *more = self._annotations(control_verb, det_seqs_v, det_seqs_sr, *more)
        gv, gsr = more[:2] if gt_seqs_v is not None else (None, None)
        idx = more[-1] if idx_list is not None else None
        N, L, MV, MS = dv.size(0), dv.size(1), dv.size(2), dsr.size(2)
        if gv is not None and (gv.dim() != 3 or gsr.dim() != 3 or gv.size(0) != N or gv.size(2) != MV or tuple(gsr.shape) != (N, gv.size(1), MS)):
            raise RuntimeError("expected gt_seqs_v (%d, Lg, %d) and gt_seqs_sr (%d, Lg, %d); got %s, %s" % (N, MV, N, MS, tuple(gv.shape), tuple(gsr.shape)))
        if idx is not None:
            idx = idx.reshape(N, -1)
            if idx.size(1) != L:
                raise RuntimeError("expected idx_list (%d, %d); got %s" % (N, L, tuple(idx.shape)))
        Lg = gv.size(1) if gv is not None else 0
        if n_verbs is None:
            n_verbs = self._keep["ssp"]["v_embed_layer.weight"].shape[0]
        max_items = int(max_items or 0)
        S, Q = N * MV, max_items if max_items > 0 else N * MV * self.RANK_L
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        with torch.cuda.device(self.device):
            out = dict(verbs=new(S, torch.int64), det_roles=new((S, self.RANK_L), torch.int32), gt_roles=new((S, self.RANK_L), torch.int32) if gv is not None else None,
                       item_gather=None, tr_locs=None, gt_locs=None, item_key=None, counts=new(4, torch.int32), status=new(N, torch.int32))
            if idx is not None:
                out.update(item_gather=new((Q, int(n_sink)), torch.int32), tr_locs=new((Q, int(n_sink)), torch.float32), gt_locs=new((Q, int(n_sink)), torch.float32),
                           item_key=new((Q, 3), torch.int32))
            plan = torch.empty(max(1, self.lib.vsr_train_batch_plan_bytes(N, MV)), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.vsr_train_batch_plan(_ptr(cv), _ptr(dv), _ptr(dsr), _ptr(gv), _ptr(gsr), Lg, _ptr(idx), N, L, MV, MS, int(n_sink), int(n_verbs), max_items,
                                                     _ptr(out["verbs"]), _ptr(out["det_roles"]), _ptr(out["gt_roles"]), _ptr(out["item_gather"]), _ptr(out["tr_locs"]),
                                                     _ptr(out["gt_locs"]), _ptr(out["item_key"]), _ptr(out["counts"]), _ptr(out["status"]), _ptr(plan), plan.numel(),
                                                     self._stream()))
        return out

    def gather_rows(self, rows, gather):
        """vsr_gather_rows: rows (n_src, D) fp32 (D a multiple of 4), gather (...) int32, both on the GPU -> (..., D) fp32 with a zero row
        where gather < 0"""
        _need_gpu(rows, "rows")
        _need_gpu(gather, "gather")
        if rows.dim() != 2 or rows.dtype != torch.float32 or gather.dtype != torch.int32:
            raise RuntimeError("expected rows (n_src, D) fp32 and gather int32; got %s %s, %s" % (tuple(rows.shape), rows.dtype, gather.dtype))
        rows, gather = rows.contiguous(), gather.contiguous()
        out = torch.empty(tuple(gather.shape) + (rows.size(1),), dtype=torch.float32, device=self.device)
        if gather.numel() == 0:
            return out
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_gather_rows(_ptr(rows), rows.size(0), rows.size(1), _ptr(gather), gather.numel(), _ptr(out), self._stream()))
        return out

    # ---- SinkhornNet training (include/vsrcap.h: vsr_sinkhorn_train_*, vsr_sinkhorn_loc_loss)
    def _check_seq(self, seq):
        _need_gpu(seq, "seq")
        if seq.dim() != 3 or seq.size(1) != self.N or seq.size(2) != 2352 or seq.size(0) == 0:
            raise RuntimeError("expected (Q, %d, 2352) rows; got %s" % (self.N, tuple(seq.shape)))
        return seq.detach().float().contiguous()

    def sinkhorn_train_forward(self, seq):
        """seq (Q,N,2352) fp32 on the GPU -> (tr (Q,N,N), tape): tr has assign()'s bits; the tape (a uint8 tensor the caller owns)
        is what sinkhorn_train_backward needs of this forward"""
        seq = self._check_seq(seq)
        Q = seq.size(0)
        tr = torch.empty(Q, self.N, self.N, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            tape = torch.empty(self.lib.vsr_sinkhorn_tape_bytes(Q, self.N), dtype=torch.uint8, device=self.device)
            ws = self._workspace(self.lib.vsr_sinkhorn_train_workspace_bytes(Q, self.N))
            _lib.check(self.lib.vsr_sinkhorn_train_forward(self.h, _ptr(seq), Q, _ptr(tr), _ptr(tape), tape.numel(), _ptr(ws), ws.numel(), self._stream()))
        return tr, tape

    def sinkhorn_loc_loss(self, tr, tr_locs, gt_locs, scale=1.0, want_grad=True):
        """tr (Q,N,N), tr_locs / gt_locs (Q,N) -> (loss_items (Q,), d_tr (Q,N,N) or None): per-item MSE of tr_locs[q] @ tr[q] against
        gt_locs[q], and the gradient of scale * loss_items.sum() with respect to tr"""
        for t, name in ((tr, "tr"), (tr_locs, "tr_locs"), (gt_locs, "gt_locs")):
            _need_gpu(t, name)
        Q = tr.size(0)
        if tr.dim() != 3 or tuple(tr.shape[1:]) != (self.N, self.N) or tuple(tr_locs.shape) != (Q, self.N) or tuple(gt_locs.shape) != (Q, self.N) or Q == 0:
            raise RuntimeError("expected tr (Q, %d, %d) and tr_locs, gt_locs (Q, %d); got %s, %s, %s"
                               % (self.N, self.N, self.N, tuple(tr.shape), tuple(tr_locs.shape), tuple(gt_locs.shape)))
        tr, tr_locs, gt_locs = (t.detach().float().contiguous() for t in (tr, tr_locs, gt_locs))
        items = torch.empty(Q, dtype=torch.float32, device=self.device)
        d_tr = torch.empty_like(tr) if want_grad else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_sinkhorn_loc_loss(_ptr(tr), _ptr(tr_locs), _ptr(gt_locs), Q, self.N, float(scale), _ptr(items), _ptr(d_tr), self._stream()))
        return items, d_tr

    def sinkhorn_train_backward(self, seq, tape, d_tr, binding=None):
        """-> the ten parameter gradients in the order of _lib.SINKHORN_FIELDS (fresh tensors: the library overwrites).  binding: the
        engine's sinkhorn_binding at the time of the forward that wrote the tape; a bind_sinkhorn() since then raises"""
        if binding is not None and binding is not self.sinkhorn_binding:
            raise RuntimeError("SinkhornNet backward: bind_sinkhorn() was called between this forward and its backward - the tape belongs "
                               "to the earlier weights / N / n_iters / tau")
        seq = self._check_seq(seq)
        _need_gpu(d_tr, "d_tr")
        Q = seq.size(0)
        if tuple(d_tr.shape) != (Q, self.N, self.N):
            raise RuntimeError("expected d_tr (%d, %d, %d); got %s" % (Q, self.N, self.N, tuple(d_tr.shape)))
        d_tr = d_tr.detach().float().contiguous()
        sd = self._keep["sinkhorn"]
        g = _lib.VsrSinkhornGrads()
        out = []
        for f in _lib.SINKHORN_FIELDS:
            name, wb = f.rsplit("_", 1)
            t = torch.empty_like(sd["%s.%s" % (name, "weight" if wb == "w" else "bias")])
            setattr(g, f, t.data_ptr())
            out.append(t)
        with torch.cuda.device(self.device):
            ws = self._workspace(self.lib.vsr_sinkhorn_train_workspace_bytes(Q, self.N))
            _lib.check(self.lib.vsr_sinkhorn_train_backward(self.h, _ptr(seq), Q, _ptr(tape), tape.numel(), _ptr(d_tr), C.byref(g), _ptr(ws), ws.numel(),
                                                            self._stream()))
        return out


    # ---- S_SSP training (include/vsrcap.h: vsr_ssp_train_*, vsr_ssp_mask_*, vsr_ssp_dropout_masks)
    def ssp_mask_layout(self, S):
        """[(byte offset, shape)] of the 33 dropout sites in the mask buffer of S sequences (1 = keep, each site contiguous from a
        16-byte boundary) and the buffer's size"""
        S = int(S)
        return [(self.lib.vsr_ssp_mask_offset(S, i), sh) for i, sh in enumerate(ssp_site_shapes(S))], self.lib.vsr_ssp_mask_bytes(S)

    def ssp_dropout_masks(self, S, seed, p=SSP_DROPOUT_P):
        """the library's masks of `seed` for S sequences: a uint8 GPU tensor of vsr_ssp_mask_bytes(S) bytes"""
        S = int(S)
        with torch.cuda.device(self.device):
            masks = torch.empty(self.lib.vsr_ssp_mask_bytes(S), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.vsr_ssp_dropout_masks(int(seed) & (2 ** 64 - 1), float(p), S, _ptr(masks), self._stream()))
        return masks

    def _check_ssp_batch(self, verbs, roles, gt, masks):
        for t, name in ((verbs, "this_verb"), (roles, "det_seqs_sr"), (gt, "gt_seqs_sr")):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError("%s must be a tensor on the GPU" % name)
            _need_gpu(t, name)
        S = roles.size(0) if roles.dim() == 2 else 0
        if S < 1 or tuple(roles.shape) != (S, 10) or tuple(gt.shape) != (S, 10) or tuple(verbs.shape) not in ((S,), (S, 1)):
            raise RuntimeError("expected this_verb (S,1) or (S,), det_seqs_sr (S,10), gt_seqs_sr (S,10) with S >= 1; got %s, %s, %s"
                               % (tuple(verbs.shape), tuple(roles.shape), tuple(gt.shape)))
        verbs = verbs.detach().to(torch.int64).reshape(-1).contiguous()
        roles, gt = roles.detach().to(torch.int32).contiguous(), gt.detach().to(torch.int32).contiguous()
        # the reference's embeddings raise IndexError for ids outside their tables (sort_model.py:81-83); the kernels would read row 0
        lo, hi = int(torch.minimum(roles.min(), gt.min())), int(torch.maximum(roles.max(), gt.max()))
        if lo < 0 or hi >= 26:
            raise IndexError("semantic-role ids must lie in [0, 26) (0 = padding); got [%d, %d]" % (lo, hi))
        n_verbs = self._keep["ssp"]["v_embed_layer.weight"].shape[0]
        v = verbs % 10000
        if int(v.min()) < 0 or int(v.max()) >= n_verbs:
            raise IndexError("verb ids %% 10000 must lie in [0, %d); got [%d, %d]" % (n_verbs, int(v.min()), int(v.max())))
        if masks is not None:
            _need_gpu(masks, "dropout_masks")
            need = self.lib.vsr_ssp_mask_bytes(S)
            if masks.dtype != torch.uint8 or masks.dim() != 1 or masks.numel() != need or not masks.is_contiguous():
                raise RuntimeError("dropout_masks must be a contiguous uint8 buffer of %d bytes (ssp_mask_layout(%d)); got %s %s"
                                   % (need, S, masks.dtype, tuple(masks.shape)))
        return verbs, roles, gt

    def _one_hot(self):
        t = self._keep["ssp"]["label_smooth.one_hot"]
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != 26:
            raise RuntimeError("label_smooth.one_hot must be a contiguous fp32 GPU buffer of 26 values")
        return t

    def ssp_train_forward(self, verbs, roles, gt, masks=None, p=SSP_DROPOUT_P, checked=False):
        """S_SSP.forward for S sequences -> (loss, a 0-d fp32 GPU tensor; tape, a uint8 tensor the caller owns: what ssp_train_backward
        needs of this forward).  masks: None (no dropout) or a buffer laid out as ssp_mask_layout(S) says.  checked: the ids and masks
        are _check_ssp_batch's own results (its range checks read the device: once per step is enough)"""
        if not checked:
            verbs, roles, gt = self._check_ssp_batch(verbs, roles, gt, masks)
        S = roles.size(0)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            tape = torch.empty(self.lib.vsr_ssp_tape_bytes(S), dtype=torch.uint8, device=self.device)
            ws = self._workspace(self.lib.vsr_ssp_train_workspace_bytes(S))
            _lib.check(self.lib.vsr_ssp_train_forward(self.h, _ptr(verbs), _ptr(roles), _ptr(gt), S, _ptr(masks), float(p), _ptr(self._one_hot()), _ptr(loss),
                                                      _ptr(tape), tape.numel(), _ptr(ws), ws.numel(), self._stream()))
        return loss, tape

    def ssp_relu_gates(self, S, tape):
        """TEST ONLY (the tape's layout is private): the six ReLU gate patterns of the forward that wrote `tape` (encoder layers 0..2, decoder layers 0..2): bool (rows, 2048),
        True where the unit passed (and, with dropout, was kept)"""
        out = []
        for dec in (0, 1):
            rows = int(S) * (11 if dec else 10)
            for l in range(3):
                off = self.lib.vsr_ssp_tape_ff_offset(int(S), dec, l)
                out.append(tape[off:off + rows * 2048 * 4].view(torch.float32).view(rows, 2048) > 0)
        return out

    def ssp_train_backward(self, verbs, roles, gt, masks, tape, d_loss, binding=None, checked=False):
        """-> the gradients of SSP_PARAM_KEYS, in that order (fresh tensors: the library overwrites).  d_loss: a 0-d GPU tensor, read on
        the device.  binding: the engine's ssp_binding at the time of the forward that wrote the tape; a bind_ssp() since then raises"""
        if binding is not None and binding is not self.ssp_binding:
            raise RuntimeError("S_SSP backward: bind_ssp() was called between this forward and its backward - the tape belongs to the earlier weights")
        if not checked:
            verbs, roles, gt = self._check_ssp_batch(verbs, roles, gt, masks)
        _need_gpu(d_loss, "d_loss")
        if d_loss.numel() != 1:
            raise RuntimeError("expected a scalar d_loss; got %s" % (tuple(d_loss.shape),))
        d_loss = d_loss.detach().float().contiguous()
        S = roles.size(0)
        sd = self._keep["ssp"]
        g = _lib.VsrSspGrads()
        out = []
        for path, key in SSP_LAYOUT:
            t = torch.empty_like(sd[key])
            _set_field(g, path, t.data_ptr())
            out.append(t)
        g.n_verbs = sd["v_embed_layer.weight"].shape[0]
        with torch.cuda.device(self.device):
            ws = self._workspace(self.lib.vsr_ssp_train_workspace_bytes(S))
            _lib.check(self.lib.vsr_ssp_train_backward(self.h, _ptr(verbs), _ptr(roles), _ptr(gt), S, _ptr(masks), _ptr(tape), tape.numel(), _ptr(d_loss),
                                                       C.byref(g), _ptr(ws), ws.numel(), self._stream()))
        return out


def _no_double_backward(what):
    if torch.is_grad_enabled():
        raise RuntimeError("%s: create_graph=True is not supported - the backward is a hand-written HIP pass with no graph of its own" % what)


class SinkhornTrainFn(torch.autograd.Function):
    """tr = SinkhornNet(seq) with a grad_fn.  The tape of a forward lives on its ctx, not in the engine: several forwards may be alive
    at once ((l1 + l2).backward(), micro-batches, an assign() in between).  params: the ten parameters in _lib.SINKHORN_FIELDS order -
    the library reads their storage live; they go through save_for_backward so that autograd's in-place check applies."""

    @staticmethod
    def forward(ctx, eng, seq, *params):
        tr, tape = eng.sinkhorn_train_forward(seq)
        ctx.eng, ctx.tape, ctx.binding = eng, tape, eng.sinkhorn_binding
        ctx.save_for_backward(seq, *params)
        return tr

    # once_differentiable sits on _backward, not here: its wrapper runs the function under no_grad, which would hide create_graph=True
    # (grad mode still enabled at this point) from the check below
    @staticmethod
    def backward(ctx, d_tr):
        _no_double_backward("SinkhornNet.forward")
        return SinkhornTrainFn._backward(ctx, d_tr)

    @staticmethod
    @once_differentiable
    def _backward(ctx, d_tr):
        seq = ctx.saved_tensors[0]
        grads = ctx.eng.sinkhorn_train_backward(seq, ctx.tape, d_tr, ctx.binding)
        return (None, None) + tuple(g if ctx.needs_input_grad[2 + i] else None for i, g in enumerate(grads))


class SinkhornLocLossFn(torch.autograd.Function):
    """scale * sum_q MSELoss(tr_locs[q] @ SinkhornNet(seq)[q], gt_locs[q]): forward, fused loss and (at backward time) the
    hand-written backward - three library calls for all Q items.  The sum over items is torch.sum over the (Q,) buffer.  tr_locs and
    gt_locs are data: they get no gradient, and SinkhornNet.loc_loss raises when either asks for one."""

    @staticmethod
    def forward(ctx, eng, seq, tr_locs, gt_locs, scale, *params):
        tr, tape = eng.sinkhorn_train_forward(seq)
        items, d_tr = eng.sinkhorn_loc_loss(tr, tr_locs, gt_locs, scale)
        ctx.eng, ctx.tape, ctx.d_tr, ctx.binding = eng, tape, d_tr, eng.sinkhorn_binding
        ctx.save_for_backward(seq, *params)
        return items.sum() * scale

    @staticmethod
    def backward(ctx, d_loss):                    # undecorated for the same reason as SinkhornTrainFn.backward
        _no_double_backward("SinkhornNet.loc_loss")
        return SinkhornLocLossFn._backward(ctx, d_loss)

    @staticmethod
    @once_differentiable
    def _backward(ctx, d_loss):
        seq = ctx.saved_tensors[0]
        grads = ctx.eng.sinkhorn_train_backward(seq, ctx.tape, ctx.d_tr * d_loss, ctx.binding)
        return (None,) * 5 + tuple(g if ctx.needs_input_grad[5 + i] else None for i, g in enumerate(grads))


class SspTrainFn(torch.autograd.Function):
    """loss = S_SSP.forward(verbs, roles, gt) with a grad_fn.  The tape and the dropout masks of a forward live on its ctx, not in the
    engine: several forwards may be alive at once ((l1 + l2).backward(), micro-batches, a generate() in between).  params: the
    parameters of SSP_PARAM_KEYS in that order - the library reads their storage live; they go through save_for_backward so that
    autograd's in-place check applies.  The ids are data (no gradient) and arrive checked (SspEngine._check_ssp_batch)."""

    @staticmethod
    def forward(ctx, eng, verbs, roles, gt, masks, p, *params):
        loss, tape = eng.ssp_train_forward(verbs, roles, gt, masks, p, checked=True)
        ctx.eng, ctx.tape, ctx.masks, ctx.binding = eng, tape, masks, eng.ssp_binding
        ctx.ids = (verbs, roles, gt)
        ctx.save_for_backward(*params)
        return loss

    @staticmethod
    def backward(ctx, d_loss):                    # undecorated for the same reason as SinkhornTrainFn.backward
        _no_double_backward("S_SSP.forward")
        return SspTrainFn._backward(ctx, d_loss)

    @staticmethod
    @once_differentiable
    def _backward(ctx, d_loss):
        ctx.saved_tensors                         # (autograd's check that no parameter was modified in place since the forward)
        grads = ctx.eng.ssp_train_backward(*ctx.ids, ctx.masks, ctx.tape, d_loss, ctx.binding, checked=True)
        return (None,) * 6 + tuple(g if ctx.needs_input_grad[6 + i] else None for i, g in enumerate(grads))
