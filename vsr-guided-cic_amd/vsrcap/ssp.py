"""Host driver of the ordering-model entry points of libvsrcap.so (include/vsrcap.h: vsr_ssp_*, vsr_sinkhorn_*): one
vsr_ssp object per device, weights borrowed from torch parameters, work enqueued on torch's current stream.  No fallback:
CPU tensors raise.

SinkhornNet trains through SinkhornTrainFn (one forward / one hand-written backward for all Q items of a loader batch) and
sinkhorn_loc_loss (the fused location loss of coco_scripts/train_sinkhorn.py:207-209)."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s); this path has no CPU implementation" % (name, t.device))


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
        def layer(pre, dec):
            vals = {}
            for i in (1, 2, 3):
                for wb, f in (("weight", "w"), ("bias", "b")):
                    vals["ln%d_%s" % (i, f)] = self._f32(sd, "%s.layer_norm%d.%s" % (pre, i, wb)) if (i < 3 or dec) else 0
            for q in "QKVO":
                vals["W" + q.lower()] = self._f32(sd, "%s.attention.linear_%s.weight" % (pre, q))
                vals["b" + q.lower()] = self._f32(sd, "%s.attention.linear_%s.bias" % (pre, q))
            vals["W1"], vals["b1"] = self._f32(sd, pre + ".ff_layer.w_1.weight"), self._f32(sd, pre + ".ff_layer.w_1.bias")
            vals["W2"], vals["b2"] = self._f32(sd, pre + ".ff_layer.w_2.weight"), self._f32(sd, pre + ".ff_layer.w_2.bias")
            return _lib.VsrSspLayer(**vals)
        w = _lib.VsrSspWeights()
        w.sr_embed, w.v_embed = self._f32(sd, "sr_embed_layer.weight"), self._f32(sd, "v_embed_layer.weight")
        w.n_verbs = sd["v_embed_layer.weight"].shape[0]
        w.fc_w, w.fc_b = self._f32(sd, "encoder.fc_feat.weight"), self._f32(sd, "encoder.fc_feat.bias")
        for l in range(3):
            w.enc[l] = layer("encoder.encoder_layers.%d" % l, False)
            w.dec[l] = layer("decoder.encoder_layers.%d" % l, True)
        w.enc_ln_w, w.enc_ln_b = self._f32(sd, "encoder.layer_norm.weight"), self._f32(sd, "encoder.layer_norm.bias")
        w.dec_ln_w, w.dec_ln_b = self._f32(sd, "decoder.layer_norm.weight"), self._f32(sd, "decoder.layer_norm.bias")
        w.exp_w, w.exp_b = self._f32(sd, "expander_nn.weight"), self._f32(sd, "expander_nn.bias")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsr_ssp_bind(self.h, C.byref(w), None))
        self._keep["ssp"] = sd

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
