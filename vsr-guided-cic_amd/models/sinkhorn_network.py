"""SinkhornNet (region ordering inside a semantic role) on MI355X: the reference's class surface over libvsrcap.so.

Mirrors /root/reference/models/sinkhorn_network.py:5-51: constructor (N, n_iters, tau), the five Linear layers (identical
state_dict keys, so eval_coco.py:102 loads 'saved_model/coco_sinkhorn/model-sh.pth'), forward(seq (b, N, 2352)) -> the
doubly-normalised (b, N, N) matrix.  `assign(seq)` additionally returns the assignment eval_coco.py:185-189 computes with
munkres on the host, for all items at once (vsr_sinkhorn_assign).

Training (coco_scripts/train_sinkhorn.py:137-215): with grad enabled and a parameter that requires grad, forward(seq) returns tr
with a grad_fn (hand-written HIP backward), so the script's torch.mm / nn.MSELoss / backward lines work on it unchanged;
loc_loss(seq, tr_locs, gt_locs, scale) is the same loss for all Q items of a loader batch in three library calls.  No gradient flows
to seq (nor to loc_loss's tr_locs / gt_locs), and create_graph=True is not supported: each raises."""
import torch
from torch import nn


class SinkhornNet(nn.Module):
    def __init__(self, N, n_iters, tau):
        super().__init__()
        self.N = N
        self.n_iters = n_iters
        self.tau = tau
        self.W1_txt = nn.Linear(300, 128)
        self.W1_vis = nn.Linear(2048, 512)
        self.W2_vis = nn.Linear(512, 128)
        self.W_fc_pos = nn.Linear(260, 256)
        self.W_fc = nn.Linear(256, N)
        self.init_weights()
        self._eng = None

    def init_weights(self):
        for m in (self.W1_txt, self.W1_vis, self.W2_vis, self.W_fc_pos, self.W_fc):
            nn.init.xavier_normal_(m.weight)
            nn.init.constant_(m.bias, 0)

    def _engine(self, device):
        if device.type != 'cuda':
            raise RuntimeError("SinkhornNet (MI355X build) computes only on the GPU: move the model and its inputs to 'cuda'. There is no CPU fallback.")
        from vsrcap.ssp import SspEngine
        key = tuple(p.data_ptr() for p in self.parameters())
        if self._eng is None or self._key != key:
            self._eng = SspEngine(device)
            self._eng.bind_sinkhorn({k: v.data for k, v in self.state_dict(keep_vars=True).items()}, self.N, self.n_iters, self.tau)
            self._key = key
        return self._eng

    def assign(self, seq):
        """seq (Q, N, 2352) -> (tr (Q,N,N), assign (Q,N) int64): assign[q][i] = column paired with row i of tr[q]^T"""
        eng = self._engine(seq.device)
        tr, a = eng.sinkhorn_assign(seq, want_matrix=True)
        return tr, a.long()

    # SinkhornNet.forward under autograd supports at most this many Sinkhorn iterations (the divisor tape of the library: SH_TRAIN_MAX_ITERS)
    TRAIN_MAX_ITERS = 64

    def _training_call(self, seq, **locs):
        """the engine and the ten parameters (in the library's field order) of a differentiable call; raises what cannot be differentiated"""
        eng = self._engine(seq.device)
        for name, t in dict(seq=seq, **locs).items():
            if t.requires_grad:
                raise RuntimeError("SinkhornNet (MI355X build): the gradient with respect to %s is not implemented (train_sinkhorn.py "
                                   "never asks for it); pass %s.detach()" % (name, name))
        if self.n_iters > self.TRAIN_MAX_ITERS:
            raise RuntimeError("SinkhornNet (MI355X build): training supports n_iters <= %d; got %d" % (self.TRAIN_MAX_ITERS, self.n_iters))
        from vsrcap._lib import SINKHORN_FIELDS
        params = []
        for f in SINKHORN_FIELDS:
            name, wb = f.rsplit("_", 1)
            params.append(getattr(getattr(self, name), "weight" if wb == "w" else "bias"))
        return eng, params

    def _wants_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def forward(self, seq):
        if not self._wants_grad():
            return self.assign(seq)[0]
        from vsrcap.ssp import SinkhornTrainFn
        eng, params = self._training_call(seq)
        return SinkhornTrainFn.apply(eng, seq, *params)

    def loc_loss(self, seq, tr_locs, gt_locs, scale=1.0):
        """scale * sum_q MSELoss(tr_locs[q] @ forward(seq)[q], gt_locs[q]) - train_sinkhorn.py:207-211 with scale = 1 / batch_size -
        for all Q items at once.  seq (Q, N, 2352), tr_locs / gt_locs (Q, N); a scalar with a grad_fn when the net is being trained."""
        from vsrcap.ssp import SinkhornLocLossFn
        if not self._wants_grad():
            eng = self._engine(seq.device)
            tr = eng.sinkhorn_assign(seq, want_matrix=True)[0]
            return eng.sinkhorn_loc_loss(tr, tr_locs, gt_locs, scale, want_grad=False)[0].sum() * float(scale)
        eng, params = self._training_call(seq, tr_locs=tr_locs, gt_locs=gt_locs)
        return SinkhornLocLossFn.apply(eng, seq, tr_locs, gt_locs, float(scale), *params)
