"""Shared by the S-SSP training tests and tests/golden/make_golden_ssp_train.py: the training oracle of S_SSP.forward
(models/sort_model.py:80-103) - oracle/ssp_oracle.py's two stacks restated with the 33 dropout sites of the reference's call order
and the label-smoothed KL loss - run under torch autograd in fp64 or fp32, the synthetic ground-truth orders, and the summary of
the gradients the fixture stores.

Dropout is DATA here as in the library: site i receives a 0/1 array of the shape SITE table gives it and applies x * keep / (1 - p).
The generator replaces nn.Dropout.forward of the real reference by the same function and asserts the call order and shapes."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import ssp_oracle as so
from vsrcap import synth

P_DROP = 0.1
N_SITES = 33
N_POS = 32                           # positions of every gradient tensor a summary keeps
CONFIDENCE = 0.9                     # LabelSmoothingKLDivLoss(0.1, 26): 1 - label_smoothing at the target ...
OFF_TARGET = float(np.float32(0.1 / 24))     # ... and its fp32 `one_hot` buffer (0.1 / (26 - 2)) everywhere else


def site_shapes(S):
    """shapes of the 33 tensors nn.Dropout sees in one S_SSP.forward of S sequences, in call order"""
    H, FF, Te, Td = so.HID, so.FF, so.MAXLEN, so.MAXLEN + 1
    sh = [(S, 1, H), (S, Te, H)]
    for _ in range(3):
        sh += [(S, so.HEADS, Te, Te), (S, Te, H), (S, Te, FF), (S, Te, H)]
    sh.append((S, Td, H))
    for _ in range(3):
        sh += [(S, so.HEADS, Td, Td), (S, Td, H), (S, so.HEADS, Td, Te), (S, Td, H), (S, Td, FF), (S, Td, H)]
    assert len(sh) == N_SITES
    return sh


def hash_masks(S, seed):
    """the generator's masks: site i keeps element n iff synth.hash_u01(n, 2000 + i, seed) >= p"""
    return [(synth.hash_u01(int(np.prod(sh)), 2000 + i, seed) >= P_DROP).astype(np.uint8).reshape(sh) for i, sh in enumerate(site_shapes(S))]


def apply_keep(x, keep):
    return x * keep.to(x.dtype) / (1.0 - P_DROP)


def make_gt(roles, seed):
    """(S, 10) ground-truth orders: per sequence a hashed permutation of its roles, zero padded; every fourth sequence with more than
    two roles loses its last one or two (the caption names fewer roles of the verb than were detected: train_region_sort.py:158-164
    fills the two rows independently)"""
    roles = np.asarray(roles)
    gt = np.zeros_like(roles)
    cut = synth.hash_int(len(roles), 1, 3, 2101, seed)
    for s, row in enumerate(roles):
        n = int((row != 0).sum())
        order = np.argsort(synth.hash_u01(n, 2200 + s, seed))
        keep = n - int(cut[s]) if (s % 4 == 1 and n > 2) else n
        gt[s, :keep] = row[:n][order][:keep]
    return gt


class TrainOracle(so.SSPOracle):
    def run(self, verbs, roles, gt, masks, pin=None, pre_acts=None):
        """pre_acts (a list): receives the six ReLU pre-activations (rows, 2048), encoder layers then decoder layers.
        pin: six (band, gate) pairs of bool (rows, 2048): inside `band` the unit passes iff `gate` instead of iff its pre-activation
        is positive (see pinned_reference)"""
        ff_index = iter(range(6))
        S, dev = roles.shape[0], roles.device                                  # (tools/ssp_train_bench.py runs this on the GPU)
        assert masks is None or len(masks) == N_SITES
        site = iter(range(N_SITES))

        def drop(x):
            i = next(site)
            if masks is None:
                return x
            keep = masks[i] if isinstance(masks[i], torch.Tensor) else torch.as_tensor(np.asarray(masks[i]))
            assert tuple(keep.shape) == tuple(x.shape), (i, tuple(keep.shape), tuple(x.shape))
            return apply_keep(x, keep)

        def mha(pre, q_in, kv_in, allowed):
            Tq, Tk, hd = q_in.shape[1], kv_in.shape[1], so.HID // so.HEADS
            q = self._lin(q_in, pre + ".linear_Q").view(S, Tq, so.HEADS, hd).transpose(1, 2)
            k = self._lin(kv_in, pre + ".linear_K").view(S, Tk, so.HEADS, hd).transpose(1, 2)
            v = self._lin(kv_in, pre + ".linear_V").view(S, Tk, so.HEADS, hd).transpose(1, 2)
            logits = q @ k.transpose(-2, -1) / math.sqrt(hd)
            if allowed is not None:
                logits = logits.masked_fill(~allowed.unsqueeze(1), -1e3)
            w = drop(F.softmax(logits, -1))                                   # dropout on the softmax OUTPUT, no renormalisation
            return self._lin((w @ v).transpose(1, 2).reshape(S, Tq, so.HID), pre + ".linear_O")

        def ff(pre, y):
            x = self._lin(y, pre + ".ff_layer.w_1")
            i = next(ff_index)
            if pre_acts is not None:
                pre_acts.append(x.detach().double().reshape(-1, so.FF))
            if pin is None:
                h = F.relu(x)
            else:
                band, gate = pin[i]
                h = x * torch.where(band, gate, x.detach().reshape(-1, so.FF) > 0).reshape(x.shape).to(x.dtype)
            return self._lin(drop(h), pre + ".ff_layer.w_2")

        p, sc = self.p, math.sqrt(so.HID)
        ve = drop(p["v_embed_layer.weight"][(verbs % 10000).long()].unsqueeze(1) * sc)
        x = self._lin(ve + drop(p["sr_embed_layer.weight"][roles.long()] * sc), "encoder.fc_feat")
        for l in range(3):
            pre = "encoder.encoder_layers.%d" % l
            y = self._ln(x, pre + ".layer_norm1")
            x1 = drop(mha(pre + ".attention", y, y, None)) + x
            x = drop(ff(pre, self._ln(x1, pre + ".layer_norm2"))) + x1
        prior = self._ln(x, "encoder.layer_norm")

        tok = torch.cat([torch.zeros(S, 1, dtype=torch.int64, device=dev), gt.long()], 1)              # [bos = 0, gt_0 .. gt_9]
        Td = tok.shape[1]
        x = drop(p["sr_embed_layer.weight"][tok] * sc)
        allowed = torch.tril(torch.ones(Td, Td, dtype=torch.bool, device=dev)).unsqueeze(0) & (tok != 0).unsqueeze(1)
        for l in range(3):
            pre = "decoder.encoder_layers.%d" % l
            h = self._ln(x, pre + ".layer_norm1")
            h1 = drop(mha(pre + ".attention", h, h, allowed)) + x
            h = self._ln(h1, pre + ".layer_norm2")
            h2 = drop(mha(pre + ".attention", h, prior, None)) + h1           # the SAME projections (sort_modules.py:87)
            x = drop(ff(pre, self._ln(h2, pre + ".layer_norm3"))) + h2
        states = self._ln(x, "decoder.layer_norm")
        assert next(site, None) is None

        logp = F.log_softmax(self._lin(states, "expander_nn"), -1)            # (S, 11, 26)
        tgt = torch.cat([gt.long(), torch.zeros(S, 1, dtype=torch.int64, device=dev)], 1)
        m = torch.cat([torch.ones(S, 1, dtype=torch.bool, device=dev), gt != 0], 1).to(self.dtype)   # decoder_mask[:, :-1] = [1, gt_0 != 0 .. gt_9 != 0]
        q = torch.full(logp.shape, OFF_TARGET, dtype=self.dtype, device=dev).scatter_(2, tgt.unsqueeze(-1), CONFIDENCE)
        return (m.unsqueeze(-1) * q * (q.log() - logp)).sum() / m.sum()


def oracle_run(w, verbs, roles, gt, masks, dtype, pin=None):
    """S_SSP.forward + backward of the oracle in `dtype`: dict(loss=float, grads={state_dict key: fp64 tensor}, pre=[the six ReLU
    pre-activations as fp64]) over the parameters the loss depends on (decoder.*.cross_attention.* is never called: absent, as its
    .grad stays None under the reference).  masks: None (eval mode) or the 33 keep arrays of site_shapes(S).  pin: TrainOracle.run"""
    o = TrainOracle(w, dtype=dtype)
    for k in o.p:
        o.p[k] = o.p[k].clone().requires_grad_(True)
    pre = []
    loss = o.run(torch.as_tensor(np.asarray(verbs)), torch.as_tensor(np.asarray(roles)), torch.as_tensor(np.asarray(gt)), masks, pin, pre)
    loss.backward()
    return dict(loss=float(loss.item()), grads={k: v.grad.detach().double() for k, v in o.p.items() if v.grad is not None}, pre=pre)


KINK_MARGIN = 16.0                    # grad_compare.MARGIN, applied to the pre-activations


def pinned_reference(r64, r32, device_gates, rerun, masks=None):
    """The loss is piecewise smooth: d w_1 and d b_1 of a feed-forward unit JUMP where one of its pre-activations crosses zero, by the
    whole contribution of that row.  S = 64 has 8.3 M pre-activations of size ~1; the fp32 oracle's differ from the fp64 oracle's by
    up to 4e-6 (rms 7e-7), so about eight of them change sign between the two oracles in every run, and as many between any other fp32
    evaluation and fp64 - each a legitimate rounding of the forward, each moving one row of a w_1 gradient by ~1e-3 of the tensor's
    scale.  No bound built on rounding error can hold across such a jump, so the comparison is made on ONE side of every kink: where
    the fp64 pre-activation lies within KINK_MARGIN x the fp32 oracle's own largest pre-activation error of zero (about 6e-5: a few
    hundred units of 8.3 M), both oracles take the side the device took (its gate, from the tape); everywhere else, and in all that
    follows the gate, they are unchanged.  Nothing is excluded from the comparison, and the fp32 yardstick loses its own flips.

    r64, r32: oracle_run's results without pins.  device_gates: six bool (rows, 2048).  rerun(dtype, pin) -> oracle_run's result.
    masks: the run's 33 keep arrays or None (a dropped unit has no side to take).
    Returns (r64, r32, number of pinned units whose side changed).

    The pin can absorb only what this argument says, which two assertions hold it to:
      - OUTSIDE the band every (kept) unit's device gate is the sign of the fp64 pre-activation: a device that gates wrongly anywhere
        rounding cannot explain it fails here;
      - INSIDE the band the number of units whose side changes is at most the number a rounding of the oracle's OWN size can flip -
        the units whose fp64 pre-activation lies within the fp32 oracle's largest pre-activation error of zero - plus the fp32
        oracle's own flips (they are pinned too).  Both counts come from the two oracles alone (S = 64: about 27 + 8)."""
    err32 = max(float((a - b).abs().max()) for a, b in zip(r64["pre"], r32["pre"]))
    tol = KINK_MARGIN * err32
    pin, moved, wrong_outside, ceiling = [], 0, 0, 0
    relu_sites = [4, 8, 12, 19, 25, 31]
    for i, (x64, x32, gate) in enumerate(zip(r64["pre"], r32["pre"], device_gates)):
        kept = torch.ones_like(x64, dtype=torch.bool) if masks is None else torch.as_tensor(np.asarray(masks[relu_sites[i]])).reshape(x64.shape) != 0
        band = kept & (x64.abs() < tol)
        gate = torch.as_tensor(gate).cpu().reshape(x64.shape)
        moved += int((band & ((gate != (x64 > 0)) | (gate != (x32 > 0)))).sum())
        wrong_outside += int((kept & ~band & (gate != (x64 > 0))).sum())
        ceiling += int((kept & (x64.abs() < err32)).sum()) + int((kept & ((x32 > 0) != (x64 > 0))).sum())
        pin.append((band, gate))
    assert wrong_outside == 0, "%d device ReLU gates differ from the fp64 oracle's outside the rounding band |x| < %.2e" % (wrong_outside, tol)
    assert moved <= ceiling, "%d pinned units changed side; roundings of the oracle's own size explain at most %d" % (moved, ceiling)
    if moved == 0:
        return r64, r32, 0
    return rerun(torch.float64, pin), rerun(torch.float32, pin), moved


def summarise(run):
    """what g17_ssp_train.npz holds of one run: the loss and, of every gradient tensor, its L2 norm and its values at N_POS positions
    (synth.hash_int on a stream fixed per tensor, in the sorted order of the names)"""
    out = {"loss": torch.tensor([run["loss"]], dtype=torch.float64)}
    for i, k in enumerate(sorted(run["grads"])):
        g = torch.as_tensor(run["grads"][k]).double().reshape(-1)
        pos = torch.from_numpy(synth.hash_int(N_POS, 0, g.numel(), 2300 + i, 0))
        out[k + "/norm"] = g.pow(2).sum().sqrt().reshape(1)
        out[k + "/at"] = g[pos].clone()
    return out


def pack(summary, names):
    """a summary's gradient part as one (len(names), 1 + N_POS) array [norm | values]: one zip member instead of two per tensor"""
    return np.stack([np.concatenate([summary[k + "/norm"].numpy(), summary[k + "/at"].numpy()]) for k in names]).astype(np.float64)


def unpack(arr, names, loss):
    out = {"loss": torch.tensor([loss], dtype=torch.float64)}
    for k, row in zip(names, np.asarray(arr)):
        out[k + "/norm"] = torch.from_numpy(row[:1].copy())
        out[k + "/at"] = torch.from_numpy(row[1:].copy())
    return out
