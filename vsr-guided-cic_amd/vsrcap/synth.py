"""Closed-form synthetic weights and inputs for the VSR captioning decoder.

Everything here is a pure function of (shape, stream id, seed) evaluated with a
splitmix64 integer mixer in numpy uint64, so the golden-vector generator (which
runs the reference in the build container), the CPU oracle, the GPU parity
tests and bench.py all regenerate bit-identical fp32 tensors without any
committed weight file and without depending on torch's RNG.

Shapes follow the reference:
  parameters  /root/reference/models/controllable_captioning.py:23-68
  detections  (B, R0, D)        data/field.py:114-150  (zero rows = padding)
  ctrl slots  (B, L, R, D)      data/field.py:15-112   (zero rows = padding)
"""
from collections import OrderedDict

import numpy as np

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _mix(x):
    x = x.astype(np.uint64, copy=True)
    x ^= x >> np.uint64(30)
    x *= _M1
    x ^= x >> np.uint64(27)
    x *= _M2
    x ^= x >> np.uint64(31)
    return x


def hash_u01(n, stream, seed=0, offset=0):
    """n uniform float64 numbers in [0,1): splitmix64 of (offset+i), keyed by (stream, seed)."""
    with np.errstate(over="ignore"):
        key = _mix(np.array([np.uint64(stream) * _GOLD + np.uint64(seed) * _M1 + np.uint64(0x1234567)], dtype=np.uint64))[0]
        idx = np.arange(offset, offset + n, dtype=np.uint64)
        x = _mix(idx * _GOLD + key)
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def hash_int(n, lo, hi, stream, seed=0):
    """n integers in [lo, hi)."""
    u = hash_u01(n, stream, seed)
    return (lo + np.floor(u * (hi - lo))).astype(np.int64)


def param_shapes(vocab_size, det_feat_size=2048, input_encoding_size=1000, rnn_size=1000, att_size=512,
                 h2_first_lstm=True, img_second_lstm=False):
    """state_dict key -> shape, in the reference's registration order
    (controllable_captioning.py:23-68)."""
    V, D, E, H, A = vocab_size, det_feat_size, input_encoding_size, rnn_size, att_size
    in1 = D + E + (H if h2_first_lstm else 0)
    in2 = H + D + (D if img_second_lstm else 0)
    s = OrderedDict()
    s["embed.weight"] = (V, E)
    s["W1_is.weight"] = (H, in1); s["W1_is.bias"] = (H,)
    s["W1_hs.weight"] = (H, H); s["W1_hs.bias"] = (H,)
    s["att_va.weight"] = (A, D)
    s["att_ha.weight"] = (A, H)
    s["att_a.weight"] = (1, A)
    s["att_sa.weight"] = (A, H)
    s["att_s.weight"] = (1, A)
    s["lstm_cell_1.weight_ih"] = (4 * H, in1); s["lstm_cell_1.weight_hh"] = (4 * H, H)
    s["lstm_cell_1.bias_ih"] = (4 * H,); s["lstm_cell_1.bias_hh"] = (4 * H,)
    s["lstm_cell_2.weight_ih"] = (4 * H, in2); s["lstm_cell_2.weight_hh"] = (4 * H, H)
    s["lstm_cell_2.bias_ih"] = (4 * H,); s["lstm_cell_2.bias_hh"] = (4 * H,)
    s["out_fc.weight"] = (V, H); s["out_fc.bias"] = (V,)
    s["s_fc.weight"] = (D, H); s["s_fc.bias"] = (D,)
    s["W1_ig.weight"] = (H, in1); s["W1_ig.bias"] = (H,)
    s["W1_hg.weight"] = (H, H); s["W1_hg.bias"] = (H,)
    s["att_ga.weight"] = (A, H)
    s["att_g.weight"] = (1, A)
    return s


# Per-tensor gain over the xavier-uniform bound.  With gain 1 everywhere the reference emits <= 13
# distinct tokens and almost never shifts the slot pointer.  These gains put the
# decoder in a token-driven regime: a large embedding and input-to-hidden weights (pre-activations
# of O(1)), weak hidden-to-hidden recurrence (so fp32 rounding differences do NOT grow from step to
# step: measured max |logp_fp32 - logp_fp64| stays ~6e-6 over 20 steps, while hh gains >= 8 made it
# grow 1.5x per step), peaky attention and a shift gate that fires ~30 % of the time.
DEFAULT_GAINS = {
    "embed.weight": 40.0,
    "out_fc.weight": 10.0, "out_fc.bias": 1.0,
    "att_a.weight": 3.0, "att_s.weight": 3.0, "att_g.weight": 12.0,
    "att_va.weight": 2.0, "att_ha.weight": 2.0, "att_sa.weight": 2.0, "att_ga.weight": 2.0,
    "lstm_cell_1.weight_ih": 4.0, "lstm_cell_1.weight_hh": 1.0,
    "lstm_cell_2.weight_ih": 4.0, "lstm_cell_2.weight_hh": 1.0,
    "W1_is.weight": 3.0, "W1_hs.weight": 1.0, "W1_ig.weight": 3.0, "W1_hg.weight": 1.0,
    "s_fc.weight": 1.0,
}
BIAS_BOUND = 0.1


def make_weights(vocab_size, det_feat_size=2048, input_encoding_size=1000, rnn_size=1000, att_size=512,
                 h2_first_lstm=True, img_second_lstm=False, seed=0, gains=None):
    """OrderedDict name -> float32 ndarray (reference layout, row-major [out, in])."""
    g = dict(DEFAULT_GAINS)
    if gains:
        g.update(gains)
    shapes = param_shapes(vocab_size, det_feat_size, input_encoding_size, rnn_size, att_size,
                          h2_first_lstm, img_second_lstm)
    out = OrderedDict()
    for tid, (name, shp) in enumerate(shapes.items()):
        n = int(np.prod(shp))
        u = hash_u01(n, 100 + tid, seed)
        if len(shp) == 2:
            bound = np.sqrt(6.0 / (shp[0] + shp[1])) * g.get(name, 1.0)
        else:
            bound = BIAS_BOUND * g.get(name, 1.0)
        out[name] = ((2.0 * u - 1.0) * bound).astype(np.float32).reshape(shp)
    return out


FEATURE_DENSITY = 0.15
FEATURE_SCALE = 2.0


def _sparse_relu(u):
    """Sparse non-negative 'post-ReLU' features: ~15 % of the entries are non-zero, U(0, FEATURE_SCALE).
    Sparse features keep the common-mode part of W.x small against its variation, which the decoder
    needs to produce diverse tokens / slot shifts with random weights."""
    t = 1.0 - FEATURE_DENSITY
    return (np.maximum(0.0, u - t) * (FEATURE_SCALE / FEATURE_DENSITY)).astype(np.float32)


def make_detections(B, R0, D, seed=0, min_valid=None):
    """(B, R0, D) fp32 >= 0 'post-ReLU' features; rows >= n0[b] are exactly zero, n0 in [min_valid, R0]."""
    if min_valid is None:
        min_valid = max(1, (R0 * 10) // 36)
    u = hash_u01(B * R0 * D, 1, seed).reshape(B, R0, D)
    x = _sparse_relu(u)
    n0 = hash_int(B, min_valid, R0 + 1, 2, seed)
    x[np.arange(R0)[None, :] >= n0[:, None]] = 0.0
    return x


def make_ctrl(B, L, R, D, seed=0):
    """(B, L, R, D) fp32 >= 0; per (image, slot) the first n in [1, R] rows are non-zero."""
    u = hash_u01(B * L * R * D, 3, seed).reshape(B, L, R, D)
    x = _sparse_relu(u)
    n = hash_int(B * L, 1, R + 1, 4, seed).reshape(B, L)
    x[np.arange(R)[None, None, :] >= n[:, :, None]] = 0.0
    return x


def make_slot_indices(B, L, R, Rb, seed=0):
    """(B, L, R) int32 index lists into an (Rb)-row feature bank, -1 = padding: per (row, slot) the n in [1, min(R, Rb)]
    bank rows with the smallest hash keys, ascending (what np.unique gives field.py:52-55)."""
    key = hash_u01(B * L * Rb, 11, seed).reshape(B, L, Rb)
    n = hash_int(B * L, 1, min(R, Rb) + 1, 12, seed).reshape(B, L)
    order = np.argsort(key, axis=-1, kind="stable")          # a random permutation of the bank rows per slot
    idx = np.full((B, L, R), -1, dtype=np.int32)
    for b in range(B):
        for l in range(L):
            idx[b, l, :n[b, l]] = np.sort(order[b, l, :n[b, l]])
    return idx


def make_verbs(B, L, n_verbs, seed=0, p=0.15):
    """(B, L) float64 (as eval_coco.py:240 builds it): -1 = no verb, else a verb id in [0, n_verbs)."""
    u = hash_u01(B * L, 5, seed).reshape(B, L)
    ids = hash_int(B * L, 0, n_verbs, 6, seed).reshape(B, L)
    v = np.where(u < p, ids, -1).astype(np.float64)
    return v


def make_captions(B, T, V, seed=0):
    return hash_int(B * T, 0, V, 7, seed).reshape(B, T)


def make_gate_gts(B, T, seed=0):
    """(B, T) in {0,1} with a trailing run of -1 padding (train.py:109 uses ignore_index=-1)."""
    g = hash_int(B * T, 0, 2, 8, seed).reshape(B, T)
    n = hash_int(B, max(1, T // 2), T + 1, 9, seed)
    g[np.arange(T)[None, :] >= n[:, None]] = -1
    return g


def make_verb_table(n_verbs, V, seed=0):
    """dict str(verb id) -> list of vocab ids, like datasets/coco/verb_2_vob_all_refine.json.
    Verb 0 has no entry, verb 1 an empty list, verb 2 one id, the rest 2..6 ids."""
    table = {}
    for v in range(n_verbs):
        if v == 0:
            continue
        if v == 1:
            table[str(v)] = []
            continue
        k = 1 if v == 2 else int(hash_int(1, 2, 7, 10 + v, seed)[0])
        table[str(v)] = [int(i) for i in hash_int(k, 1, V, 1000 + v, seed)]
    return table


# ---------------------------------------------------------------------------------------------- ordering models
def ssp_param_shapes(n_verbs=2663):
    """state_dict keys / shapes of the reference's S_SSP (models/sort_model.py:13-52) in its own order, without the
    positional-encoding / label-smoothing buffers."""
    H, F_ = 512, 2048
    sh = OrderedDict()
    sh["sr_embed_layer.weight"] = (26, H)
    sh["v_embed_layer.weight"] = (n_verbs, H)

    def layer(pre, dec):
        names = ["attention"] + (["cross_attention"] if dec else [])
        for a in names:
            for q in "QKVO":
                sh["%s.%s.linear_%s.weight" % (pre, a, q)] = (H, H)
                sh["%s.%s.linear_%s.bias" % (pre, a, q)] = (H,)
        sh[pre + ".ff_layer.w_1.weight"] = (F_, H); sh[pre + ".ff_layer.w_1.bias"] = (F_,)
        sh[pre + ".ff_layer.w_2.weight"] = (H, F_); sh[pre + ".ff_layer.w_2.bias"] = (H,)
        for i in range(1, 4 if dec else 3):
            sh["%s.layer_norm%d.weight" % (pre, i)] = (H,)
            sh["%s.layer_norm%d.bias" % (pre, i)] = (H,)
    sh["encoder.layer_norm.weight"] = (H,); sh["encoder.layer_norm.bias"] = (H,)
    for l in range(3):
        layer("encoder.encoder_layers.%d" % l, False)
    sh["encoder.fc_feat.weight"] = (H, H); sh["encoder.fc_feat.bias"] = (H,)
    sh["decoder.layer_norm.weight"] = (H,); sh["decoder.layer_norm.bias"] = (H,)
    for l in range(3):
        layer("decoder.encoder_layers.%d" % l, True)
    sh["expander_nn.weight"] = (26, H); sh["expander_nn.bias"] = (26,)
    return sh


def sinkhorn_param_shapes(N=10):
    """SinkhornNet (models/sinkhorn_network.py:5-16)"""
    return OrderedDict([("W1_txt.weight", (128, 300)), ("W1_txt.bias", (128,)), ("W1_vis.weight", (512, 2048)), ("W1_vis.bias", (512,)),
                        ("W2_vis.weight", (128, 512)), ("W2_vis.bias", (128,)), ("W_fc_pos.weight", (256, 260)), ("W_fc_pos.bias", (256,)),
                        ("W_fc.weight", (N, 256)), ("W_fc.bias", (N,))])


def _fill(shapes, seed, stream0, gain):
    w = OrderedDict()
    for i, (k, shp) in enumerate(shapes.items()):
        n = int(np.prod(shp))
        u = hash_u01(n, stream0 + i, seed).reshape(shp)
        if k.endswith("weight") and len(shp) == 2:
            fan = shp[0] + shp[1]
            if "embed" in k:
                w[k] = ((u - 0.5) * 2 * 0.08).astype(np.float32)
            else:
                w[k] = ((u - 0.5) * 2 * gain * np.sqrt(6.0 / fan)).astype(np.float32)
        elif "layer_norm" in k and k.endswith("weight"):
            w[k] = (1.0 + 0.2 * (u - 0.5)).astype(np.float32)
        else:
            w[k] = (0.1 * (u - 0.5)).astype(np.float32)
    return w


def make_ssp_weights(seed=0, n_verbs=2663, gain=1.6):
    return _fill(ssp_param_shapes(n_verbs), seed, 500, gain)


def make_sinkhorn_weights(seed=0, N=10, gain=1.5):
    return _fill(sinkhorn_param_shapes(N), seed, 800, gain)


def make_ssp_inputs(S, seed=0, n_verbs=2663):
    """verbs (S,) in [1, n_verbs), roles (S,10): n in [1,10] DISTINCT role ids in 1..25, zero padded (eval_coco.py:150-166)"""
    verbs = hash_int(S, 1, n_verbs, 900, seed).astype(np.int64)
    n = hash_int(S, 1, 11, 901, seed)
    roles = np.zeros((S, 10), dtype=np.int64)
    for s in range(S):
        order = np.argsort(hash_u01(25, 902 + s, seed))
        roles[s, :n[s]] = order[:n[s]] + 1
    return verbs, roles


def make_sinkhorn_inputs(Q, seed=0, N=10):
    """(Q, N, 2352) region rows [300 + 2048 + 4]: the first n rows are filled (n in [2, N]), the rest is zero (eval_coco.py:178-182)"""
    n = hash_int(Q, 2, N + 1, 910, seed)
    x = np.zeros((Q, N, 2352), dtype=np.float32)
    u = hash_u01(Q * N * 2352, 911, seed).reshape(Q, N, 2352)
    x[:, :, :300] = (u[:, :, :300] - 0.5) * 2
    x[:, :, 300:2348] = _sparse_relu(u[:, :, 300:2348])
    x[:, :, 2348:] = u[:, :, 2348:]
    for q in range(Q):
        x[q, n[q]:] = 0
    return x, n


def make_rank_batch(N, MV, seed, L=10):
    """A loader batch for the eval loop's caption ranking: (control_verb (N, MV), det_seqs_v (N, L, MV), det_seqs_sr (N, L, MV) int64,
    feats (N, L, 2352) fp32).  Every caption has 1..MV verbs, 3..L filled slots that each serve some of its verbs once, and role ids in
    [1, 7) - few distinct roles, so repeated roles (Sinkhorn items) are common.  The generator of tests/test_gpu_ssp.py's rank_captions test."""
    rng = np.random.RandomState(seed)
    control_verb = np.zeros((N, MV), dtype=np.int64)
    det_seqs_v = np.zeros((N, L, MV), dtype=np.int64)
    det_seqs_sr = np.zeros((N, L, MV), dtype=np.int64)
    for n in range(N):
        nv = rng.randint(1, MV + 1)
        control_verb[n, :nv] = rng.choice(np.arange(1, 2600), nv, replace=False)
        for j in range(rng.randint(3, L + 1)):
            vs = rng.permutation(control_verb[n, :nv])[:rng.randint(1, nv + 1)]     # a slot serves each verb at most once
            for k, v in enumerate(vs):
                det_seqs_v[n, j, k] = v
                det_seqs_sr[n, j, k] = rng.randint(1, 7)
    feats, _ = make_sinkhorn_inputs(N, 7)
    feats[:] = np.abs(hash_u01(feats.size, 77, 7).reshape(feats.shape).astype(np.float32))
    return control_verb, det_seqs_v, det_seqs_sr, feats
