"""Gradients against the fp64 oracle, element by element and slice by slice, with the fp32 oracle's own error as the yardstick.

oracle_grads() runs one loss (XE, or SCST on replayed samples) through vo.Oracle in a given dtype and returns everything as fp64.
The fp64 run is the reference.  The fp32 run is the yardstick: what one honest fp32 evaluation of the same graph loses.

compare() holds each of the 28 gradients to two metrics:
  (a) max |got - ref| / max |ref|                                          - one wrong element of the tensor's own size
  (b) max over slices s of ||got_s - ref_s||_2 / (||ref_s||_2 + floor)     - one wrong row, column or tile that (a) hides under
      the tensor's largest element.  The slices are those along dim 0 and, for 2-D tensors, those along dim 1 as well (a slice of
      a 1-D tensor is one element).  floor = FLOOR_SHARE x the median norm of the slices whose reference is not exactly zero, so
      that a slice of near-zero gradient is measured against a typical slice instead of against itself; a slice whose reference
      IS zero (an embedding row no caption reads) is held to that floor too, so anything written into it counts.
The bound of a metric on a tensor is margin x the same metric of the fp32 oracle on that tensor, computed from the same inputs; no
absolute constant but ULP_FLOOR, a few fp32 ulps of the tensor's scale, for a tensor whose yardstick happens to be 0.

MARGIN = 16 = 4 x 4:
  4  the device and the CPU oracle are two fp32 summation orders (slabs, k pieces, row-ordered sums).  Each differs from fp64 by an
     independent sample of the same rounding noise, and over ~1e6 elements the max of one sample can be a few times another's.
  4  the device's tanhf / expf / sigmoid are a few ulp where the CPU's are at most 1 ulp.
Neither grows with the problem size.  The bound never looks at the code under test.

The project's older ceiling (tests/test_gpu_train.py::_check: 2e-3 of max |ref|, 3e-3 for SCST) stays as a second, unconditional
assert of compare(), so nothing that failed before passes now."""
import vsr_oracle as vo

MARGIN = 16.0
FLOOR_SHARE = 0.25                   # metric (b): share of the median slice norm added to every slice's norm
ULP_FLOOR = 4.0 * 2.0 ** -23         # lowest bound of either metric: 4 fp32 ulps of the tensor's (slice's) scale
FACTOR_CAP = 1e-4                    # no per-tensor factor may lift a bound past this share of max |ref|


def xe_loss_fn(caps, gts):
    return lambda lw, lg: vo.xe_loss(lw, lg, caps, gts)[0]


def scst_loss_fn(reward, base):
    return lambda lw, lg: vo.scst_loss(lw, lg, reward.to(lw.dtype), base.to(lw.dtype))


def oracle_grads(w, T, det, dtype, loss_fn, caps=None, ctrl_seq=None, ctrl=None, forced=None, **flags):
    """One forward + backward of the CPU oracle in `dtype`.
    XE:   caps (B, T) and ctrl_seq (B, T, R, D): teacher-forced forward, loss_fn = xe_loss_fn(caps, gts).
    SCST: ctrl (B, L, R, D) and forced = (words, gates): replayed sample_rl, loss_fn = scst_loss_fn(reward, baseline).
    Returns dict(loss=float, logp_words, logp_gates, grads={name: tensor}), every tensor fp64."""
    assert (caps is None) != (forced is None)
    o = vo.Oracle(w, T, 2, as_written=True, dtype=dtype, **flags)
    for k in o.p:
        o.p[k].requires_grad_(True)
    if caps is not None:
        lw, lg = o.forward(det.to(dtype), caps, ctrl_seq.to(dtype))
    else:
        _, (lw, lg) = o.sample_rl(det.to(dtype), ctrl.to(dtype), forced=forced)
    loss = loss_fn(lw, lg)
    loss.backward()
    return dict(loss=float(loss.item()), logp_words=lw.detach().double(), logp_gates=lg.detach().double(),
                grads={k: o.p[k].grad.detach().double() for k in o.p})


def _slice_metric(err, ref, dim):
    """max over the slices along `dim` of ||err_s|| / (||ref_s|| + floor)"""
    other = [d for d in range(ref.dim()) if d != dim]
    en = err.pow(2).sum(other).sqrt() if other else err.abs()
    rn = ref.pow(2).sum(other).sqrt() if other else ref.abs()
    live = rn[rn > 0]
    if live.numel() == 0:
        return 0.0 if float(en.max()) == 0.0 else float("inf")
    floor = FLOOR_SHARE * float(live.median())
    return float((en / (rn + floor)).max())


def metrics(got, ref):
    """(a, b) of one tensor against its fp64 reference"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = got - ref
    scale = float(ref.abs().max())
    a = float(err.abs().max()) / scale if scale > 0 else (0.0 if float(err.abs().max()) == 0.0 else float("inf"))
    b = max(_slice_metric(err, ref, d) for d in range(min(ref.dim(), 2)))
    return a, b


def over_ceiling(got, ref, ceiling):
    """the project's older check alone (tests/test_gpu_train.py::_check): names of the tensors that miss it"""
    bad = []
    for k in ref:
        g, r = got[k].double(), ref[k].double()
        if (g - r).abs().max().item() > ceiling * (r.abs().max().item() + 1e-12) + 1e-9:
            bad.append(k)
    return bad


def compare(got, ref64, yard32, margin=MARGIN, ceiling=2e-3, factors=None, label=""):
    """Every tensor of `got` against ref64 under both metrics; the bound is margin x the metric of yard32 (x factors[name], if the
    caller names a cause for one).  Prints the worst ratio = error / yardstick per metric and returns them as
    {"a": (ratio, name), "b": (ratio, name)}.  Raises AssertionError naming every miss."""
    factors = factors or {}
    assert set(got) == set(ref64) == set(yard32), "not the same 28 tensors"
    worst = {"a": (0.0, ""), "b": (0.0, "")}
    missed = []
    for k in ref64:
        ma, mb = metrics(got[k], ref64[k])
        ya, yb = metrics(yard32[k], ref64[k])
        f = float(factors.get(k, 1.0))
        for tag, m, y in (("a", ma, ya), ("b", mb, yb)):
            unit = max(y, ULP_FLOOR / margin)                       # the yardstick, lifted to the ulp floor where it is ~0
            bound = margin * unit * f
            if f != 1.0:
                bound = min(bound, max(FACTOR_CAP, margin * unit))  # a factor never lifts a bound past FACTOR_CAP
            ratio = m / unit
            if ratio > worst[tag][0]:
                worst[tag] = (ratio, k)
            if not m <= bound:
                missed.append("%s (%s): %.3e > %.3e = %g x yardstick %.3e%s  [ratio %.1f]"
                              % (k, tag, m, bound, margin, unit, " x factor %g" % f if f != 1.0 else "", ratio))
    print("%s worst error / fp32-oracle error: (a) %.2f %s   (b) %.2f %s"
          % (label, worst["a"][0], worst["a"][1], worst["b"][0], worst["b"][1]))
    over = over_ceiling(got, ref64, ceiling)
    assert not over, "%s over the %g-of-max ceiling: %s" % (label, ceiling, ", ".join(over))
    assert not missed, "%s beyond %g x the fp32 oracle's own error:\n  " % (label, margin) + "\n  ".join(missed)
    return worst


def check_outputs(loss, logp_words, logp_gates, ref64, label=""):
    """loss within 1e-4 and log-probs within 2e-4 of the fp64 oracle (the bounds the suite held against the fp32 oracle)"""
    dl = abs(loss - ref64["loss"])
    dw = float((logp_words.detach().double().cpu() - ref64["logp_words"]).abs().max())
    dg = float((logp_gates.detach().double().cpu() - ref64["logp_gates"]).abs().max())
    print("%s |dloss| %.2e  max |dlogp_words| %.2e  max |dlogp_gates| %.2e" % (label, dl, dw, dg))
    assert dl < 1e-4, "%s loss %.7f vs fp64 %.7f" % (label, loss, ref64["loss"])
    assert dw <= 2e-4 and dg <= 2e-4, "%s log-probs off by %.3e (words) / %.3e (gates)" % (label, dw, dg)
