"""How far a kernel's result may lie from the reference: no further than K times what a plain transform of the same precision does.

The contract bounds (1e-5, 1e-4, 1e-12, 1e-10 normwise) leave a float32 kernel a factor of 20 ... 60 and a float64 one several thousand
above its real accuracy.  Here a case's result and the yardstick's (tests/plain.py at the kernel's own precision, on the same input and
constants) are measured against the same reference with the same four metrics, and the kernel passes when each of its four is at most
K times the yardstick's.  With d = out - ref, every clip of the case taken together:

  e_max   max|d| / max|ref|                       the project's normwise metric
  e_rms   ||d||_2 / ||ref||_2
  e_row   max over rows of rms_row(d) / rms_row(ref)      a row: a bin, band, coefficient or CQT bin of all clips' frames; for a 1-D
          output the positions n mod hop.  One wrong table entry shows here.
  e_col   the same over frames (each clip's own); for a 1-D output over hop-long blocks.  A frame slot of a tile or a segment edge.

K is not tuned on the kernels:

  K_RMS = 2   the shipped FFT core, emulated on the host, sits at 0.99 ... 1.07 of the yardstick in rms, a statistic over >= 3e4
              elements that does not fluctuate; the factor 2 is for what surrounds the core (real-split and fold passes, two-level root
              products, packed FMAs), each adding rounding of the size the transform already has;
  K_MAX = 3   for e_max, e_row and e_col: each a maximum over at most a few thousand rms estimates of 20 ... 66 samples, of which
              kernel and yardstick draw theirs independently;
  BLUESTEIN   twice both: those routes run three transforms of >= 2 W points and two chirp products where the yardstick runs one
              mixed-radix transform of W points.

A case above its factor is a finding.  A per-case factor (never above MAX_FACTOR) needs a cause, written next to it."""
import numpy as np

K_RMS, K_MAX = 2.0, 3.0
BLUESTEIN = 2.0
MAX_FACTOR = 8.0
METRICS = ("e_max", "e_rms", "e_row", "e_col")


def factors(bluestein=False, own=None):
    """metric -> K.  own: a per-case factor that replaces both (its cause stands in the case table)."""
    if own is not None:
        assert K_MAX < own <= MAX_FACTOR
        return dict.fromkeys(METRICS, float(own))
    m = BLUESTEIN if bluestein else 1.0
    return {"e_max": K_MAX * m, "e_rms": K_RMS * m, "e_row": K_MAX * m, "e_col": K_MAX * m}


def _sq(a):
    a = np.asarray(a)
    return (a.real.astype(np.longdouble) ** 2 + a.imag.astype(np.longdouble) ** 2) if np.iscomplexobj(a) else a.astype(np.longdouble) ** 2


def _worst(num, den):
    """max of sqrt(num / den) over the groups that have a reference level; inf where a group without one carries an error."""
    num, den = np.asarray(num, np.longdouble).reshape(-1), np.asarray(den, np.longdouble).reshape(-1)
    if np.any((den == 0) & (num > 0)):
        return float("inf")
    live = den > 0
    return float(np.sqrt((num[live] / den[live]).max())) if live.any() else 0.0


def _blocks(sq, hop):
    """Sums over hop-long blocks of a 1-D array of squares (the last block takes the remainder) and over the positions n mod hop."""
    n = len(sq)
    count = max(n // hop, 1)
    edges = np.arange(count) * hop
    col = np.add.reduceat(sq, edges) if n else np.zeros(0, np.longdouble)
    row = np.zeros(hop, np.longdouble)
    for r in range(min(hop, n)):
        row[r] = sq[r::hop].sum()
    return row, col


def measure(outs, refs, hop=None):
    """outs, refs: per clip a (rows, frames) array, or a 1-D signal (then hop is its block length).  -> {metric: value}."""
    assert len(outs) == len(refs) and len(refs)
    d2, r2 = [], []
    wide = np.complex256 if any(np.iscomplexobj(r) for r in refs) else np.longdouble
    for o, r in zip(outs, refs):
        o, r = np.asarray(o), np.asarray(r)
        assert o.shape == r.shape and r.ndim in (1, 2), (o.shape, r.shape)
        d2.append(_sq(o.astype(wide) - r.astype(wide)))
        r2.append(_sq(r))
    total_d, total_r = sum(float(a.sum()) for a in d2), sum(float(a.sum()) for a in r2)
    peak_r = max(float(a.max()) for a in r2 if a.size)
    res = {"e_max": float(np.sqrt(max(float(a.max()) for a in d2 if a.size) / peak_r)) if peak_r else 0.0,
           "e_rms": float(np.sqrt(total_d / total_r)) if total_r else 0.0}
    if refs[0].ndim == 2:
        row_d, row_r = sum(a.sum(axis=1) for a in d2), sum(a.sum(axis=1) for a in r2)
        col_d, col_r = np.concatenate([a.sum(axis=0) for a in d2]), np.concatenate([a.sum(axis=0) for a in r2])
    else:
        assert hop, "a 1-D result needs its hop"
        parts_d, parts_r = [_blocks(a, hop) for a in d2], [_blocks(a, hop) for a in r2]
        row_d, row_r = sum(p[0] for p in parts_d), sum(p[0] for p in parts_r)
        col_d, col_r = np.concatenate([p[1] for p in parts_d]), np.concatenate([p[1] for p in parts_r])
    res["e_row"], res["e_col"] = _worst(row_d, row_r), _worst(col_d, col_r)
    return res


def ratios(kernel, yard):
    return {m: (kernel[m] / yard[m] if yard[m] > 0 else (0.0 if kernel[m] == 0 else float("inf"))) for m in METRICS}


def over(kernel, yard, k):
    """The metrics at which the kernel exceeds k[metric] times the yardstick."""
    return [m for m in METRICS if not kernel[m] <= k[m] * yard[m]]


def line(name, kernel_name, kernel, yard):
    """One line per case: kernel, the eight numbers and the four ratios."""
    r = ratios(kernel, yard)
    return (f"{name} {kernel_name} | kernel " + " ".join(f"{m}={kernel[m]:.3g}" for m in METRICS) + " | yardstick "
            + " ".join(f"{m}={yard[m]:.3g}" for m in METRICS) + " | ratio " + " ".join(f"{m}={r[m]:.2f}" for m in METRICS))


def record(kernel_name, kernel, yard, k):
    return {"kernel": kernel_name, "kernel_metrics": {m: float(f"{kernel[m]:.4g}") for m in METRICS},
            "yardstick_metrics": {m: float(f"{yard[m]:.4g}") for m in METRICS},
            "ratios": {m: round(v, 3) for m, v in ratios(kernel, yard).items()}, "factors": k}
