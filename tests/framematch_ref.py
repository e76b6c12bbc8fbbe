"""NumPy restatement of the frame-matching contract (include/v3d_hip.h, "Frame matching"): signatures through an integral image,
scores in int64, the host's correlation and the decision rule of video_3d_pipeline/framematch.py.  Test infrastructure: written
from the contract, not from the product code, and the product never imports it.

  signature   cell (cy, cx) of a W x H plane = rows [cy*H//36, (cy+1)*H//36) x columns [cx*W//64, (cx+1)*W//64);
              sig[cy*64 + cx] = (256 * S) // c, S the sum of the cell's bytes, c its pixel count
  scores      G = 2304; num[i][j] = G * sum(a_i*b_j) - sum(a_i)*sum(b_j); var[i] = G * sum(a_i^2) - (sum a_i)^2  (int64)
  zncc        Z = num / sqrt(float64(var_a) * float64(var_b)); NaN where either variance is 0 (uninformative)
  decide      see decide() below
"""
import numpy as np

GW, GH, G = 64, 36, 2304


def signature(gray):
    """u8 [H,W] or [n,H,W] -> uint16 [2304] or [n,2304]"""
    g = np.asarray(gray)
    if g.ndim == 3:
        return np.stack([signature(f) for f in g])
    H, W = g.shape
    assert g.dtype == np.uint8 and 64 <= W <= 8192 and 36 <= H <= 8192
    I = np.zeros((H + 1, W + 1), np.int64)
    I[1:, 1:] = g.astype(np.int64).cumsum(0).cumsum(1)
    ys = np.arange(GH + 1) * H // GH
    xs = np.arange(GW + 1) * W // GW
    S = I[ys[1:, None], xs[None, 1:]] - I[ys[:-1, None], xs[None, 1:]] - I[ys[1:, None], xs[None, :-1]] + I[ys[:-1, None], xs[None, :-1]]
    c = (ys[1:] - ys[:-1])[:, None] * (xs[1:] - xs[:-1])[None, :]
    return ((256 * S) // c).astype(np.uint16).reshape(G)


def scores(sig_a, sig_b):
    """uint16 [na,2304], [nb,2304] -> (num int64 [na,nb], var_a int64 [na], var_b int64 [nb])"""
    a = np.asarray(sig_a).astype(np.int64).reshape(-1, G)
    b = np.asarray(sig_b).astype(np.int64).reshape(-1, G)
    sa, sb = a.sum(1), b.sum(1)
    num = G * (a @ b.T) - sa[:, None] * sb[None, :]
    return num, G * (a * a).sum(1) - sa * sa, G * (b * b).sum(1) - sb * sb


def zncc(num, var_a, var_b):
    """-> float64 [na,nb], NaN for the uninformative pairs"""
    va = np.asarray(var_a).astype(np.float64)[:, None]
    vb = np.asarray(var_b).astype(np.float64)[None, :]
    den = np.sqrt(va * vb)
    Z = np.full(den.shape, np.nan)
    ok = den > 0
    Z[ok] = np.asarray(num).astype(np.float64)[ok] / den[ok]
    return Z


def _argmax(values, search):
    """index into d = -search .. search of the largest defined value; ties to the smaller |d|, then to the negative d"""
    order = sorted(range(2 * search + 1), key=lambda k: (abs(k - search), k - search))
    best = None
    for k in order:
        if not np.isnan(values[k]) and (best is None or values[k] > values[best]):
            best = k
    return best


def decide(probes, search, min_score, min_margin):
    """probes: [(Z [w,nb], col0)]: window row a and shift d meet at column col0 + a + d of Z (a pair whose column lies outside
    [0, nb) has no 4K frame).  Per probe m_p(d) = mean of the informative in-range pairs, defined iff they are at least half of
    the window; the probe's shift = argmax_d m_p; M(d) = mean of the defined m_p(d); d* = argmax_d M; margin = M(d*) - second
    best.  refined iff M(d*) >= min_score, margin >= min_margin and every probe with a shift agrees with d*; else inconsistent
    iff a probe disagrees, else undetermined."""
    nd = 2 * search + 1
    m = np.full((len(probes), nd), np.nan)
    for p, (Z, col0) in enumerate(probes):
        w, nb = Z.shape
        for k in range(nd):
            vals = []
            for a in range(w):
                col = col0 + a + k - search
                if 0 <= col < nb and not np.isnan(Z[a, col]):
                    vals.append(Z[a, col])
            if vals and 2 * len(vals) >= w:
                m[p, k] = float(np.mean(vals))
    shifts, pscores = [], []
    for p in range(len(probes)):
        k = _argmax(m[p], search)
        shifts.append(None if k is None else k - search)
        pscores.append(None if k is None else float(m[p, k]))
    M = np.full(nd, np.nan)
    for k in range(nd):
        col = m[:, k][~np.isnan(m[:, k])] if len(probes) else np.zeros(0)
        if col.size:
            M[k] = float(np.mean(col))
    kb = _argmax(M, search)
    out = dict(M=M, probe_shifts=shifts, probe_scores=pscores)
    if kb is None:
        out.update(status="undetermined", best_shift=0, shift=0, score=None, margin=None)
        return out
    rest = [M[k] for k in range(nd) if k != kb and not np.isnan(M[k])]
    margin = float(M[kb] - max(rest)) if rest else 0.0
    d = kb - search
    agree = all(s == d for s in shifts if s is not None)
    if M[kb] >= min_score and margin >= min_margin and agree:
        status = "refined"
    else:
        status = "undetermined" if agree else "inconsistent"
    out.update(status=status, best_shift=d, shift=d if status == "refined" else 0, score=float(M[kb]), margin=margin)
    return out


def probe_starts(count, window, probes):
    """first SBS frame (relative to the start frame) of each probe window: `probes` windows of `window` frames spread evenly over
    `count` frames; fewer, or a shorter window, when the clip is short"""
    w = min(window, count)
    if probes <= 1 or count - w <= 0:
        return [0], w
    return sorted({(count - w) * p // (probes - 1) for p in range(probes)}), w


def refine_ref(left, guide, g0, search, window, probes, min_score, min_margin):
    """the whole refinement on two luma clips held in memory: left u8 [n,H,W] (the SBS side), guide u8 [m,Hg,Wg]"""
    starts, w = probe_starts(len(left), window, probes)
    plist, ints = [], []
    for s in starts:
        lo, hi = max(0, g0 + s - search), min(len(guide), g0 + s + w + search)
        if hi <= lo:
            continue
        num, va, vb = scores(signature(left[s:s + w]), signature(guide[lo:hi]))
        ints.append((num, va, vb))
        plist.append((zncc(num, va, vb), g0 + s - lo))
    out = decide(plist, search, min_score, min_margin)
    out["ints"] = ints
    return out


def match_clips(W, H, n_sbs, speed=6, delay=3, extra=4, seed=5):
    """the recovery clips: a synthetic.temporal_clip left view of n_sbs + delay + extra frames is the content; the SBS side shows
    content frames delay .. delay + n_sbs - 1, the guide shows every content frame zoomed x2 (pixel repetition) with gain 0.8,
    offset +30 and N(0, 2) noise.  So SBS frame i matches guide frame i + delay -> (left u8 [n_sbs,H,W], guide u8 [m,2H,2W])"""
    from video_3d_pipeline import synthetic as syn
    content = syn.temporal_clip(W, H, n_sbs + delay + extra, speed=speed)[0]
    rng = np.random.default_rng(seed)
    big = np.repeat(np.repeat(content, 2, axis=1), 2, axis=2).astype(np.float64)
    guide = np.clip(np.rint(0.8 * big + 30.0 + rng.normal(0.0, 2.0, big.shape)), 0, 255).astype(np.uint8)
    return content[delay:delay + n_sbs], guide


def match_sbs_clips(W, H, n_sbs, delay=3, extra=4, seed=5, speed=6):
    """match_clips as the two containers of the CLIs: (SBS BGR [n_sbs,H,W,3] with each eye squeezed to W/2, guide BGR
    [n_sbs + delay + extra, 2H, 2W, 3]); SBS frame i matches guide frame i + delay"""
    from video_3d_pipeline import synthetic as syn
    _, guide = match_clips(W, H, n_sbs, speed=speed, delay=delay, extra=extra, seed=seed)
    sbs = syn.temporal_sbs_clip(W, H, n_sbs + delay + extra, speed=speed)[delay:delay + n_sbs]
    return sbs, np.ascontiguousarray(np.repeat(guide[..., None], 3, axis=3))
