"""Bit-exact contract of the spatial registration entries (v3d_register.hip; include/v3d_hip.h "Spatial registration") in plain
integer NumPy: the row and column sums of a luma plane, the 1-D affine match of two profiles and the u16 warp.  Shares no code
with the kernels.  Every `>>` and `//` below is NumPy's / Python's: the mathematical floor, for negative numbers too.

Rounding of every conversion to Q16 the host does (video_3d_pipeline/register.py restates these lines and
tests/test_register_host.py holds it to them): round half up, floor(x + 1/2), evaluated in exact rationals
(fractions.Fraction of the floats, which is exact), so a map read back from alignment_data.json gives the same integers on
every machine:

  map_to_q16(A, B, Ws, Wo)    output pixel xo sits at xi = (xo + 1/2) / Wo, its source index is (A xi + B) Ws - 1/2, so
                              ax = rhu(65536 A Ws / Wo),   bx = rhu(65536 ((A / (2 Wo) + B) Ws - 1/2));
  candidate(p0, p1, nb)       the search's candidates are pairs of source positions in Q16 (integers already): the source position p0
                              of the target's first edge and p1 of its last one; a = rhu((p1 - p0) / nb), b = p0;
  normalised(a, b, na, nb)    the way back, exact: A = a nb / (65536 na), B = b / (65536 na), as the nearest float64.
"""
from fractions import Fraction

import numpy as np

Q = 65536
A_MIN, A_MAX, B_MAX = 1 << 12, 1 << 20, 1 << 29            # candidate domain of the match
WARP_B_MAX = 1 << 40
FIELDS = 6


def rhu(x) -> int:
    """round half up of a rational"""
    return int((Fraction(x) + Fraction(1, 2)).__floor__())


# ---- 1. profiles ----
def profiles(gray):
    """gray u8 [n,H,W] -> (col u32 [n,W], row u32 [n,H])"""
    g = np.asarray(gray, dtype=np.uint8).astype(np.int64)
    return g.sum(axis=1).astype(np.uint32), g.sum(axis=2).astype(np.uint32)


# ---- 2. match ----
def edges(nb: int, bins: int):
    """t_j = floor(j nb 65536 / bins), j = 0 .. bins (int64)"""
    return (np.arange(bins + 1, dtype=np.int64) * nb * Q) // bins


def integral(P, p):
    """I(p) of profile P (length n) at the Q16 positions p in [0, n 65536] (int64 array)"""
    P = np.asarray(P).astype(np.int64)
    pre = np.concatenate([[0], np.cumsum(P)])
    Pz = np.concatenate([P, [0]])
    p = np.asarray(p, dtype=np.int64)
    i, f = p >> 16, p & 65535
    return pre[i] * Q + f * Pz[i]


def bin_means(P, e):
    """floor mean of P over [e_j, e_j+1) for the edge rows e [..., m+1] -> (means [..., m] int64, valid [..., m] bool); invalid
    bins (an edge outside [0, n 65536]) give 0"""
    n = len(P)
    e = np.asarray(e, dtype=np.int64)
    lo, hi = e[..., :-1], e[..., 1:]
    ok = (lo >= 0) & (hi <= n * Q)
    lo_c, hi_c = np.where(ok, lo, 0), np.where(ok, hi, Q)
    m = (integral(P, hi_c) - integral(P, lo_c)) // (hi_c - lo_c)
    return np.where(ok, m, 0), ok


def check_candidates(cand):
    c = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    bad = (c[:, 0] < A_MIN) | (c[:, 0] > A_MAX) | (np.abs(c[:, 1]) > B_MAX)
    if bad.any():
        raise ValueError(f"candidate {c[np.flatnonzero(bad)[0]].tolist()} outside 2^12 <= a <= 2^20, |b| <= 2^29")
    return c


def match_scores(prof_a, prof_b, cand, bins: int):
    """prof_a u32 [K,na], prof_b u32 [K,nb], cand int64 [C,2] -> int64 [K,C,6]:
    (n_pairs, sum da, sum db, sum da db, sum da^2, sum db^2) over the valid difference pairs"""
    pa, pb = np.atleast_2d(np.asarray(prof_a)), np.atleast_2d(np.asarray(prof_b))
    K, nb = pb.shape
    if not (8 <= bins <= 1024 and nb >= bins and pa.shape[0] == K):
        raise ValueError("bins outside [8, 1024], nb < bins or unequal frame counts")
    c = check_candidates(cand)
    t = edges(nb, bins)
    s = ((c[:, :1] * t[None, :]) >> 16) + c[:, 1:]                         # [C, bins+1]
    out = np.zeros((K, len(c), FIELDS), dtype=np.int64)
    for k in range(K):
        mb, _ = bin_means(pb[k], t)
        ma, ok = bin_means(pa[k], s)
        pair = ok[:, :-1] & ok[:, 1:]
        da = np.where(pair, ma[:, 1:] - ma[:, :-1], 0)
        db = np.where(pair, (mb[1:] - mb[:-1])[None, :], 0)
        out[k] = np.stack([pair.sum(1), da.sum(1), db.sum(1), (da * db).sum(1), (da * da).sum(1), (db * db).sum(1)], axis=1)
    return out


def match_scores_wrapping(prof_a, prof_b, cand, bins: int):
    """match_scores for profile samples of any u32 value: the header's formula as a literal loop in Python integers, each of the
    six sums reduced mod 2^64 and read as int64 (the record "wraps").  Below the headroom (samples < 2^21) nothing wraps and it
    equals match_scores; it shares none of its code"""
    pa, pb = np.atleast_2d(np.asarray(prof_a)), np.atleast_2d(np.asarray(prof_b))
    (K, na), nb = pa.shape, pb.shape[1]
    if not (8 <= bins <= 1024 and nb >= bins and pb.shape[0] == K):
        raise ValueError("bins outside [8, 1024], nb < bins or unequal frame counts")
    c = check_candidates(cand)
    t = [(j * nb * Q) // bins for j in range(bins + 1)]
    out = np.zeros((K, len(c), FIELDS), dtype=np.int64)

    def means(P, e):
        """floor means of the list P over [e_j, e_j+1), None where a bin leaves [0, len(P) 65536]"""
        pre = [0]
        for v in P:
            pre.append(pre[-1] + v)
        Pz = P + [0]
        I = [pre[p >> 16] * Q + (p & 65535) * Pz[p >> 16] if 0 <= p <= len(P) * Q else None for p in e]
        return [None if I[j] is None or I[j + 1] is None else (I[j + 1] - I[j]) // (e[j + 1] - e[j]) for j in range(len(e) - 1)]
    for k in range(K):
        A, B = [int(v) for v in pa[k]], [int(v) for v in pb[k]]
        mb = means(B, t)
        for ci, (a, b) in enumerate(c.tolist()):
            ma = means(A, [((a * tj) >> 16) + b for tj in t])
            rec = [0] * FIELDS
            for j in range(bins - 1):
                if ma[j] is None or ma[j + 1] is None:
                    continue
                da, db = ma[j + 1] - ma[j], mb[j + 1] - mb[j]
                rec = [r + v for r, v in zip(rec, (1, da, db, da * db, da * da, db * db))]
            out[k, ci] = [((r + (1 << 63)) % (1 << 64)) - (1 << 63) for r in rec]
    return out


def zncc(rec, bins: int):
    """the six sums -> Z float64 (same leading shape); NaN if a variance is 0 or n_pairs < bins / 2.  Python integers: the
    products n * sum(da db) reach 2^62 and the variances' product leaves int64"""
    rec = np.asarray(rec, dtype=np.int64)
    Z = np.full(rec.shape[:-1], np.nan)
    for idx in np.ndindex(*rec.shape[:-1]):
        n, sa, sb, sab, saa, sbb = (int(v) for v in rec[idx])
        va, vb = n * saa - sa * sa, n * sbb - sb * sb
        if 2 * n >= bins and va > 0 and vb > 0:
            Z[idx] = (n * sab - sa * sb) / (float(va) ** 0.5 * float(vb) ** 0.5)
    return Z


# ---- 3. warp ----
def warp(src, ax, bx, ay, by, fill, Wo, Ho):
    """src u16 [n,Hs,Ws] -> u16 [n,Ho,Wo]"""
    s = np.asarray(src, dtype=np.uint16).astype(np.int64)
    n, Hs, Ws = s.shape
    u = int(ax) * np.arange(Wo, dtype=np.int64) + int(bx)
    v = int(ay) * np.arange(Ho, dtype=np.int64) + int(by)
    inx, iny = (u >= 0) & (u <= (Ws - 1) * Q), (v >= 0) & (v <= (Hs - 1) * Q)
    u, v = np.where(inx, u, 0), np.where(iny, v, 0)
    i0, j0 = u >> 16, v >> 16
    i1, j1 = np.minimum(i0 + 1, Ws - 1), np.minimum(j0 + 1, Hs - 1)
    fx, fy = ((u >> 8) & 255)[None, None, :], ((v >> 8) & 255)[None, :, None]
    top = (256 - fx) * s[:, j0][:, :, i0] + fx * s[:, j0][:, :, i1]
    bot = (256 - fx) * s[:, j1][:, :, i0] + fx * s[:, j1][:, :, i1]
    val = ((256 - fy) * top + fy * bot + 32768) >> 16
    return np.ascontiguousarray(np.where((iny[:, None] & inx[None, :])[None], val, int(fill)).astype(np.uint16))


# ---- host conversions ----
def map_to_q16(A, B, Ws: int, Wo: int):
    A, B = Fraction(A), Fraction(B)
    return rhu(Q * A * Ws / Wo), rhu(Q * ((A / (2 * Wo) + B) * Ws - Fraction(1, 2)))


def candidate(p0: int, p1: int, nb: int):
    return rhu(Fraction(int(p1) - int(p0), nb)), int(p0)


def normalised(a: int, b: int, na: int, nb: int):
    return float(Fraction(int(a) * nb, Q * na)), float(Fraction(int(b), Q * na))
