"""Spatial registration of the SBS clip's left eye to the 4K clip (no counterpart in the reference, which assumes both releases
share one framing).

The model is one affine map per axis, (Ax, Bx, Ay, By) in normalised plane coordinates: the 4K point at the fraction xi = (X + 1/2)
/ Whi of the width shows what the left eye shows at the fraction sigma = Ax xi + Bx of its width, likewise Ay, By for the height;
the identity is (1, 0, 1, 0).  It covers crop, letterbox, pillarbox, uniform and anamorphic scale and shift.

estimate() -- the align CLI's --register-spatial -- takes a few probe frames, has the device sum the rows and the columns of the
left eye's gray plane and of the 4K luma (v3d_plane_profiles_batch) and scores candidate maps between the profiles of an axis in
exact integers (v3d_profile_match_scores); the search policy (search_axis), the correlation (zncc) and the decision rule (decide)
are plain NumPy here.  spatial_block() / resolve() carry the result through alignment_data.json to the upscale and pipeline CLIs,
which warp the low-res u16 depth into the 4K frame's framing (v3d_warp_u16_batch, warp_q16) right before the guided filter.

Bit-exact contract of the device part, and the rounding of every conversion to Q16 done here: tests/register_ref.py.
"""
import math
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .framematch import FPS_TOLERANCE, _clip_frames, probe_starts
from .utils import get_video_info, iter_frames

Q = 65536
DEFAULT_PROBES, DEFAULT_MIN_SCORE, DEFAULT_BINS = 3, 0.5, 512          # min score: a product convention, as framematch's
SCALE_SPAN, OFFSET_SPAN = (Fraction(4, 5), Fraction(5, 4)), Fraction(1, 4)   # the first grid: x0.8 .. x1.25, +-25 % of the source
FINEST_STEP = Q // 8                                                   # no source sample moves further in the last refinement
A_MIN, A_MAX, B_MAX = 1 << 12, 1 << 20, 1 << 29                        # candidate domain of v3d_profile_match_scores
MAX_CANDIDATES = 65535
IDENTITY = (1.0, 0.0, 1.0, 0.0)
AGREE = Q                                                              # probes agree within one source pixel at both ends
ADVICE = "python -m video_3d_pipeline.align --register-spatial"


# ---- conversions to Q16: round half up in exact rationals (a float is an exact rational) ----
def rhu(x) -> int:
    return int((Fraction(x) + Fraction(1, 2)).__floor__())


def map_to_q16(A, B, Ws: int, Wo: int) -> Tuple[int, int]:
    """normalised map of one axis -> the warp's (ax, bx) for a source of Ws samples and an output grid of Wo: output pixel xo
    sits at xi = (xo + 1/2) / Wo, its source index is (A xi + B) Ws - 1/2 (low-res samples at pixel centres, as the guided
    filter places them)"""
    A, B = Fraction(A), Fraction(B)
    return rhu(Q * A * Ws / Wo), rhu(Q * ((A / (2 * Wo) + B) * Ws - Fraction(1, 2)))


def candidate(p0: int, p1: int, nb: int) -> Tuple[int, int]:
    """source positions (Q16) of the target's first and last edge -> the match entry's (a, b)"""
    return rhu(Fraction(int(p1) - int(p0), nb)), int(p0)


def normalised(a: int, b: int, na: int, nb: int) -> Tuple[float, float]:
    """the match entry's (a, b) between profiles of na and nb samples -> (A, B), the nearest float64 of the exact value"""
    return float(Fraction(int(a) * nb, Q * na)), float(Fraction(int(b), Q * na))


def ends(a: int, b: int, nb: int) -> Tuple[int, int]:
    """where (a, b) puts the target's two ends in the source, Q16"""
    return int(b), ((int(a) * nb * Q) >> 16) + int(b)


def zncc(rec, bins: int) -> np.ndarray:
    """the records of v3d_profile_match_scores [..., 6] -> Z float64 [...]; NaN where a variance is 0 or n_pairs < bins / 2 (a
    candidate that overlaps less than half of the target carries no vote; the in-band refusal n_pairs = -1 has none either).
    int64 holds every term: n <= 2^10, sums of products < 2^52, squares of sums < 2^62."""
    r = np.asarray(rec, dtype=np.int64)
    n, sa, sb, sab, saa, sbb = (r[..., i] for i in range(6))
    va, vb, num = n * saa - sa * sa, n * sbb - sb * sb, n * sab - sa * sb
    ok = (2 * n >= bins) & (va > 0) & (vb > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = num.astype(np.float64) / (np.sqrt(va.astype(np.float64)) * np.sqrt(vb.astype(np.float64)))
    return np.where(ok, Z, np.nan)


# ---- search policy ----
def search_levels(na: int, nb: int, bins: int) -> List[Tuple[int, int, int]]:
    """[(bins, step in Q16 source samples, reach in steps)] coarse to fine for an axis with na source and nb target samples.  The
    first level scores an eighth of the bins on a grid of half such a bin; each refinement looks `reach` steps around the best
    candidate of the level before, the last one in steps of at most 1/8 source sample with all the bins (at most one per sample
    of either profile)."""
    bf = max(8, min(int(bins), nb, na))                                  # a bin below one source sample repeats that sample: no finer
    b0, b1 = max(8, bf // 8), max(8, bf // 2)
    step0 = max((Q * na) // (2 * b0), FINEST_STEP)
    r = max(2, math.isqrt(-(-step0 // FINEST_STEP) - 1) + 1)               # ceil(sqrt(step0 / FINEST_STEP)): r * r * FINEST_STEP >= step0
    step1 = max(step0 // r, 1)
    step2 = max(min(step1 // r, FINEST_STEP), 1)
    return [(b0, step0, 0), (b1, step1, -(-step0 // step1)), (bf, step2, -(-step1 // step2))]


def first_grid(na: int, nb: int, step: int) -> np.ndarray:
    """the first level's (p0, p1) pairs, int64 [C,2]: offsets p0 over +-25 % of the source, spans p1 - p0 over x0.8 .. x1.25 of it,
    both on a grid of `step` through the nominal map (0, na 65536)"""
    full = na * Q
    k0 = int(full * OFFSET_SPAN) // step
    lo, hi = -(int(full * (1 - SCALE_SPAN[0])) // step), int(full * (SCALE_SPAN[1] - 1)) // step
    p0 = np.arange(-k0, k0 + 1, dtype=np.int64) * step
    span = full + np.arange(lo, hi + 1, dtype=np.int64) * step
    return np.stack([np.repeat(p0, len(span)), (p0[:, None] + span[None, :]).reshape(-1)], axis=1)


def refine_grid(best: Sequence[int], step: int, reach: int) -> np.ndarray:
    """(p0, p1) pairs `reach` steps of `step` around `best` at either end"""
    k = np.arange(-reach, reach + 1, dtype=np.int64) * step
    return np.stack([np.repeat(best[0] + k, len(k)), np.tile(best[1] + k, len(k))], axis=1)


def to_candidates(pairs: np.ndarray, nb: int) -> Tuple[np.ndarray, np.ndarray]:
    """(p0, p1) pairs -> (the pairs inside the entry's domain, their (a, b) int64 [C,2]); a = rhu((p1 - p0) / nb) in integers"""
    span = pairs[:, 1] - pairs[:, 0]
    a = (2 * span + nb) // (2 * nb)                                      # floor(span / nb + 1/2)
    keep = (a >= A_MIN) & (a <= A_MAX) & (np.abs(pairs[:, 0]) <= B_MAX)
    return pairs[keep], np.stack([a[keep], pairs[keep, 0]], axis=1)


def pick(Z: np.ndarray, pairs: np.ndarray, na: int) -> Optional[int]:
    """the index of the largest defined Z; ties go to the candidate nearest the nominal map (0, na 65536), then to the first"""
    if not len(Z) or np.all(np.isnan(Z)):
        return None
    top = np.flatnonzero(Z == np.nanmax(Z))
    dist = np.abs(pairs[top, 0]) + np.abs(pairs[top, 1] - na * Q)
    return int(top[np.argmin(dist)])


def search_axis(score, na: int, nb: int, bins: int) -> Optional[Dict]:
    """one probe, one axis.  score(cand int64 [C,2], bins) -> records [C,6] (the device entry, or a stand-in).  -> dict(a, b, z)
    of the finest level's best candidate, or None when no candidate of a level has a defined Z (a flat profile)"""
    best = None
    for level, (b, step, reach) in enumerate(search_levels(na, nb, bins)):
        pairs = first_grid(na, nb, step) if level == 0 else refine_grid(best, step, reach)
        pairs, cand = to_candidates(pairs, nb)
        if not len(cand):
            return None
        Z = np.concatenate([zncc(score(cand[i:i + MAX_CANDIDATES], b), b) for i in range(0, len(cand), MAX_CANDIDATES)])
        i = pick(Z, pairs, na)
        if i is None:
            return None
        best, out = pairs[i], dict(a=int(cand[i, 0]), b=int(cand[i, 1]), z=float(Z[i]))
    return out


# ---- decision rule ----
def _median(values: Sequence[int]) -> int:
    v = sorted(int(x) for x in values)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) // 2


def decide(probes_x: Sequence[Optional[Dict]], probes_y: Sequence[Optional[Dict]], size_eye: Tuple[int, int], size_guide: Tuple[int, int],
           min_score: float = DEFAULT_MIN_SCORE) -> Dict:
    """The decision rule.  probes_x / probes_y: per probe the search_axis result of that axis (None: no defined Z).
    1. per axis, the map is the median of a and of b over the probes that have a Z (integers; an even count takes the floor of
       the two middle values' mean), its score the median of their Z;
    2. a probe agrees iff its map puts both ends of the target within one source pixel of where the median puts them;
    3. registered iff both axes have a median, both scores are >= min_score and every probe agrees on both axes;
    4. otherwise inconsistent iff a probe disagrees (a film that switches aspect ratio), else undetermined (flat or black probes,
       weak texture); both keep the identity."""
    out, agree, q16, scores = dict(status="undetermined", map=IDENTITY, map_q16=None, score=None), True, [], []
    for probes, na, nb in ((probes_x, size_eye[0], size_guide[0]), (probes_y, size_eye[1], size_guide[1])):
        have = [p for p in probes if p is not None and not np.isnan(p["z"])]
        if not have:
            q16.append(None)
            continue
        a, b = _median([p["a"] for p in have]), _median([p["b"] for p in have])
        z = sorted(p["z"] for p in have)
        scores.append((z[(len(z) - 1) // 2] + z[len(z) // 2]) / 2)
        e = ends(a, b, nb)
        agree = agree and all(max(abs(u - v) for u, v in zip(ends(p["a"], p["b"], nb), e)) <= AGREE for p in have)
        q16.append((a, b))
    if not agree:
        out["status"] = "inconsistent"
    if None in q16:
        return out
    out.update(map_q16=[list(q16[0]), list(q16[1])], score=[float(s) for s in scores])
    if agree and min(scores) >= min_score:
        (Ax, Bx), (Ay, By) = normalised(*q16[0], size_eye[0], size_guide[0]), normalised(*q16[1], size_eye[1], size_guide[1])
        out.update(status="registered", map=(Ax, Bx, Ay, By))
    return out


def check_parameters(probes, min_score, bins):
    for name, v, lo, hi in (("probes", probes, 1, 64), ("bins", bins, 8, 1024)):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError(f"register {name} must be an integer in [{lo}, {hi}], got {v!r}")
    if not np.isfinite(min_score):
        raise ValueError(f"register min_score must be finite, got {min_score!r}")
    return int(probes), float(min_score), int(bins)


def estimate(sbs_video: str, video_4k: str, guide_start_frame: int, start_frame: int = 0, probes: int = DEFAULT_PROBES,
             unsqueeze: bool = True, max_frames: Optional[int] = None, min_score: float = DEFAULT_MIN_SCORE, bins: int = DEFAULT_BINS,
             backend=None, input_layout: str = "sbs") -> Dict:
    """Fit the left eye of the SBS clip to the 4K clip.  `probes` single frames spread over the clip (framematch.probe_starts), SBS
    frame start_frame + s against 4K frame guide_start_frame + s; the backend puts the left-eye gray (the plane the matcher sees:
    unsqueezed unless told otherwise) and the 4K luma on the device and returns their profiles (sbs_left_profiles,
    guide_profiles), match_scores(prof_a, prof_b, cand, bins) runs the device entry and returns the records.  Returns decide()'s
    result plus the per-probe maps, both plane sizes and the parameters.  input_layout "tb": the left eye is the top half of the
    frame (the backend's call and the result gain the keyword; an SBS run's are what they were).  ValueError: unreadable clips,
    unequal frame rates, bad parameters."""
    probes, min_score, bins = check_parameters(probes, min_score, bins)
    info_s, info_g = get_video_info(sbs_video), get_video_info(video_4k)
    if not info_s or not info_g:
        raise ValueError(f"Could not read video info: {sbs_video if not info_s else video_4k}")
    if abs(float(info_s["fps"]) - float(info_g["fps"])) > FPS_TOLERANCE:
        raise ValueError(f"spatial registration refused: frame rates differ ({info_s['fps']:.3f} vs {info_g['fps']:.3f} fps)")
    from .depth import check_frame_halves, check_input_layout, sbs_eye_size
    layout = {"input_layout": check_input_layout(input_layout)} if input_layout != "sbs" else {}
    check_frame_halves(info_s["width"], info_s["height"], input_layout)
    count, n4k = _clip_frames(info_s, start_frame, max_frames), _clip_frames(info_g)
    if count < 1:
        raise ValueError("No frames extracted from video")
    if backend is None:
        from .pipeline import HipPipelineBackend
        backend = HipPipelineBackend("cuda")
    g0 = int(guide_start_frame)
    used, sbs, guides = [], [], []
    for s in probe_starts(count, 1, probes)[0]:
        if not 0 <= g0 + s < n4k:
            continue                                              # the probe lies outside the 4K clip
        f, g = list(iter_frames(sbs_video, start_frame + s, 1)), list(iter_frames(video_4k, g0 + s, 1))
        if f and g:
            used.append(int(s)); sbs.append(f[0]); guides.append(g[0])
    We, He = sbs_eye_size(info_s, unsqueeze, **layout)
    Wg, Hg = info_g["width"], info_g["height"]
    px: List[Optional[Dict]] = []
    py: List[Optional[Dict]] = []
    if used:
        col_e, row_e = backend.sbs_left_profiles(sbs, unsqueeze, **layout)
        col_g, row_g = backend.guide_profiles(guides, Hg, Wg)
        for p in range(len(used)):
            px.append(search_axis(lambda c, b: backend.match_scores(col_e[p:p + 1], col_g[p:p + 1], c, b)[0], We, Wg, bins))
            py.append(search_axis(lambda c, b: backend.match_scores(row_e[p:p + 1], row_g[p:p + 1], c, b)[0], He, Hg, bins))
    out = decide(px, py, (We, He), (Wg, Hg), min_score)
    out.update(probe_frames=used, probes_x=px, probes_y=py, eye_size=[We, He], guide_size=[Wg, Hg], unsqueeze=bool(unsqueeze),
               parameters=dict(probes=probes, min_score=min_score, bins=bins, start_frame=int(start_frame), max_frames=max_frames,
                               guide_start_frame=g0), **layout)
    return out


# ---- alignment_data.json ----
def spatial_block(res: Dict) -> Dict:
    """what an estimate() result adds to alignment_data.json under "spatial" """
    def probe(p, na, nb):
        if p is None:
            return None
        A, B = normalised(p["a"], p["b"], na, nb)
        return dict(a=p["a"], b=p["b"], A=A, B=B, score=p["z"])
    (We, He), (Wg, Hg) = res["eye_size"], res["guide_size"]
    return dict(status=res["status"], map=[float(v) for v in res["map"]], map_q16=res["map_q16"], score=res["score"],
                probe_frames=res["probe_frames"], probes_x=[probe(p, We, Wg) for p in res["probes_x"]],
                probes_y=[probe(p, He, Hg) for p in res["probes_y"]], eye_size=[We, He], guide_size=[Wg, Hg],
                unsqueeze=res["unsqueeze"], parameters=res["parameters"],
                **({"input_layout": res["input_layout"]} if res.get("input_layout", "sbs") != "sbs" else {}))


def parse_map(text: str) -> Tuple[float, float, float, float]:
    """--spatial-map Ax,Bx,Ay,By"""
    try:
        m = tuple(float(v) for v in str(text).split(","))
    except ValueError:
        m = ()
    if len(m) != 4 or not all(np.isfinite(m)) or m[0] <= 0 or m[2] <= 0:
        raise ValueError(f"--spatial-map wants Ax,Bx,Ay,By with finite numbers and positive scales, got {text!r}")
    return m


def resolve(alignment_file: Optional[str], no_spatial: bool = False, spatial_map: Optional[str] = None,
            eye_size: Optional[Sequence[int]] = None, guide_size: Optional[Sequence[int]] = None, unsqueeze: Optional[bool] = None,
            input_layout: Optional[str] = None) -> Optional[Dict]:
    """What a run applies: None (nothing: no block, --no-spatial, a block that is not `registered`, or the identity) or dict(map,
    source).  --spatial-map wins over the file.  A block estimated on other plane sizes (eye_size, guide_size: (W, H), or a
    callable that returns it or None), with another unsqueeze setting or with another input layout than the run's (each compared
    where the run knows it; a CLI with --input-layout passes it only for "tb", and None here stands for "sbs" once the run knows its
    unsqueeze setting) is refused: ValueError."""
    if no_spatial:
        return None
    if spatial_map is not None:
        m, source = parse_map(spatial_map), "--spatial-map"
    else:
        if alignment_file is None:
            return None
        from .align import load_alignment_data
        block = load_alignment_data(alignment_file).get("spatial")
        if not block or block.get("status") != "registered":
            return None
        if unsqueeze is not None and block.get("unsqueeze") is not None and bool(block["unsqueeze"]) != bool(unsqueeze):
            raise ValueError(f"{alignment_file}: the spatial map was estimated with unsqueeze={bool(block['unsqueeze'])}, this run has "
                             f"unsqueeze={bool(unsqueeze)}; estimate it again with `{ADVICE}` or pass --no-spatial")
        if unsqueeze is not None or input_layout is not None:         # a run that splits the clip itself knows its layout
            mine_layout, theirs_layout = input_layout or "sbs", block.get("input_layout") or "sbs"
            if mine_layout != theirs_layout:
                raise ValueError(f"{alignment_file}: the spatial map was estimated with input_layout={theirs_layout}, this run has "
                                 f"input_layout={mine_layout}; estimate it again with `{ADVICE}` or pass --no-spatial")
        for name, mine, theirs in (("left-eye plane", eye_size, block.get("eye_size")), ("4K frame", guide_size, block.get("guide_size"))):
            mine = mine() if callable(mine) else mine                 # a CLI reads its clips' sizes only when there is a block to hold them to
            if mine is not None and theirs is not None and [int(v) for v in mine] != [int(v) for v in theirs]:
                raise ValueError(f"{alignment_file}: the spatial map was estimated on a {name} of {theirs[0]}x{theirs[1]}, this run has "
                                 f"{mine[0]}x{mine[1]}; estimate it again with `{ADVICE}` or pass --no-spatial")
        m, source = parse_map(",".join(repr(float(v)) for v in block["map"])), str(alignment_file)
    if tuple(m) == IDENTITY:
        return None
    return dict(map=tuple(m), source=source, eye_size=block.get("eye_size") if spatial_map is None else None)


def check_block_size(applied: Dict, width: int, height: int):
    """the upscale CLI learns the low-res size (and with it the unsqueeze setting of the depth run) from the depth maps themselves:
    a map estimated on another left-eye plane is refused"""
    eye = applied.get("eye_size")
    if eye is not None and [int(eye[0]), int(eye[1])] != [int(width), int(height)]:
        raise ValueError(f"{applied['source']}: the spatial map was estimated on a left-eye plane of {eye[0]}x{eye[1]}, the depth maps are "
                         f"{width}x{height} (another size or unsqueeze setting); estimate it again with `{ADVICE}` or pass --no-spatial")


def warp_q16(amap: Sequence[float], src_size: Sequence[int], guide_size: Sequence[int]) -> Dict:
    """the numbers of v3d_warp_u16_batch for a low-res plane of src_size (W, H) and a 4K frame of guide_size: the output grid is
    ceil(Whi / 2) x ceil(Hhi / 2), the guided filter's exact-2x route when the 4K size is even.  ValueError outside the entry's
    domain."""
    (Ws, Hs), (Whi, Hhi) = src_size, guide_size
    Wo, Ho = (Whi + 1) // 2, (Hhi + 1) // 2
    ax, bx = map_to_q16(amap[0], amap[1], Ws, Wo)
    ay, by = map_to_q16(amap[2], amap[3], Hs, Ho)
    if not (A_MIN <= ax <= A_MAX and A_MIN <= ay <= A_MAX and abs(bx) <= 1 << 40 and abs(by) <= 1 << 40):
        raise ValueError(f"spatial map {tuple(amap)} from {Ws}x{Hs} to {Wo}x{Ho} leaves the warp's range (steps of 1/16 .. 16 source samples)")
    return dict(q=(ax, bx, ay, by), size=(Wo, Ho))


def manifest_entries(applied: Optional[Dict]) -> Dict:
    """what a run that applied a map adds to its output manifest"""
    return {} if applied is None else {"spatial_map": [float(v) for v in applied["map"]], "spatial_map_source": applied["source"]}


def add_register_arguments(parser):
    parser.add_argument('--register-spatial', action='store_true',
                        help='After the temporal steps, fit the left eye to the 4K frame (crop, letterbox, scale, shift per axis) on the GPU')
    parser.add_argument('--register-probes', type=int, default=DEFAULT_PROBES, help=f'Probe frames spread over the clip (default {DEFAULT_PROBES})')
    parser.add_argument('--register-min-score', type=float, default=DEFAULT_MIN_SCORE, help=f'Least correlation to accept (default {DEFAULT_MIN_SCORE})')
    parser.add_argument('--register-bins', type=int, default=DEFAULT_BINS, help=f'Bins of the profile match (default {DEFAULT_BINS})')


def add_apply_arguments(parser):
    parser.add_argument('--no-spatial', action='store_true', help='Ignore the spatial block of --alignment-file')
    parser.add_argument('--spatial-map', default=None, metavar='Ax,Bx,Ay,By',
                        help='Warp the low-res depth through this map (normalised plane coordinates) before the guided filter')
