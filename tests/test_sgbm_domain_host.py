"""CPU tests of the inputs and of the oracle at the edges of the SGBM matcher's accepted domain: the contents that use the
int16 headroom, the acceptance rule's arithmetic, the oracle at the largest accepted P2 against the independent NumPy
restatement (int64 sums, clipped once), the parameter normalisation and uniquenessRatio above 100.
test_sgbm_domain_gpu.py holds the kernels to what is pinned here."""
import numpy as np
import pytest

import np_sgm
import sgbm_domain as sd
from conftest import textured_pair


@pytest.mark.parametrize("ftzero", [15, 17, 21, 31])
@pytest.mark.parametrize("W,H", [(64 + 136, 60), (64 + 70, 40), (69, 1)])
def test_ceiling_content_reaches_90_percent_of_the_box_sum_ceiling(oracle, ftzero, W, H):
    """a condition on the INPUT: without such content the headroom 25 * (2 * ftzero + 63) above P2 is never used"""
    P2 = sd.p2max(ftzero)
    L, R = sd.ceiling_pair(W, H, ftzero)
    C = oracle.cost_volume(L, R, oracle.default_params(P2=P2, P1=P2 - 1, preFilterCap=sd.CAP_OF_FTZERO[ftzero])).astype(np.int64)
    reached, ceiling = int(C.max()) - P2, sd.cost_ceiling(ftzero)
    print(f"ftzero {ftzero} {W}x{H}: max(C) - P2 = {reached} of {ceiling} ({100.0 * reached / ceiling:.1f} %)")
    assert C.min() >= P2 and reached <= ceiling
    assert reached >= 0.9 * ceiling


def test_other_contents_stay_below_the_ceiling_content(oracle):
    """binary noise against its inverse and uniform noise use far less of the headroom; the binary pair is kept
    because it saturates S and rejects about half of the pixels"""
    P2 = sd.p2max(15)
    p = oracle.default_params(P2=P2, P1=P2 - 1)
    W, H = 64 + 136, 60
    shares = {}
    for name, (L, R) in (("binary", sd.binary_inverse_pair(W, H, 1)), ("uniform", sd.noise_pair(W, H, 1))):
        shares[name] = (int(oracle.cost_volume(L, R, p).max()) - P2) / sd.cost_ceiling(15)
        print(f"{name}: {100.0 * shares[name]:.1f} % of the ceiling")
    assert shares["uniform"] < shares["binary"] < 0.9
    L, R = sd.binary_inverse_pair(W, H, 1)
    raw, S = oracle.sgbm_raw(L, R, p, want_S=True)
    assert S.max() == 32767
    valid = (raw[:, sd.D:] >= 0).mean()
    assert 0.3 < valid < 0.7


def test_acceptance_rule_arithmetic():
    assert sd.p2max(15) == 15220 and sd.p2max(31) == 14820
    assert sd.p2max(17) == 15170 and sd.p2max(21) == 15070
    for cap, ft in ((0, 15), (14, 15), (15, 15), (16, 17), (20, 21), (30, 31), (31, 31)):
        assert sd.ftzero_of(cap) == ft
        P2 = sd.p2max(ft)
        assert sd.accepted(P2, cap) and not sd.accepted(P2 + 1, cap)
        assert 2 * P2 + sd.cost_ceiling(ft) == 32765             # the rule is about an even number: one below 32767 is never hit
    assert not sd.accepted(1, 32) and not sd.accepted(1, 63)
    assert sd.accepted(12000, 0) and not sd.accepted(20000, 0)   # the two values the older tests use


@pytest.mark.parametrize("mode,dirs", [(0, np_sgm.DIRS5), (1, np_sgm.DIRS8)])
@pytest.mark.parametrize("ftzero", [15, 31])
def test_oracle_at_p2max_vs_numpy(oracle, ftzero, mode, dirs):
    """the oracle's int16 arithmetic at the largest accepted P2 (P1 = P2 - 1) on ceiling content, against int64 sums
    clipped once: cost volume, S and raw disparity; S saturates in the 5-path mode as well"""
    W, H = 90, 35                                                # the smallest tried at which the five paths saturate at ftzero = 15
    P2, cap = sd.p2max(ftzero), sd.CAP_OF_FTZERO[ftzero]
    L, R = sd.ceiling_pair(W, H, ftzero)
    p = oracle.default_params(P1=P2 - 1, P2=P2, preFilterCap=cap, mode=mode)
    C = np_sgm.cost_volume(L, R, P2=P2, ft=ftzero)
    assert np.array_equal(oracle.cost_volume(L, R, p).astype(np.int32), C)
    assert C.max() - P2 >= 0.9 * sd.cost_ceiling(ftzero)
    raw, S = oracle.sgbm_raw(L, R, p, want_S=True)
    Sn = np_sgm.aggregate(C, P1=P2 - 1, P2=P2, dirs=dirs)
    assert np.array_equal(S.astype(np.int32), Sn)
    assert S.max() == 32767, f"S must saturate in mode {mode} (max {S.max()})"
    assert np.array_equal(raw.astype(np.int32), np_sgm.wta(Sn, W))


@pytest.mark.parametrize("mode,dirs", [(0, np_sgm.DIRS5), (1, np_sgm.DIRS8)])
def test_oracle_at_p2max_textured_vs_numpy(oracle, mode, dirs):
    """the same on a textured pair, where pixels survive the uniqueness and L-R checks"""
    W, H = 82, 7
    L, R = textured_pair(W, H, 5, max_disp=15)
    for ftzero in (15, 31):
        P2 = sd.p2max(ftzero)
        p = oracle.default_params(P1=P2 - 1, P2=P2, preFilterCap=sd.CAP_OF_FTZERO[ftzero], mode=mode)
        C = np_sgm.cost_volume(L, R, P2=P2, ft=ftzero)
        assert np.array_equal(oracle.cost_volume(L, R, p).astype(np.int32), C)
        raw, S = oracle.sgbm_raw(L, R, p, want_S=True)
        Sn = np_sgm.aggregate(C, P1=P2 - 1, P2=P2, dirs=dirs)
        assert np.array_equal(S.astype(np.int32), Sn)
        assert np.array_equal(raw.astype(np.int32), np_sgm.wta(Sn, W))
        assert (raw[:, sd.D:] >= 0).any()


NORMALISATION = [
    (dict(P1=0), dict(P1=2)),
    (dict(P1=-5), dict(P1=2)),
    (dict(P2=0, P1=3), dict(P2=5, P1=3)),
    (dict(P2=0), dict(P2=601)),                                  # P2 <= 0 -> 5, then P2 < P1 + 1 -> P1 + 1 with the default P1 = 600
    (dict(P1=600, P2=600), dict(P1=600, P2=601)),
    (dict(P1=900, P2=100), dict(P1=900, P2=901)),
    (dict(uniquenessRatio=-1), dict(uniquenessRatio=10)),
    (dict(disp12MaxDiff=0), dict(disp12MaxDiff=1)),
    (dict(disp12MaxDiff=-1), dict(disp12MaxDiff=1)),
    (dict(preFilterCap=14), dict(preFilterCap=15)),
    (dict(preFilterCap=16), dict(preFilterCap=17)),
    (dict(preFilterCap=30), dict(preFilterCap=31)),
]


@pytest.mark.parametrize("given,normal", NORMALISATION, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_oracle_normalises_parameters(oracle, given, normal):
    """on a textured pair, and on one with unmatched patches where the uniqueness test and the L-R check decide pixels"""
    for L, R in (textured_pair(64 + 100, 40, seed=17), sd.patchy_pair(64 + 136, 60, 17)):
        a = oracle.sgbm_compute(L, R, oracle.default_params(**given))
        b = oracle.sgbm_compute(L, R, oracle.default_params(**normal))
        assert np.array_equal(a, b)
        assert (a[:, sd.D:] >= 0).mean() > 0.2                   # not vacuous: the pair matches under these parameters


def test_normalised_values_differ_from_their_neighbours(oracle):
    """the rules above are not satisfied by an oracle that ignores the parameter: on the patchy pair every one matters"""
    L, R = sd.patchy_pair(64 + 136, 60, 17)
    raw = lambda **kw: oracle.sgbm_raw(L, R, oracle.default_params(**kw))
    base = raw()
    assert not np.array_equal(raw(P1=2), raw(P1=40))
    assert not np.array_equal(raw(P1=3, P2=5), raw(P1=3, P2=9))
    assert not np.array_equal(raw(preFilterCap=17), raw(preFilterCap=15))
    assert not np.array_equal(base, raw(uniquenessRatio=0))
    assert not np.array_equal(base, raw(disp12MaxDiff=2)) and not np.array_equal(base, raw(disp12MaxDiff=64))


def test_uniqueness_ratio_above_100_in_the_oracle(oracle):
    """left == right noise: min S == 0 at d = 0 everywhere.  At 100 the comparison S[d] * 0 < 0 never rejects; above 100
    the factor is negative and any far S[d] > 0 rejects.  The kernels do not reproduce this: v3d_sgbm_create refuses it."""
    W, H = 200, 40
    L, R = sd.same_view_noise(W, H, 3)
    n = (W - sd.D) * H
    counts = {u: int((oracle.sgbm_raw(L, R, oracle.default_params(uniquenessRatio=u))[:, sd.D:] >= 0).sum()) for u in (100, 101, 150)}
    assert counts == {100: n, 101: 0, 150: 0}
    Ws, Hs = 82, 7
    Ls, Rs = sd.same_view_noise(Ws, Hs, 4)
    for u in (100, 101):
        raw, S = oracle.sgbm_raw(Ls, Rs, oracle.default_params(uniquenessRatio=u), want_S=True)
        assert np.array_equal(raw.astype(np.int32), np_sgm.wta(S.astype(np.int32), Ws, uniq=u))


def test_gpu_headroom_inputs_are_not_vacuous(oracle):
    """what test_sgbm_domain_gpu.py relies on, at its own sizes: the cost ceiling is reached, S saturates in the 5-path
    mode, and pixels survive into the raw disparity"""
    for cap in sd.CAPS:
        ft = sd.ftzero_of(cap)
        P2 = sd.p2max(ft)
        W, H = sd.HEADROOM_SIZES[cap]
        L, R = sd.ceiling_pair(W, H, ft)
        p = oracle.default_params(preFilterCap=cap, P2=P2, P1=P2 - 1)
        assert int(oracle.cost_volume(L, R, p).max()) - P2 >= 0.9 * sd.cost_ceiling(ft)
        raw, S = oracle.sgbm_raw(L, R, p, want_S=True)
        assert S.max() == 32767 and (raw[:, sd.D:] >= 0).mean() > 0.05


def test_gpu_speckle_inputs_have_components_of_every_size(oracle):
    """the pairs of the GPU speckle-parameter test are not vacuous: every parameter value changes the oracle's output"""
    pairs = sd.speckle_pairs()
    outs = lambda **kw: [oracle.sgbm_compute(L, R, oracle.default_params(**kw)) for L, R in pairs]
    differ = lambda a, b: any(not np.array_equal(x, y) for x, y in zip(a, b))
    base, off = outs(), outs(speckleWindowSize=-1)
    assert differ(base, off) and differ(off, outs(speckleWindowSize=1)) and differ(base, outs(speckleWindowSize=1))
    assert differ(base, outs(speckleRange=0)) and differ(base, outs(speckleRange=2048))
    assert all((o[:, sd.D:] >= 0).any() for o in off)
    for (L, R), o in zip(pairs, outs(speckleWindowSize=10 ** 6)):
        assert (o == -16).all()
