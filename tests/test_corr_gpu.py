"""GPU parity of the MFMA correlation lookup (BASELINE config 4) against the fp32 oracle.
bf16 inputs, f32 accumulate; the warped right features are rounded to bf16 once: tolerance 2e-2 of the
output scale.  The fp32 oracle does not model that bf16 rounding; the tight bar is
tests/test_corr_accuracy_gpu.py, which holds every route to the per-output interval of the float64 reference
tests/corr_ref.py (about one float32 ulp of the output's scale)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("h,w,G", [(12, 48, 4), (9, 37, 2), (30, 64, 4)])
def test_corr_matches_oracle(native, oracle, pattern, h, w, G):
    rng = np.random.default_rng(h * w + pattern)
    C = 64 * G
    fl = _bf16_round(rng.normal(0, 1, (C, h, w)).astype(np.float32))
    fr = _bf16_round(rng.normal(0, 1, (C, h, w)).astype(np.float32))
    flow = rng.uniform(-3, 3, (2, h, w)).astype(np.float32)
    want = oracle.corr_lookup(fl, fr, flow, G, pattern)
    fl_d = torch.from_numpy(fl).permute(1, 2, 0).contiguous().to("cuda", torch.bfloat16)
    fr_d = torch.from_numpy(fr).permute(1, 2, 0).contiguous().to("cuda", torch.bfloat16)
    got = native.corr_lookup(fl_d, fr_d, torch.from_numpy(flow).cuda(), G, pattern).cpu().numpy()
    # per element: SURVEY 8(d)'s rtol 2e-2 plus a floor of 2 % of the typical output (rms) for values near zero
    rms = float(np.sqrt(np.mean(want.astype(np.float64) ** 2)))
    err, bound = np.abs(got - want), 2e-2 * np.abs(want) + 2e-2 * rms
    assert (err <= bound).all(), f"worst err/bound {float((err / bound).max()):.3f} (max abs err {float(err.max()):.4e})"


@pytest.mark.parametrize("pattern", [0, 1])
def test_configs3_full_size_against_the_oracle(native, oracle, pattern):
    """BASELINE configs[3] at its real size (270 x 480 x 256 features, G = 4, both offset patterns) against the fp32 oracle
    -- not against another HIP kernel.  Per-element bound |got - want| <= 2e-2 |want| + 2e-2 rms(want): SURVEY 8(d)'s
    rtol 2e-2 plus a floor for outputs near zero (a sum of 64 signed products has no relative accuracy at its zero
    crossings; the floor is 2 % of the typical output, ~9 sigma of the bf16 rounding of the warped features)."""
    h, w, G = 270, 480, 4
    C = 64 * G
    rng = np.random.default_rng(270 * 480 + pattern)
    fl = _bf16_round(rng.normal(0, 1, (C, h, w)).astype(np.float32))
    fr = _bf16_round(rng.normal(0, 1, (C, h, w)).astype(np.float32))
    flow = rng.uniform(-4, 4, (2, h, w)).astype(np.float32)
    want = oracle.corr_lookup(fl, fr, flow, G, pattern)
    fl_d = torch.from_numpy(fl).permute(1, 2, 0).contiguous().to("cuda", torch.bfloat16)
    fr_d = torch.from_numpy(fr).permute(1, 2, 0).contiguous().to("cuda", torch.bfloat16)
    got = native.corr_lookup(fl_d, fr_d, torch.from_numpy(flow).cuda(), G, pattern).cpu().numpy()
    assert got.shape == want.shape == (G * 9, h, w)
    rms = float(np.sqrt(np.mean(want.astype(np.float64) ** 2)))
    err = np.abs(got - want)
    bound = 2e-2 * np.abs(want) + 2e-2 * rms
    worst = float((err / bound).max())
    assert worst <= 1.0, f"worst err/bound {worst:.3f} (max abs err {float(err.max()):.3e}, rms(want) {rms:.3e})"


def test_one_hot_channels_pick_shifted_copies(native):
    """one-hot features + zero flow: corr picks the (clamped) shifted copies (SURVEY 8c known-answer 12)"""
    h, w, G = 4, 32, 1
    C = 64
    fl = np.zeros((h, w, C), np.float32)
    fr = np.zeros((h, w, C), np.float32)
    fl[..., 0] = 1.0
    fr[..., 0] = np.arange(w, dtype=np.float32)[None, :]          # exactly representable in bf16 up to 256
    out = native.corr_lookup(torch.from_numpy(fl).to("cuda", torch.bfloat16), torch.from_numpy(fr).to("cuda", torch.bfloat16),
                             torch.zeros((2, h, w), device="cuda"), G, 0).cpu().numpy()
    for k in range(9):
        want = np.clip(np.arange(w) + k - 4, 0, w - 1) / 64.0
        assert np.allclose(out[k], want[None, :], atol=1e-6), k


def test_rejects_bad_channels(native):
    a = torch.zeros((4, 16, 48), device="cuda", dtype=torch.bfloat16)
    with pytest.raises(native.NativeError):
        native.corr_lookup(a, a, torch.zeros((2, 4, 16), device="cuda"), 1, 0)


def test_fused_gather_gemm_is_bit_identical(native):
    """option corr_gather=1 builds the B operand on the fly (no materialised warp): same bits, measured slower"""
    h, w, G = 10, 40, 2
    g = torch.Generator(device="cpu").manual_seed(3)
    fl = torch.randn((h, w, 64 * G), generator=g).to("cuda", torch.bfloat16)
    fr = torch.randn((h, w, 64 * G), generator=g).to("cuda", torch.bfloat16)
    flow = (torch.rand((2, h, w), generator=g) * 6 - 3).cuda()
    for pat in (0, 1):
        a = native.corr_lookup(fl, fr, flow, G, pat)
        native.set_option("corr_gather", 1)
        try:
            b = native.corr_lookup(fl, fr, flow, G, pat)
        finally:
            native.set_option("corr_gather", 0)
        assert torch.equal(a, b)


@pytest.mark.parametrize("h,w,G", [(10, 40, 2), (7, 64, 4), (5, 130, 4), (3, 17, 1), (270, 480, 4)])
def test_lds_gather_gemm_equals_the_two_kernel_form(native, h, w, G):
    """k_corr_fused0 (1x9 default: the block's 72 warped positions staged once in LDS, outputs transposed through LDS) gives the
    bits of k_corr_warp + k_corr: ragged last block, rows narrower than a block, the full 270x480x256 shape"""
    g = torch.Generator(device="cpu").manual_seed(h * w)
    fl = torch.randn((h, w, 64 * G), generator=g).to("cuda", torch.bfloat16)
    fr = torch.randn((h, w, 64 * G), generator=g).to("cuda", torch.bfloat16)
    flow = (torch.rand((2, h, w), generator=g) * 8 - 4).cuda()
    try:
        native.set_option("corr_fused", 1)
        a = native.corr_lookup(fl, fr, flow, G, 0)
        native.set_option("corr_fused", 0)
        b = native.corr_lookup(fl, fr, flow, G, 0)
    finally:
        native.set_option("corr_fused", 1)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} differ, max {float((a - b).abs().max())}"
