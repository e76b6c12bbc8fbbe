"""Host logic of --png-encoder {zlib,gpu} on the CPU: the stand-in backends of test_host.py / test_pipeline_host.py /
test_convert_host.py, extended with the three `gpu` methods, which serve the streams of tests/png_ref.py (what the device
produces, bit for bit).  The default creates no encoder and calls none of the new methods; `gpu` writes the same file names
with the same decoded pixels; the flag exists, with its validation, on all four CLIs."""
import io
import json
import os

import numpy as np
import pytest

import png_ref as P
import stereo_ref as R
from test_convert_host import RefRenderBackend, RefStereoPipelineBackend, _clip4k, _depths, W4, H4
from test_host import OracleStereoBackend, OracleUpscaleBackend
from test_pipeline_host import SW, SH

CALLS = []


def _stream(img, fmt):
    return np.frombuffer(P.stream(np.asarray(img), fmt), np.uint8)


class PngStereo(OracleStereoBackend):
    def png_streams_u16(self, u16):
        CALLS.append("png_streams_u16")
        return [_stream(np.asarray(f, np.uint16), P.GRAY16) for f in u16]


class PngPipeline(RefStereoPipelineBackend, PngStereo):
    def render_stereo_png(self, u16_4k, gains, layout):
        CALLS.append("render_stereo_png")
        return [None if f is None else _stream(f, P.BGR8) for f in self.render_stereo(u16_4k, gains, layout)]


class PngUpscale(OracleUpscaleBackend):
    def upscale_png(self, depth_lo, guide, r, eps):
        CALLS.append("upscale_png")
        return _stream(self.upscale_u16(depth_lo, guide, r, eps), P.GRAY16)


class PngRender(RefRenderBackend):
    def render_batch_png(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None):
        CALLS.append("render_batch_png")
        return [_stream(f, P.BGR8) for f in self.render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity)]


def _decoded(d):
    """{file name: pixels} of a directory of PNGs (other files: their bytes)"""
    from PIL import Image
    out = {}
    for f in sorted(os.listdir(d)):
        data = open(os.path.join(d, f), "rb").read()
        if f.endswith(".png"):
            with Image.open(io.BytesIO(data)) as im:
                out[f] = np.asarray(im).copy()
        else:
            out[f] = data
    return out


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture()
def clips(tmp_path):
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.utils import write_png16
    np.save(tmp_path / "sbs.npy", np.stack([syn.sbs_frame(SW, SH, i) for i in range(5)]))
    np.save(tmp_path / "guide.npy", np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(4)]))
    np.save(tmp_path / "v4k.npy", _clip4k(5))
    ddir = tmp_path / "depth_4k_frames"
    ddir.mkdir()
    for i, d in enumerate(_depths(5)):
        write_png16(ddir / f"depth4k_{i:06d}.png", d)
    CALLS.clear()
    return tmp_path


def test_depth_cli_gpu_mode_writes_the_same_pixels(clips):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    dirs = {}
    for mode in ("zlib", "gpu"):
        work = str(clips / f"d_{mode}")
        ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=2, stereo_only=True, backend=PngStereo(), png_encoder=mode)
        dirs[mode] = ex.process_video_sbs(str(clips / "sbs.npy"))
        assert (CALLS == []) if mode == "zlib" else (CALLS == ["png_streams_u16"] * 3)
    assert dirs["zlib"].name == dirs["gpu"].name                   # the encoder is no part of the cache key: same maps
    _same(_decoded(dirs["zlib"]), _decoded(dirs["gpu"]))
    from video_3d_pipeline.utils import read_png16, _decode_png16_fast
    f = sorted(dirs["gpu"].glob("depth_*.png"))[0]
    assert _decode_png16_fast(f.read_bytes()) is not None and np.array_equal(read_png16(f), read_png16(dirs["zlib"] / f.name))


def test_default_backends_need_no_new_method(clips):
    """zlib mode runs on stand-ins that do not have the gpu methods at all"""
    from video_3d_pipeline import convert
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    work = str(clips / "plain")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=2, stereo_only=True, backend=OracleStereoBackend())
    assert ex.png_encoder == "zlib"
    ddir = ex.process_video_sbs(str(clips / "sbs.npy"), max_frames=2)
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    up.process_depth_upscaling(str(ddir), str(clips / "guide.npy"), output_path=str(clips / "plain_up.json"))
    pipe = SbsTo4kDepthPipeline(work_dir=work, batch_size=2, stereo_only=True, backend=RefStereoPipelineBackend())
    pipe.run(str(clips / "sbs.npy"), str(clips / "guide.npy"), output_path=str(clips / "plain_pipe.json"), max_frames=2,
             stereo_output=str(clips / "plain_3d.json"))
    assert convert.main([str(clips / "v4k.npy"), str(clips / "depth_4k_frames"), "--output", str(clips / "plain_c.json")],
                        backend=RefRenderBackend()) == 0
    assert CALLS == []
    for be in (ex.backend, up.backend, pipe.backend):
        assert not hasattr(be, "_png")


def test_upscale_cli_gpu_mode_writes_the_same_pixels(clips):
    from video_3d_pipeline import upscale
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(clips / "u")
    ddir = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, stereo_only=True, backend=OracleStereoBackend()).process_video_sbs(
        str(clips / "sbs.npy"), max_frames=3)
    out = {}
    for mode in ("zlib", "gpu"):
        o = clips / f"up_{mode}.json"
        assert upscale.main([str(ddir), str(clips / "guide.npy"), "--output", str(o), "--png-encoder", mode], backend=PngUpscale()) == 0
        out[mode] = json.loads(o.read_text())
        assert (CALLS == []) if mode == "zlib" else (CALLS == ["upscale_png"] * 3)
    _same(_decoded(out["zlib"]["frames_dir"]), _decoded(out["gpu"]["frames_dir"]))
    assert {k: v for k, v in out["zlib"].items() if k != "frames_dir"} == {k: v for k, v in out["gpu"].items() if k != "frames_dir"}


def test_pipeline_gpu_mode_writes_the_same_pixels(clips):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    man = {}
    for mode in ("zlib", "gpu"):
        pipe = SbsTo4kDepthPipeline(work_dir=str(clips / f"p_{mode}"), batch_size=2, stereo_only=True, backend=PngPipeline(), png_encoder=mode)
        out = pipe.run(str(clips / "sbs.npy"), str(clips / "guide.npy"), output_path=str(clips / f"p_{mode}.json"), keep_depth_maps=True,
                       stereo_output=str(clips / f"s_{mode}.json"))
        man[mode] = (json.loads(open(out).read()), json.loads((clips / f"s_{mode}.json").read_text()), pipe.extractor.get_cache_path(str(clips / "sbs.npy"), 0, 5))
        if mode == "zlib":
            assert CALLS == []
    assert set(CALLS) == {"png_streams_u16", "render_stereo_png"} and CALLS.count("render_stereo_png") == 2     # 5 frames, 4 guides, passes of 2
    for k in (0, 1):
        _same(_decoded(man["zlib"][k]["frames_dir"]), _decoded(man["gpu"][k]["frames_dir"]))
        assert {a: b for a, b in man["zlib"][k].items() if a != "frames_dir"} == {a: b for a, b in man["gpu"][k].items() if a != "frames_dir"}
    _same(_decoded(man["zlib"][2]), _decoded(man["gpu"][2]))
    assert man["zlib"][1]["count"] == 4


def test_convert_cli_gpu_mode_writes_the_same_pixels(clips):
    from video_3d_pipeline import convert
    out = {}
    for mode in ("zlib", "gpu"):
        o = clips / f"c_{mode}.json"
        be = PngRender()
        assert convert.main([str(clips / "v4k.npy"), str(clips / "depth_4k_frames"), "--output", str(o), "--layout", "half-sbs",
                             "--png-encoder", mode], backend=be) == 0
        out[mode] = json.loads(o.read_text())
        assert be.batches == [4, 1] and ((CALLS == []) if mode == "zlib" else (CALLS == ["render_batch_png"] * 2))
    a, b = _decoded(out["zlib"]["frames_dir"]), _decoded(out["gpu"]["frames_dir"])
    _same(a, b)
    gains = R.stereo_gains()
    assert np.array_equal(b["frame_000000.png"][..., ::-1], R.render(_clip4k(5)[0], _depths(5)[0], *gains, R.HALF_SBS))
    assert {k: v for k, v in out["zlib"].items() if k != "frames_dir"} == {k: v for k, v in out["gpu"].items() if k != "frames_dir"}


def test_flag_and_validation_on_all_four_clis(clips, capsys):
    from video_3d_pipeline import convert, depth, pipeline, upscale
    from video_3d_pipeline.png_gpu import PNG_ENCODERS, check_png_encoder
    assert PNG_ENCODERS == ("zlib", "gpu") and check_png_encoder("gpu") == "gpu"
    for main, argv in ((depth.main, ["x.npy"]), (upscale.main, ["d", "v.npy"]), (pipeline.main, ["x.npy", "v.npy"]), (convert.main, ["v.npy", "d"])):
        with pytest.raises(SystemExit):
            main(argv + ["--png-encoder", "lz4"])
        assert "--png-encoder" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            main(["--help"])
        assert "--png-encoder {zlib,gpu}" in capsys.readouterr().out
    for make in (lambda: depth.HybridStereoDepthExtractor(work_dir=str(clips / "v"), cache_dir=str(clips / "v"), backend=OracleStereoBackend(), png_encoder="GPU"),
                 lambda: upscale.SimpleDepthUpscaler(backend=OracleUpscaleBackend(), png_encoder=None),
                 lambda: pipeline.SbsTo4kDepthPipeline(work_dir=str(clips / "v"), backend=RefStereoPipelineBackend(), png_encoder="png"),
                 lambda: convert.DepthTo3DConverter(backend=RefRenderBackend(), png_encoder=1)):
        with pytest.raises(ValueError, match="png_encoder"):
            make()
    # the flag reaches the constructors
    rc = depth.main([str(clips / "sbs.npy"), "--work-dir", str(clips / "w"), "--stereo-only", "--device", "cpu", "--png-encoder", "gpu"])
    assert rc == 1 and "MI355X" in capsys.readouterr().out          # parsed, then refused for the device: no GPU needed here


def test_device_encoder_slices_the_batch_into_its_streams():
    """png_gpu.DevicePngEncoder's own host logic (buffer sizes, offsets D2H, one copy of the used bytes, per-frame views ended by
    utils.png_stream_end) over stand-ins for torch's device side and for the native call, which leaves png_ref.batch's bytes --
    including the 128-wide one-row gray frame whose stream ends 15 bytes before its slot does"""
    import contextlib
    import types
    import torch
    from video_3d_pipeline.png_gpu import DevicePngEncoder

    class HostTorch:
        uint8, int64 = torch.uint8, torch.int64

        @staticmethod
        def empty(*a, pin_memory=False, device=None, **k):
            return torch.empty(*a, **k)

        class cuda:
            device = staticmethod(lambda d: contextlib.nullcontext())
            current_stream = staticmethod(lambda: types.SimpleNamespace(synchronize=lambda: None))

    class RefNative:
        PNG_GRAY16, PNG_BGR8, PNG_MAX_WIDTH, PNG_MAX_HEIGHT = 0, 1, 8192, 65535
        calls = 0

        @staticmethod
        def lib():
            return types.SimpleNamespace(v3d_png_out_bytes=P.out_bytes, v3d_png_ws_bytes=lambda *a: 64)

        @classmethod
        def png_deflate_batch(cls, frames, out, offsets, ws):
            cls.calls += 1
            fmt = P.GRAY16 if frames.dim() == 3 else P.BGR8
            o, off, _ = P.batch([f.numpy().view(np.uint16) if fmt == P.GRAY16 else f.numpy() for f in frames], fmt)
            out[:] = 0xEE                                            # a reused buffer holds the last batch's bytes
            out[:o.size] = torch.from_numpy(o)
            offsets[:len(off)] = torch.from_numpy(off.astype(np.int64))

    enc = DevicePngEncoder(HostTorch, RefNative, "cpu")
    pads = set()
    for fmt, W, H, n in ((P.GRAY16, 128, 1, 3), (P.BGR8, 85, 4, 2), (P.GRAY16, 253, 5, 4), (P.GRAY16, 128, 1, 1)):
        frames = [P.content_image(fmt, W, H, 5 * W + H + 2 * f) for f in range(n)]
        a = np.stack(frames)
        got = enc.encode(torch.from_numpy(a.view(np.int16) if fmt == P.GRAY16 else a))
        assert len(got) == n
        for g, f in zip(got, frames):
            assert bytes(g) == P.stream(f, fmt)
            pads.add(-len(g) % 16)
    assert RefNative.calls == 4 and 15 in pads
    with pytest.raises(ValueError, match="outside the encoder's range"):
        enc.encode(torch.zeros((1, 2, 8200), dtype=torch.int16))
