"""Fixed Huffman tables on the GPU (jpge_set_huffman: ITU T.81 Annex K or the caller's
tables).  In a fixed mode the statistics kernel runs its instance without histograms
(stats_wave_kernel<kN, kGray, false>), no frame waits on the host between its kernels, and
the stream is the coefficients coded with the given tables.  The expected bytes come from
tests/_fixedhuff.py, which test_fixedhuff_cpu.py pins to the reference; everything here is
byte-exact.  The default mode must be untouched by any of it (the mode-switching test)."""
import io

import numpy as np
import pytest

import _adversarial as A
import _fixedhuff as F
import _formats
import _gray
import _oracle
import _yuv
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

OPT, STD, CUSTOM = J.JPGE_HUFF_OPTIMAL, J.JPGE_HUFF_STANDARD, J.JPGE_HUFF_CUSTOM


@pytest.fixture(scope="module")
def std():
    return [J.standard_huffman(t) for t in range(4)]


@pytest.fixture(scope="module")
def long_specs(std):
    """Every symbol on a 15- or 16-bit code, the ones Annex K codes shortest on 16 bits."""
    return [F.long_code_spec(s) for s in std]


@pytest.fixture(scope="module")
def enc():
    """This module's own context (default lanes), left in the optimal mode by every test."""
    e = J.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lone():
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


class fixed:
    """with fixed(enc, mode, specs, ...): the setting, and the defaults again afterwards."""

    def __init__(self, enc, mode, specs=None, sub=420, restart=0, fmt=J.JPGE_FMT_RGB8):
        self.enc, self.args = enc, (mode, specs, sub, restart, fmt)

    def __enter__(self):
        mode, specs, sub, restart, fmt = self.args
        self.enc.set_huffman(mode, specs)
        self.enc.set_subsampling(sub)
        self.enc.set_restart(restart)
        self.enc.set_input_format(fmt)
        return self.enc

    def __exit__(self, *exc):
        self.enc.set_huffman(OPT)
        self.enc.set_subsampling(420)
        self.enc.set_restart(0)
        self.enc.set_input_format(J.JPGE_FMT_RGB8)


# ---- Annex K, byte-exact ----
# 256x256: 1536 blocks = 12 entropy tiles, several statistics and code workgroups and a
# placement scan across them; 17x9: edge replication; 8x8 and 16x16: one MCU
@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("w,h", [(8, 8), (16, 16), (17, 9), (96, 64), (256, 256)])
def test_standard_matches_helper(enc, std, w, h, q):
    rgb = J.synth_rgb8(100 + w, w, h)
    with fixed(enc, STD):
        got = enc.encode(rgb, quality=q)
    assert got == F.expected_rgb(rgb, q, std)
    assert F.dht_specs(got) == std
    assert got != _oracle.encode(rgb, q)


@pytest.mark.parametrize("mode", [420, 444, 422, 411, 4200, 4201])
def test_standard_every_subsampling_mode(enc, std, mode):
    rgb = np.random.default_rng(mode).integers(0, 256, (40, 72, 3), dtype=np.uint8)
    with fixed(enc, STD, sub=mode):
        got = enc.encode(rgb, quality=75)
        batch = enc.encode_batch([rgb, rgb[::-1].copy()], quality=75)
    assert got == F.expected_rgb(rgb, 75, std, mode)
    assert batch[0] == got and batch[1] == F.expected_rgb(rgb[::-1].copy(), 75, std, mode)


@pytest.mark.parametrize("restart", [1, 3, 6])  # (6: one MCU row of 96x64)
def test_standard_restart_intervals(enc, std, restart):
    rgb = J.synth_rgb8(31, 96, 64)
    with fixed(enc, STD, restart=restart):
        got = enc.encode(rgb, quality=90)
        batch = enc.encode_batch([rgb] * 3, quality=90)
    want = F.expected_rgb(rgb, 90, std, 420, restart)
    assert got == want and batch == [want] * 3


@pytest.mark.parametrize("w,h", [(17, 9), (256, 256)])
def test_standard_gray(enc, std, w, h):
    # (the one-component instance without histograms; two DHT segments)
    plane = _gray.plane("photo", w, h, seed=3)
    qy = _oracle.quality_tables(90)[0]
    with fixed(enc, STD, fmt=J.JPGE_FMT_GRAY8):
        got = enc.encode(plane, quality=90)
        batch = enc.encode_batch([plane] * 5, quality=90)
    want = F.expected_gray(plane, qy, std)
    assert got == want and batch == [want] * 5
    assert F.dht_specs(got) == [std[0], std[1], None, None]


def test_standard_gray_restart(enc, std):
    plane = _gray.plane("random", 96, 64, seed=5)
    with fixed(enc, STD, fmt=J.JPGE_FMT_GRAY8, restart=7):
        got = enc.encode(plane, quality=75)
    assert got == F.expected_gray(plane, _oracle.quality_tables(75)[0], std, 7)


@pytest.mark.parametrize("fmt", [J.JPGE_FMT_BGRA8, J.JPGE_FMT_RGB8_PLANAR])
def test_standard_rgb_layouts(enc, std, fmt):
    rgb = J.synth_rgb8(41, 96, 64)
    with fixed(enc, STD, fmt=fmt):
        got = enc.encode(_formats.to_format(rgb, fmt), quality=90)
    assert got == F.expected_rgb(rgb, 90, std)


def test_standard_nv12(enc, std):
    w, h, q = 96, 64, 90
    y, cb, cr = _yuv.samples(_yuv.NV12, 6, w, h)
    coef = _yuv.want_coeffs(_yuv.pad_planes(_yuv.NV12, y, cb, cr), 420, q)
    qy, qc = _oracle.quality_tables(q)
    with fixed(enc, STD, fmt=_yuv.NV12):
        got = enc.encode(_yuv.build(_yuv.NV12, y, cb, cr), quality=q)
    assert got == F.expected_coeffs(*coef, w, h, qy, qc, std)


# ---- the caller's tables ----
@pytest.mark.parametrize("name", ["F1", "F2a", "F2b", "F3"])
def test_custom_long_codes_on_long_record_frames(enc, long_specs, name):
    """15- and 16-bit codes on the frequent symbols of the frames built for long records:
    the longest-code path of the code kernel and the heaviest 0xFF stuffing (a 16-bit code
    plus 6 extra bits per record: four adjacent records pass 64 bits everywhere)."""
    f = A.GRAY_FRAMES[name]()
    with fixed(enc, CUSTOM, long_specs, fmt=J.JPGE_FMT_GRAY8):
        got = enc.encode(f.plane, qy=f.qy)
        assert enc.huffman() == (CUSTOM, long_specs)
    assert got == F.expected_gray(f.plane, f.qy, long_specs)


def test_custom_long_codes_three_components(enc, long_specs):
    f = A.f4()
    with fixed(enc, CUSTOM, long_specs, sub=444, fmt=J.JPGE_FMT_YUV444_PLANAR):
        got = enc.encode(f.frame, qy=f.qy, qc=f.qc)
    assert got == F.expected_yuv444(f.planes, f.qy, f.qc, long_specs)


def test_custom_permutation_of_annex_k(enc, std):
    specs = [F.permuted_spec(s, seed=7 + t) for t, s in enumerate(std)]
    rgb = J.synth_rgb8(51, 96, 64)
    with fixed(enc, CUSTOM, specs):
        got = enc.encode(rgb, quality=90)
    with fixed(enc, STD):
        plain = enc.encode(rgb, quality=90)
    assert got == F.expected_rgb(rgb, 90, specs)
    assert got != plain and F.dht_specs(got) == specs


def test_set_huffman_rejects_through_the_c_abi(enc, std):
    ac_short = (std[1][0][:15] + [std[1][0][15] - 1], std[1][1][:-1])  # one run/size pair missing
    dup = (std[0][0], std[0][1][:-1] + [std[0][1][0]])
    full = ([0, 0, 4, 8] + [0] * 12, std[0][1])  # Kraft sum exactly 2^16
    for bad in ([std[0], ac_short, std[2], std[3]], [dup, std[1], std[2], std[3]], [full, std[1], std[2], std[3]],
                [std[1], std[1], std[2], std[3]]):
        with pytest.raises(J.JpgeError):
            enc.set_huffman(CUSTOM, bad)
    for mode, specs in ((3, std), (-1, None), (CUSTOM, None)):
        with pytest.raises(J.JpgeError):
            enc.set_huffman(mode, specs)
    assert enc.huffman() == (OPT, None)  # (a refused setting changes nothing)
    enc.set_huffman(STD, None)
    assert enc.huffman() == (STD, std)
    enc.set_huffman(OPT)


# ---- the single-image path: K1, K2, code and pack queued at once ----
@pytest.mark.parametrize("w,h", [(96, 64), (256, 256)])
def test_single_image_one_lane(lone, std, w, h):
    import torch

    rgb = J.synth_rgb8(61 + w, w, h)
    want = F.expected_rgb(rgb, 90, std)
    d_in = torch.from_numpy(rgb.reshape(-1)).cuda()
    cap = J.max_jpeg_bytes(w, h)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    with fixed(lone, STD):
        for _ in range(3):
            out.fill_(0xA5)
            torch.cuda.synchronize()
            n = lone.encode_ptr(d_in.data_ptr(), w, h, w * 3, out.data_ptr(), cap, quality=90)
            assert out[:n].cpu().numpy().tobytes() == want  # (torch's stream, no synchronisation)
        for _ in range(3):
            assert lone.encode(rgb, quality=90) == want  # host output
        # another quality on the same geometry: the slot's kept headers must not be reused
        assert lone.encode(rgb, quality=50) == F.expected_rgb(rgb, 50, std)
        assert lone.encode(rgb, quality=90) == want
    assert lone.encode(rgb, quality=90) == _oracle.encode(rgb, 90)


def test_single_image_output_too_small(lone, std):
    import torch

    rgb = J.synth_rgb8(5, 320, 240, kind=1)
    d_in = torch.from_numpy(rgb.reshape(-1)).cuda()
    with fixed(lone, STD):
        for cap in (64, 4096):  # the header does not fit; the scan does not fit
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            with pytest.raises(J.JpgeError):
                lone.encode_ptr(d_in.data_ptr(), 320, 240, 320 * 3, out.data_ptr(), cap, quality=100)
        small = J.synth_rgb8(6, 96, 64)
        assert lone.encode(small, quality=90) == F.expected_rgb(small, 90, std)  # the context still works


# ---- the pipeline ----
def test_pipeline_sets_with_a_short_last_set(enc, std):
    # 9 frames of 256x256 on 4 lanes: frame sets of 4, the last one short
    frames = [J.synth_rgb8(200 + i, 256, 256, kind=i % 2) for i in range(9)]
    with fixed(enc, STD):
        lone_outs = [enc.encode(f, quality=90) for f in frames]
        outs = enc.encode_batch(frames, quality=90)
        again = enc.encode_batch(frames[::-1], quality=90)
    assert lone_outs[0] == F.expected_rgb(frames[0], 90, std)
    assert outs == lone_outs and again == lone_outs[::-1]


def test_pipeline_mixed_geometries(enc, std):
    sizes = [(96, 64), (256, 256), (17, 9), (640, 480), (96, 64), (33, 47), (256, 256), (8, 8), (200, 136), (96, 64), (72, 40)]
    frames = [J.synth_rgb8(300 + i, w, h) for i, (w, h) in enumerate(sizes)]
    with fixed(enc, STD):
        lone_outs = [enc.encode(f, quality=75) for f in frames]
        outs = enc.encode_batch(frames, quality=75)
    assert outs == lone_outs
    for i in (0, 2, 5):
        assert outs[i] == F.expected_rgb(frames[i], 75, std)


def test_pipeline_one_lane(lone, std):
    frames = [J.synth_rgb8(400 + i, 256, 256) for i in range(5)]
    with fixed(lone, STD):
        outs = lone.encode_batch(frames, quality=90)
        assert outs == [lone.encode(f, quality=90) for f in frames]
    assert outs[3] == F.expected_rgb(frames[3], 90, std)


def test_group_batch_follows_the_members_setting(std):
    frames = [J.synth_rgb8(500 + i, 96, 64) for i in range(5)]
    with J.Group([0, 0]) as g:
        g.set_huffman(STD)
        outs = g.encode_batch(frames, quality=90)
        with pytest.raises(J.JpgeError):  # stripes share per-image tables
            g.encode_striped(J.synth_rgb8(1, 640, 480), quality=90)
        g.set_huffman(OPT)
        rgb = J.synth_rgb8(2, 640, 480)
        assert g.encode_striped(rgb, quality=90) == _oracle.encode(rgb, 90)
        assert g.encode_batch(frames, quality=90) == [_oracle.encode(f, 90) for f in frames]
    assert outs == [F.expected_rgb(f, 90, std) for f in frames]


# ---- mode switches on one context ----
def test_mode_switching_keeps_every_mode_exact(enc, std, long_specs):
    frames = [J.synth_rgb8(600 + i, 256, 256) for i in range(6)]
    small = J.synth_rgb8(7, 96, 64)
    want_opt = [_oracle.encode(f, 90) for f in frames]
    want_std = [F.expected_rgb(f, 90, std) for f in frames[:2]]
    want_long = F.expected_rgb(small, 90, long_specs)
    try:
        assert enc.encode_batch(frames, quality=90) == want_opt  # optimal: imports and exports carried
        assert enc.encode(small, quality=90) == _oracle.encode(small, 90)
        enc.set_huffman(STD)
        outs = enc.encode_batch(frames, quality=90)
        assert outs[:2] == want_std and enc.encode(frames[1], quality=90) == want_std[1]
        enc.set_huffman(CUSTOM, long_specs)
        assert enc.encode(small, quality=90) == want_long
        assert enc.encode_batch([small] * 6, quality=90) == [want_long] * 6
        enc.set_huffman(OPT)
        assert enc.encode(small, quality=90) == _oracle.encode(small, 90)
        assert enc.encode_batch(frames, quality=90) == want_opt
        enc.set_huffman(STD)
        assert enc.encode(frames[0], quality=90) == want_std[0]
        enc.set_huffman(OPT)
        assert enc.encode(frames[0], quality=90) == want_opt[0]
    finally:
        enc.set_huffman(OPT)


def test_stage_entries_and_timing_in_a_fixed_mode(enc, std):
    rgb = J.synth_rgb8(71, 96, 64)
    counts, first = enc.symbol_stats(rgb, quality=90)
    coef = enc.fdct_quant(rgb, quality=90)
    with fixed(enc, STD):
        c2, f2 = enc.symbol_stats(rgb, quality=90)  # the stage entries: as in the optimal mode
        coef2 = enc.fdct_quant(rgb, quality=90)
        enc.set_timing(1)
        enc.reset_timing()
        enc.encode(rgb, quality=90)
        t = enc.timing()
        enc.set_timing(0)
    assert np.array_equal(counts, c2) and np.array_equal(first, f2)
    assert all(np.array_equal(a, b) for a, b in zip(coef, coef2))
    assert t["frames"] == 1 and t["symbols"] == 0 and t["dc_stats_sum"] > 0


# ---- one large frame: size-independent checks, no Python symbol loop ----
def test_1080p_decodes_to_the_same_coefficients_and_pixels(enc, std):
    rgb = J.synth_rgb8(81, 1920, 1080)
    with fixed(enc, STD):
        jpg = enc.encode(rgb, quality=90)
    opt = enc.encode(rgb, quality=90)
    assert opt == _oracle.encode(rgb, 90) and len(jpg) > len(opt)
    info, y, cb, cr = J.decode_coeffs(jpg)
    wy, wcb, wcr = enc.fdct_quant(rgb, quality=90)
    assert (info.width, info.height) == (1920, 1080)
    assert np.array_equal(y, wy) and np.array_equal(cb, wcb) and np.array_equal(cr, wcr)
    assert F.dht_specs(jpg) == std
    try:
        from PIL import Image
    except ImportError:
        return
    # (the same coefficients and quantisers: the decoded pixels are equal exactly)
    a, b = (np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in (jpg, opt))
    assert np.array_equal(a, b)


# ---- where a fixed mode is refused ----
def test_stripes_and_planes_refuse_a_fixed_mode(lone):
    import torch

    rgb = J.synth_rgb8(9, 640, 480)
    d = torch.from_numpy(rgb.reshape(-1)).cuda()
    planes = [np.ascontiguousarray(rgb[:, :, c], np.float64) for c in range(3)]
    lone.set_huffman(STD)
    try:
        for _ in range(2):
            with pytest.raises(J.JpgeError) as e:
                lone.stripe_transform(d.data_ptr(), 640 * 3, 640, 480, 0, 30, 90)
            assert e.value.status == 1  # JPGE_E_ARG
        with pytest.raises(J.JpgeError) as e:
            lone.encode_planes(*planes, 640, 480, J.JPGE_TO_RGB, 90)
        assert e.value.status == 1
    finally:
        lone.set_huffman(OPT)
    assert len(lone.stripe_transform(d.data_ptr(), 640 * 3, 640, 480, 0, 30, 90)) == 3
    assert lone.encode_planes(*planes, 640, 480, J.JPGE_TO_RGB, 90) == _oracle.encode(rgb, 90)


def test_encode_file_and_cli_follow_the_mode(enc, std, tmp_path):
    import os
    import subprocess

    rgb = J.synth_rgb8(91, 72, 40)
    ppm = tmp_path / "in.ppm"
    ppm.write_bytes(b"P6\n72 40\n255\n" + rgb.tobytes())
    want = F.expected_rgb(rgb, 90, std)
    with fixed(enc, STD):
        enc.encode_file(str(ppm), str(tmp_path / "a.jpg"), quality=90)
        enc.encode_files([str(ppm)] * 3, [str(tmp_path / f"b{i}.jpg") for i in range(3)], quality=90)
    assert (tmp_path / "a.jpg").read_bytes() == want
    assert all((tmp_path / f"b{i}.jpg").read_bytes() == want for i in range(3))
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jpgenc_amd", "bin", "jpgenc")
    for arg, exp in (("standard", want), ("optimal", _oracle.encode(rgb, 90))):
        out = tmp_path / f"cli_{arg}.jpg"
        r = subprocess.run([cli, "-q", "90", "--huffman", arg, str(ppm), str(out)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == exp
