"""Whole files of every Y, Cb, Cr input layout against a stream built on the CPU
(tests/_stream3.py: the oracle's primitives for the coefficients, the DC chains, the four texts
and the per-image tables restated in Python, _fixedhuff's coder for the header and the scan;
pinned to _oracle.encode by test_stream3_cpu.py).  The layouts' own test files (test_gpu_yuv.py,
_yuvxf, _yuv422, _yuv10, the NV12 cases of _downscale, test_chroma_420_against_encode_planes)
compare their encodes with Encoder.encode_planes or a YUV444_PLANAR encode on a second context,
whose statistics, table, code and pack stages are the encoder's own: here no GPU code runs in
the making of an expectation, and encode_planes is itself compared with it on planes that do
not come from an RGB frame, which closes the pin those files rest on.  Every comparison is
exact; a failure names the first differing byte and the part of the file it lies in."""
import numpy as np
import pytest

import _stream3 as S
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def enc():
    e = J.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc1():
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _defaults(enc, enc1):
    yield
    for e in (enc, enc1):
        e.set_downscale(1)
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)


def _check(got: bytes, case: S.Case, what: str = ""):
    assert len(got) <= J.max_jpeg_bytes(*case.size)
    d = S.difference(got, S.built(case).jpg)
    if d:
        pytest.fail(f"{case.name}{what}: {d}")


def _encode(e, case: S.Case) -> bytes:
    qy, qc = S.tables(case)
    S.configure(e, case)
    return e.encode(S.frame(case), qy=qy, qc=qc)


def _batch(e, cases) -> list:
    """jpge_encode_batch of the cases' frames (one layout, one pair of tables)."""
    qy, qc = (np.ascontiguousarray(t, np.uint8) for t in S.tables(cases[0]))
    S.configure(e, cases[0])
    frames, geom = J._as_frames([S.frame(c) for c in cases], cases[0].fmt)
    outs = [np.zeros(J.max_jpeg_bytes(w, h), np.uint8) for w, h, _ in geom]
    arr = (J.Frame * len(frames))()
    for i, (f, o, (w, h, stride)) in enumerate(zip(frames, outs, geom)):
        arr[i].rgb, arr[i].width, arr[i].height, arr[i].stride = f.ctypes.data, w, h, stride
        arr[i].maxval, arr[i].out, arr[i].cap = 255, o.ctypes.data, o.size
    assert J.lib().jpge_encode_batch(e.ctx, arr, len(frames), qy.ctypes.data, qc.ctypes.data, 0) == 0
    return [o[:arr[i].len].tobytes() for i, o in enumerate(outs)]


# ---- 1. the layouts, their modes, restart intervals, transforms, downscale, fixed tables ----
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_whole_file(enc, case):
    _check(_encode(enc, case), case)


# ---- 2. the content frames: category 11, size 10 and 64-symbol blocks in the chroma tables ----
CONTENT = S.CONTENT[S.HALF] + S.CONTENT[S.FULL]


@pytest.mark.parametrize("case", CONTENT, ids=[c.name for c in CONTENT])
@pytest.mark.parametrize("lanes", [4, 1])
def test_content(enc, enc1, lanes, case):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    _check(_encode(e, case), case)


def _sets() -> dict:
    """Five frames of one size, layout and pair of tables each: a set of 4 and a set of 1 form."""
    half = {c.fmt: [x for x in S.CONTENT[S.HALF] if x.fmt == c.fmt] for c in S.CONTENT[S.HALF]}
    out = {S.FMT_NAMES[fmt]: cs + cs[1::-1] for fmt, cs in half.items()}  # checker, edges, noise, edges, checker
    full = {c.kind: c for c in S.CONTENT[S.FULL]}
    out["yuv444"] = [full[k] for k in ("checker", "edges", "F4full", "noise", "F4full")]
    out["yuv444-F4"] = [full["F4"]] * 5  # (its chroma table is not the others')
    return out


@pytest.mark.parametrize("name", list(_sets()))
@pytest.mark.parametrize("lanes", [4, 1])
def test_content_batch(enc, enc1, lanes, name):
    cases = _sets()[name]
    assert len(cases) == 5 and len({(c.fmt, c.size) for c in cases}) == 1
    outs = _batch(enc if lanes == 4 else enc1, cases)
    for i, c in enumerate(cases):
        _check(outs[i], c, f" (frame {i} of the batch)")


# ---- 3. encode_planes itself ----
@pytest.mark.parametrize("case", S.PLANES, ids=[c.name for c in S.PLANES])
def test_encode_planes(enc1, case):
    enc1.set_restart(case.restart)
    _check(enc1.encode_planes(*S.planes(case), *case.size, J.JPGE_TO_YCBCR, case.quality), case, " through encode_planes")
    _check(_encode(enc1, case), case)
