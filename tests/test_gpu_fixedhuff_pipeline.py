"""The lane pipeline's switches in a fixed Huffman mode (jpge_set_huffman): forced frame-set
sizes over several lanes, the pipeline-depth switches, a failing member of a set, and one
lane running sets in both modes.  Both Huffman modes run through one lane loop
(Encoder::run_lane, two stage schedules), and these cases hold its fixed-tables schedule to
the bytes of tests/_fixedhuff.py (pinned to the reference by test_fixedhuff_cpu.py), as
test_gpu_sets.py and test_gpu_env_modes.py hold the per-image one to the oracle's.  Small
frames only (96x64, 17x9); everything is byte-exact.  Continues test_gpu_fixedhuff.py."""
import functools
import os

import numpy as np
import pytest

import _fixedhuff as F
import _oracle
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

OPT, STD = J.JPGE_HUFF_OPTIMAL, J.JPGE_HUFF_STANDARD


def _encoder(**env):
    """A context opened under the given JPGE_* switches (they are read when it opens)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return J.Encoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _small_frames(w, h, n):
    """n frames of distinct content with their Annex K and per-image bytes at quality 90,
    computed once for the tests below."""
    std = [J.standard_huffman(t) for t in range(4)]
    frames = [J.synth_rgb8(700 + 16 * w + i, w, h, kind=i % 3) for i in range(n)]
    assert len({f.tobytes() for f in frames}) == n
    return frames, [F.expected_rgb(f, 90, std) for f in frames], [_oracle.encode(f, 90) for f in frames]


@pytest.mark.parametrize("set_size", [1, 2, 3, 4])
def test_pipeline_forced_set_sizes_three_lanes(set_size):
    # 13 frames: a short last set at every size above 1
    frames, want, _ = _small_frames(96, 64, 13)
    enc = _encoder(JPGE_LANES=3, JPGE_SET=set_size)
    try:
        enc.set_huffman(STD)
        assert enc.encode_batch(frames, quality=90) == want
    finally:
        enc.close()


@pytest.mark.parametrize("lookahead", [1, 8])
@pytest.mark.parametrize("drain_lag", [0, 2, 4])
def test_pipeline_depth_switches(drain_lag, lookahead):
    # (the look-ahead has no stage to act on in a fixed mode, but the slot ring is sized from
    # it: every value gives the helper's bytes, so the same ones)
    frames, want, _ = _small_frames(17, 9, 11)
    enc = _encoder(JPGE_LANES=2, JPGE_DRAIN_LAG=drain_lag, JPGE_LOOKAHEAD=lookahead)
    try:
        enc.set_huffman(STD)
        assert enc.encode_batch(frames, quality=90) == want
    finally:
        enc.close()


def test_pipeline_member_errors_stay_with_their_frame():
    # one member in the middle of a set (2 lanes: sets of 4) with a device output buffer that
    # holds the headers but not the scan: that frame reports JPGE_E_NOSPACE and every other
    # frame is exact; the next batch on the context, every capacity sufficient, is exact for
    # every frame (the failed frame's slot gives up the tables it kept)
    import ctypes

    import torch

    frames, want, _ = _small_frames(96, 64, 9)
    frames = [np.ascontiguousarray(f) for f in frames]
    full = J.max_jpeg_bytes(96, 64)
    assert all(len(w) > 700 for w in want)
    enc = _encoder(JPGE_LANES=2)
    try:
        enc.set_huffman(STD)
        qy, qc = J.quality_tables(90)
        for bad in (5, None):
            outs = [torch.zeros(full, dtype=torch.uint8, device="cuda") for _ in frames]
            torch.cuda.synchronize()
            arr = (J.Frame * len(frames))()
            for i, (f, o) in enumerate(zip(frames, outs)):
                arr[i].rgb, arr[i].width, arr[i].height = f.ctypes.data, 96, 64
                arr[i].stride, arr[i].maxval = 96 * 3, 255
                arr[i].out, arr[i].cap = o.data_ptr(), (700 if i == bad else full)
            st = J.lib().jpge_encode_batch(enc._ctx, arr, len(frames), qy.ctypes.data_as(ctypes.c_void_p),
                                           qc.ctypes.data_as(ctypes.c_void_p), J.JPGE_DEVICE_OUTPUT)
            if bad is None:
                assert st == 0
            else:
                assert st == 2 and arr[bad].status == 2  # JPGE_E_NOSPACE
            for i in range(len(frames)):
                if i != bad:
                    assert arr[i].status == 0
                    assert outs[i][:arr[i].len].cpu().numpy().tobytes() == want[i]
    finally:
        enc.close()


def test_one_lane_sets_in_both_modes():
    # the one configuration in which a single lane runs sets; the switches between the modes
    # cross the tables the slots keep in a fixed mode
    frames, want_std, want_opt = _small_frames(96, 64, 10)
    enc = _encoder(JPGE_LANES=1, JPGE_EXT_PLACE=1, JPGE_SET=3)
    try:
        assert enc.encode_batch(frames, quality=90) == want_opt
        enc.set_huffman(STD)
        assert enc.encode_batch(frames, quality=90) == want_std
        enc.set_huffman(OPT)
        assert enc.encode_batch(frames, quality=90) == want_opt
    finally:
        enc.close()
