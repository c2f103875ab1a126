"""Fixed Huffman tables (jpge_set_huffman), the parts that need no GPU:

- tests/_fixedhuff.py, the GPU tests' source of expected bytes, is pinned to the reference:
  fed the per-image optimal tables it reproduces _oracle.encode byte for byte;
- jpge_standard_huffman is ITU T.81 Annex K as libjpeg carries it (a committed fixture, and
  Pillow's own DHT segments where Pillow imports);
- the spec validation and the canonical code assignment, in a stand-alone host program
  (tests/cpp/test_huffspec.cpp), plain and under AddressSanitizer + UBSan.
"""
import io
import os
import subprocess

import numpy as np
import pytest

import _fixedhuff as F
import _oracle
import jpgenc_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the helper reproduces the reference when given the reference's tables ----
def test_helper_reproduces_oracle_420_from_histograms():
    # the tables from the oracle's histograms through the host table builder
    for seed, (w, h), q in ((1, (96, 64), 90), (2, (40, 24), 50), (3, (17, 9), 90)):
        rgb = J.synth_rgb8(seed, w, h)
        specs = F.optimal_specs(rgb, q)
        want = _oracle.encode(rgb, q)
        assert F.dht_specs(want) == specs
        assert F.expected_rgb(rgb, q, specs) == want


@pytest.mark.parametrize("mode,restart", [(444, 0), (420, 3), (420, 1), (422, 0), (411, 5), (444, 2)])
def test_helper_reproduces_oracle_modes_and_restart(mode, restart):
    # (the oracle's histogram stage is 4:2:0 without restart intervals: here the tables
    # are read back from the oracle's own DHT segments, which pins the scan: coefficients,
    # MCU order, DC chains, symbols, canonical codes, fill, stuffing and RSTn)
    rgb = np.random.default_rng(mode + restart).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    want = _oracle.encode(rgb, 75, restart=restart, subsampling=mode)
    specs = F.dht_specs(want)
    assert all(s is not None for s in specs)
    assert F.expected_rgb(rgb, 75, specs, mode, restart) == want


def test_helper_reproduces_gray_reference():
    import _gray
    for restart in (0, 3):
        b = _gray.built("random", 17, 9, 90, restart)
        specs = F.dht_specs(b.jpg)
        assert specs[2] is None and specs[3] is None
        assert F.expected_gray(_gray.plane("random", 17, 9), _oracle.quality_tables(90)[0], specs, restart) == b.jpg


def test_canonical_codes_match_the_table_builder():
    rgb = J.synth_rgb8(4, 64, 48)
    counts, first = _oracle.stage_hist(rgb, 90)
    for t in range(4):
        bits, hv, code, ln = J.huffman_table(counts[t], first[t].astype(np.uint64))
        assert F.canonical((bits.tolist(), hv)) == {s: (int(code[s]), int(ln[s])) for s in hv}


# ---- Annex K ----
def test_standard_tables_equal_the_fixture():
    golden = F.golden_specs()
    assert [list(map(len, g)) for g in golden] == [[16, 12], [16, 162], [16, 12], [16, 162]]
    assert golden[0][0] == [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert golden[1][0] == [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
    for t in range(4):
        bits, vals = J.standard_huffman(t)
        assert (bits, vals) == (golden[t][0], golden[t][1]), t
    for bad in (-1, 4):
        with pytest.raises(J.JpgeError):
            J.standard_huffman(bad)


def test_standard_tables_equal_pillow():
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(J.synth_rgb8(1, 32, 32)).save(buf, "JPEG", quality=75, optimize=False)
    # (libjpeg may put several tables into one DHT segment: dht_specs walks them)
    assert F.dht_specs(buf.getvalue()) == [J.standard_huffman(t) for t in range(4)]


def test_standard_tables_are_complete_prefix_codes():
    for t in range(4):
        codes = F.canonical(J.standard_huffman(t))
        need = set(range(12)) if t % 2 == 0 else {0x00, 0xF0} | {(r << 4) | s for r in range(16) for s in range(1, 11)}
        assert set(codes) == need
        words = sorted(format(c, "0%db" % ln) for c, ln in codes.values())
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))
        assert not any(set(w) == {"1"} for w in words)


def test_engineered_tables_of_the_gpu_tests_are_what_they_claim():
    std = [J.standard_huffman(t) for t in range(4)]
    for t in range(4):
        bits, vals = F.long_code_spec(std[t])
        assert sum(bits[:14]) == 0 and sorted(vals) == sorted(std[t][1])
        codes = F.canonical((bits, vals))
        assert codes[std[t][1][0]][1] == 16  # Annex K's shortest code's symbol: now 16 bits
        pb, pv = F.permuted_spec(std[t])
        assert pb == std[t][0] and pv != std[t][1] and sorted(pv) == sorted(std[t][1])


# ---- validation and code assignment: the stand-alone host program ----
CASES = ("annexk_valid", "annexk_codes", "reject_incomplete_ac", "reject_dc_without_11", "reject_repeated_symbol",
         "reject_kraft_full", "accept_kraft_below_full", "reject_over_256_symbols", "reject_unknown_mode",
         "reject_custom_null", "reject_dc_in_ac_slot", "accept_16_bit_codes", "random_specs")


@pytest.fixture(scope="module")
def huffspec_plain():
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_huffspec")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES)
def test_spec_validation(huffspec_plain, case):
    rc, out = huffspec_plain
    assert f"ok {case}" in out.splitlines(), out[-2000:]
    assert rc == 0 and out.rstrip().endswith(f"{len(CASES)} cases, 0 failed"), out[-2000:]


def test_spec_validation_sanitized():
    # built as the other sanitized host programs are (make asan's flags), this one target only
    exe = os.path.join("tests", "cpp", "bin", "asan", "test_huffspec")
    r = subprocess.run(["make", "-s", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, exe)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and f"{len(CASES)} cases, 0 failed" in out, out[-4000:]
