"""The engineered frames of _adversarial.py have the properties they are built for: every
check recomputes what the frame really contains from the oracle (_gray.build, _gray.hist,
_oracle.huffman, orc_stage_hist, orc_stage_coeffs_mode) and the record model stated in
_adversarial.py.  test_gpu_adversarial.py encodes the same frames on the GPU."""
import numpy as np
import pytest

import _adversarial as A
import _gray as G
import _oracle

ZRL, EOB = 0xF0, 0x00


# ---- F1, F1': four long records side by side ----
@pytest.mark.parametrize("name", ["F1", "F1'"])
def test_long_groups(name):
    b = A.built(name)
    m = A.gray_metrics(b)
    print(name, m)
    assert m.block_long_run >= 7  # a whole 4-record group of >= 17-bit records, wherever groups start
    assert m.widest4 > 64
    ac = A.lengths(b.ac_text)
    assert 16 in ac.values()
    # the rare blocks are where they were put, and hold the eight (r, 6) symbols
    for g in A.GRAY_FRAMES[name]().meta["rare"]:
        assert [s for s, _, _ in b.blocks[g][1:]] == [(r << 4) | 6 for r in range(8)] + [EOB], g
        assert all(ac[(r << 4) | 6] + 6 >= A.LONG for r in range(8))


def test_long_groups_sizes():
    assert A.f1().size == (400, 400) and A.f1p().size == (400, 400)
    assert A.f1().meta["rare"] == (1250,) and A.f1p().meta["rare"] == (0, 127, 2499)


# ---- F2: blocks of 128 records ----
@pytest.mark.parametrize("restart", [0, 1, 7, 5000])
@pytest.mark.parametrize("name,size,blocks", [("F2a", (1024, 16), 256), ("F2b", (1032, 24), 387)])
def test_full_blocks(name, size, blocks, restart):
    assert A.GRAY_FRAMES[name]().size == size
    b = A.built(name, restart)
    assert len(b.blocks) == blocks
    for g, blk in enumerate(b.blocks):
        assert len(blk) == 64, g  # DC + 63 AC: no EOB, no ZRL
        assert blk[0][0] >= 7 and blk[0][1] >= 7, g  # the DC category
        assert all(s >> 4 == 0 and s & 15 >= 7 and n == s & 15 for s, n, _ in blk[1:]), g
    assert EOB not in b.ac_text
    m = A.gray_metrics(b)
    print(name, restart, m)
    assert m.max_records == 128 and m.full_blocks == blocks


# ---- F3: zero runs across the 16-position parts ----
def _positions(blk):
    """zig-zag positions of a block's non-zero AC values, its ZRL count, whether it ends in EOB"""
    pos, p, zrl = [], 0, 0
    for s, _, _ in blk[1:]:
        if s == ZRL:
            p += 16
            zrl += 1
        elif s != EOB:
            p += (s >> 4) + 1
            pos.append(p)
    return tuple(pos), zrl, blk[-1][0] == EOB and len(blk) > 1


def test_run_sweep():
    f, b = A.f3(), A.built("F3")
    assert f.size == (520, 256) and len(b.blocks) == 2080
    support = f.meta["support"]
    assert sum(len(s) == 2 for s in support) == 1953 and sum(len(s) == 1 for s in support) == 63
    runs, zrls, ends = set(), set(), set()
    for g, blk in enumerate(b.blocks):
        pos, zrl, eob = _positions(blk)
        assert pos == support[g], g  # rle_block on the oracle's coefficients gives back the block's positions
        assert eob == (not pos or pos[-1] != 63), g
        zrls.add(zrl)
        ends.add(eob)
        runs.update(q - p - 1 for p, q in zip((0,) + pos, pos))
    assert runs == set(range(63))  # every run length, 15, 16, 31, 32, 47, 48 and 62 among them
    assert zrls == {0, 1, 2, 3} and ends == {True, False}
    syms = set(b.ac_text)
    assert ZRL in syms and any(s >> 4 == 15 and s & 15 for s in syms) and any(s >> 4 == 14 for s in syms)
    assert {s & 15 for s in syms if s not in (ZRL, EOB)} == {1, 2, 3}
    assert len(set(b.dc_text)) >= 6  # the DC categories vary
    assert any(len(blk) == 64 for blk in b.blocks)  # the block of all 63 positions
    print("F3", A.gray_metrics(b))


# ---- F4: the chroma tables ----
def test_chroma_long_codes():
    f, c = A.f4(), A.chroma("F4")
    assert f.size == (96, 64) and not (f.planes[0] != 128).any()
    assert np.all(f.qc == 2) and np.all(f.qy == 1)
    print("F4", c.metrics)
    assert c.metrics.widest4 > 64 and c.metrics.block_long_run >= 7
    # the long records are the Cr plane's rare block; and the tables hold continuations
    ac = A.lengths(c.ac_text)
    assert [s for s, _, _ in c.cr.blocks[0][1:]] == [(r << 4) | 6 for r in range(8)] + [EOB]
    assert all(ac[(r << 4) | 6] + 6 >= A.LONG for r in range(8))
    assert any(s & 15 >= 7 for s in c.cr.ac_text) and max(c.cr.dc_text) >= 7
    assert len(ac) >= 20


def test_chroma_full_blocks():
    f, c = A.f4full(), A.chroma("F4full")
    assert f.size == (96, 64) and not (f.planes[0] != 128).any()
    print("F4full", c.metrics)
    assert c.metrics.max_records == 128 and c.metrics.full_blocks == 2 * 96
    assert min(c.dc_text) >= 7 and all(s & 15 >= 7 for s in c.ac_text)


def test_chroma_repeated_2x2_is_the_same_chroma():
    """the 4:2:0 leg: each chroma sample repeated 2x2, so S420_m's average of four equal
    values gives the planes back"""
    for f in (A.f4(), A.f4full()):
        for p in f.planes[1:]:
            up = np.repeat(np.repeat(p, 2, 0), 2, 1).astype(np.float64) - 128.0
            assert np.array_equal(_oracle.subsample_mode(up, 420), p.astype(np.float64) - 128.0)


# ---- the gray planes as R = G = B frames ----
def _stage_hist(rgb, qy, qc):
    h, w = rgb.shape[:2]
    counts, first = np.zeros(1024, np.uint32), np.zeros(1024, np.int64)
    _oracle.orc().orc_stage_hist(rgb.ctypes.data, w, h, 255, qy.ctypes.data, qc.ctypes.data, counts.ctypes.data,
                                 first.ctypes.data)
    return counts.reshape(4, 256), first.reshape(4, 256)


def _lengths_of(counts, first):
    """code lengths from a histogram: a text with the same counts and order of first occurrence"""
    present = np.nonzero(counts)[0]
    order = present[np.argsort(first[present], kind="stable")]
    text = list(order) + [s for s in order for _ in range(int(counts[s]) - 1)]
    return A.lengths(text)


@pytest.mark.parametrize("name", ["F1", "F1'", "F2a", "F2b"])
def test_rgb_420_keeps_the_properties(name):
    f = A.GRAY_FRAMES[name]()
    counts, first = _stage_hist(A.rgb(f.plane), f.qy, f.qy)
    want = G.hist(A.built(name))[0]
    assert counts[2].sum() == counts[2][0] and counts[3].sum() == counts[3][EOB]  # no chroma
    if name == "F2b":  # 1032x24 is padded to 1040x32: the blocks of the frame itself are still full
        big = np.array([s & 15 >= 7 for s in range(256)])
        assert counts[1][big].sum() >= want[1].sum() == 63 * 387
        return
    # (whole MCUs, so the same blocks; the colour conversion's Y is not bit for bit the plane,
    # and a few values on a rounding tie move: the properties are checked, not the counts)
    if name == "F2a":
        assert counts[1].sum() == counts[1][0x07] == 63 * 256 and not counts[0][:7].any()
        return
    ac = _lengths_of(counts[1], first[1])
    assert 16 in ac.values() and all(ac[(r << 4) | 6] + 6 >= A.LONG for r in range(8))
    assert all(counts[1][(r << 4) | 6] == len(f.meta["rare"]) for r in range(8))


@pytest.mark.parametrize("name", ["F1", "F1'", "F2a", "F2b"])
def test_rgb_444_keeps_the_blocks(name):
    """At 4:4:4 the Y blocks are the plane's blocks in raster order.  The colour conversion's
    Y is the plane up to 1e-14, which moves a few values that sit exactly on a rounding tie
    (natural positions 0, 4, 32, 36, whose transform is sums and one factor) by one: the
    blocks that carry the property are checked on the oracle's coefficients themselves."""
    f = A.GRAY_FRAMES[name]()
    rgb = A.rgb(f.plane)
    h, w = f.plane.shape
    n = -(-w // 8) * -(-h // 8)
    y, cb, cr = (np.zeros((n, 64), np.int16) for _ in range(3))
    _oracle.orc().orc_stage_coeffs_mode(rgb.ctypes.data, w, h, 255, f.qy.ctypes.data, f.qy.ctypes.data, 444,
                                        y.ctypes.data, cb.ctypes.data, cr.ctypes.data)
    assert not cb.any() and not cr.any()
    gray = A.built(name).coef
    moved = np.argwhere(y != gray)
    assert set(moved[:, 1]) <= {0, 4, 32, 36} and np.abs(y - gray).max() <= 1
    if name.startswith("F2"):  # every block still full, every DC difference still of category >= 7
        assert np.all(np.abs(y[:, 1:]) >= 64) and np.all(np.abs(y[:, 1:]) <= 127)
        d = np.diff(np.concatenate([[0], y[:, 0].astype(np.int64)]))
        assert np.all(np.abs(d) >= 64)
    else:  # the rare blocks as they were; the counts are the 4:2:0 leg's (the same Y blocks in another order)
        rare = list(f.meta["rare"])
        assert np.array_equal(y[rare], gray[rare])
