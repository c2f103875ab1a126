"""bench.py's plain / --full split and --dump-outputs, without a GPU."""
import numpy as np
import pytest

import bench

torch = pytest.importorskip("torch")


def test_plain_run_drops_the_legs_beside_the_headline():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--solo-batches", "2", "--latency-calls", "9"])
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert a.no_verify and a.no_cpu_baseline
    assert (a.d2h_steps, a.solo_batches, a.latency_calls) == (0, 0, 0)


def test_full_keeps_the_legs_and_their_options():
    a = bench.parse(["--full"])
    assert a.full and not a.no_verify and not a.no_cpu_baseline
    assert (a.d2h_steps, a.solo_batches, a.latency_calls) == (5, 2, 128)
    a = bench.parse(["--full", "--no-verify", "--d2h-steps", "0", "--latency-calls", "16"])
    assert a.no_verify and (a.d2h_steps, a.solo_batches, a.latency_calls) == (0, 2, 16)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


@pytest.mark.parametrize("n", [1, 7, 100])
def test_dump_outputs(tmp_path, n):
    rng = np.random.default_rng(n)
    # shorter than a chunk, a chunk exactly, and longer ones
    sizes = ([5, bench.DUMP_CHUNK, bench.DUMP_CHUNK + 1] + rng.integers(1, 4 * bench.DUMP_CHUNK, n).tolist())[:n]
    segs = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)) for s in sizes]
    out = [tmp_path / "a", tmp_path / "b"]
    for d in out:
        bench.dump_outputs(str(d), segs)
    got = {p.stem: np.load(p) for p in out[0].iterdir()}
    assert sorted(got) == ["byte_sums", "lens", "sample", "sample_offsets", "sample_slots"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for k, v in got.items():  # the same outputs give the same files
        assert np.array_equal(v, np.load(out[1] / f"{k}.npy"))
    assert got["lens"].tolist() == [s.numel() for s in segs]
    assert got["byte_sums"].tolist() == [int(s.sum()) for s in segs]
    slots = got["sample_slots"].astype(int)
    assert set(range(min(n, bench.DUMP_SLOTS))) <= set(slots.tolist()) and slots.max() < n
    for a, i in enumerate(slots):
        s = segs[i].numpy()
        for b, off in enumerate(got["sample_offsets"][a].astype(int)):
            m = min(bench.DUMP_CHUNK, len(s) - off)
            assert np.array_equal(got["sample"][a, b, :m], s[off:off + m].astype(np.float32))
            assert not got["sample"][a, b, m:].any()
        # the first chunk is the head, the second ends with the output's last byte
        assert got["sample_offsets"][a, 0] == 0
        assert got["sample_offsets"][a, 1] + min(bench.DUMP_CHUNK, len(s)) == len(s)
