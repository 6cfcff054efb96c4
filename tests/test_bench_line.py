"""bench.py's line of record: the LAST stdout line must be one short JSON object with the contract's keys (round-4 verdict: a 20 KB
line came back from the driver as parsed = null).  Shape to match: the reference's one-line report, /root/reference/test/benchmark.c:374-382."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
       "config", "roofline", "cpu_baseline", "vs_cpu_baseline", "details_file")
# round 6: the median pass, the size check on the same bytes and what unchanged callers get ride along (round-5 verdict, "Next round" 1)
EXTRA = ("value_median_pass", "compressed_size_vs_software_same_bytes", "unchanged_callers", "box_ceilings_GBps")
CONFIG = ("workload", "level", "block_bytes", "chunks_per_gpu_per_step", "threads_per_rank", "libzstd", "libzstd_build")
ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms_avg", "algorithmic_bytes_per_launch")
CPU = ("value", "unit", "cores", "kind", "sample")


def canned():
    """the full result object of round 4's run (20 KB, 30 side legs): what slim_line has to cut down"""
    with open(os.path.join(ROOT, "profiles", "r04_bench.json")) as f:
        return json.load(f)


def test_slim_line_has_the_contract_keys_and_fits():
    import bench
    out = canned()
    assert len(json.dumps(out)) > 15000  # the canned object IS the oversized one
    line = bench.slim_line(out, "bench_details.json")
    s = json.dumps(line)
    assert len(s) < 4096 and "\n" not in s
    assert set(TOP) <= set(line) and set(line) <= set(TOP) | set(EXTRA)
    assert line["unchanged_callers"]["MBps"] == out["unchanged_callers"]["value"]
    assert all(k in line["config"] for k in CONFIG)
    assert all(k in line["roofline"] for k in ROOFLINE)
    assert all(k in line["cpu_baseline"] for k in CPU)
    assert line["value"] == out["value"] and line["roofline"]["frac"] == out["roofline"]["frac"]
    assert line["cpu_baseline"]["value"] == out["cpu_baseline"]["value"]
    assert line["vs_cpu_baseline"] == out["vs_cpu_baseline"]
    assert json.loads(s) == line  # a round trip through the text the driver sees


def test_slim_line_survives_long_strings_and_missing_cpu_legs():
    import bench
    out = canned()
    out["config"]["workload"] = "w" * 5000
    out["config"]["libzstd_build"] = "b" * 5000
    out["cpu_baseline"]["sample"] = "s" * 5000
    out["data"] = "d" * 5000
    assert len(json.dumps(bench.slim_line(out, "x.json"))) < 4096
    out.pop("cpu_baseline")
    out.pop("vs_cpu_baseline")
    line = bench.slim_line(out, None)  # --no-cpu / N > 1
    assert line["cpu_baseline"] is None and line["vs_cpu_baseline"] is None


def test_slim_line_sheds_optional_keys_instead_of_failing(monkeypatch):
    """round-5 ADVICE: a line that would not fit must not end a finished run without its line of record — the optional keys go, the
    contract's keys stay"""
    import bench
    out = canned()
    out["box_ceilings"] = {"h2d": {"GBps_median": 50.0}, "d2h": {"GBps_median": 50.0}}
    monkeypatch.setattr(bench, "SLIM_LINE_MAX", 1500)
    line = bench.slim_line(out, "bench_details.json")
    assert len(json.dumps(line)) < 1500
    assert set(TOP) <= set(line)
    assert line["value"] == out["value"] and line["roofline"]["frac"] == out["roofline"]["frac"]
    assert line["cpu_baseline"]["value"] == out["cpu_baseline"]["value"]
    assert "box_ceilings_GBps" not in line


def test_plain_run_line_keeps_the_contract_keys_without_the_side_legs():
    """a plain run (no --full) times `value` and nothing else: its line still carries every contract key, `roofline` and `cpu_baseline`
    null, and the headline keys as measured"""
    import bench
    out = {k: v for k, v in canned().items() if k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                                      "scaling", "vs_baseline", "dtype", "data", "config", "e2e")}
    line = bench.slim_line(out, "bench_details.json")
    s = json.dumps(line)
    assert len(s) < 4096 and json.loads(s) == line
    assert set(TOP) <= set(line) and set(line) <= set(TOP) | set(EXTRA)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["vs_cpu_baseline"] is None
    assert all(k in line["config"] for k in CONFIG)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] == out[k], k


def test_side_legs_need_full(monkeypatch):
    """--full is off by default: `bench.py --gpus 1 --steps N --warmup W` is a plain run"""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and not a.no_cpu and not a.kernel_only and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu"])
    a = bench.parse()
    assert a.full and a.no_cpu


def test_write_details_names_a_file(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    os.mkdir(tmp_path / "gpurun_out")
    name = bench.write_details({"a": 1})
    assert name == "bench_details.json"
    assert json.load(open(tmp_path / "bench_details.json")) == {"a": 1}
    assert json.load(open(tmp_path / "gpurun_out" / "bench_details.json")) == {"a": 1}


def test_dump_outputs_writes_a_fixed_sample_within_its_budget(tmp_path, monkeypatch):
    """--dump-outputs: the last step's arrays as float32 / float64 .npy files, a seeded sample of chunks and blocks (the same one every
    run), at most 64 MB in all"""
    import ctypes as C

    import numpy as np
    import torch

    import bench
    pick = bench.dump_sample(8192, bench.DUMP_BLOCKS)
    assert np.array_equal(pick, bench.dump_sample(8192, bench.DUMP_BLOCKS)) and len(set(pick.tolist())) == bench.DUMP_BLOCKS
    assert list(pick) == sorted(pick) and bench.dump_sample(5, 16).tolist() == [0, 1, 2, 3, 4]
    # the samples shrink instead of going over the budget: 3/8 of it for the frames, 3/8 for the sequences
    seq_bytes = (131072 // 3 + 1 + 131072 // 1024 + 1) * 4 * 8
    assert bench.dump_count(bench.DUMP_BLOCKS, seq_bytes) == bench.DUMP_BLOCKS  # 128 KiB blocks: the whole sample fits
    assert bench.dump_count(16, 8 * 1000 * 1000) == 3 and bench.dump_count(16, 10 ** 9) == 1
    assert bench.DUMP_BLOCKS * seq_bytes + bench.DUMP_FRAMES * (131072 + 1024) * 4 <= bench.DUMP_MAX_BYTES * 3 // 4

    # the kernel's results: a count per block (0xFFFFFFFF = error) and `stride` entries of 4 words per block
    nb, stride = 64, 8
    seqs = torch.arange(nb * stride * 4, dtype=torch.int32).reshape(-1, 4)
    cnt = torch.tensor([i % (stride + 1) for i in range(nb)], dtype=torch.int32)
    pick = bench.dump_sample(nb, bench.DUMP_BLOCKS)
    cnt[int(pick[0])] = -1
    k = bench.kernel_outputs(cnt, seqs, stride)
    assert k["kernel_counts"].dtype == np.float64 and k["kernel_counts"][pick[0]] == 0xFFFFFFFF
    assert np.array_equal(k["kernel_sample_blocks"], pick)
    want = np.concatenate([seqs[i * stride:i * stride + (0 if i == pick[0] else int(cnt[i]))].numpy() for i in pick])
    assert np.array_equal(k["kernel_sample_sequences"], want.astype(np.float64))

    # the frames: one per chunk, `stride` bytes apart in the destination buffer
    n, fstride = 40, 16
    dst = (C.c_char * (n * fstride)).from_buffer_copy((bytes(range(256)) * 3)[:n * fstride])
    sizes = (C.c_size_t * n)(*[3 + i % 7 for i in range(n)])
    f = bench.frame_outputs(dst, sizes, fstride, n)
    chunks = f["frame_sample_chunks"].astype(int)
    assert np.array_equal(chunks, bench.dump_sample(n, bench.DUMP_FRAMES)) and np.array_equal(f["frame_sizes"], list(sizes))
    assert f["frame_sample_bytes"].dtype == np.float32
    assert bytes(f["frame_sample_bytes"].astype(np.uint8)) == b"".join(dst.raw[c * fstride:c * fstride + sizes[c]] for c in chunks)

    bench.dump_outputs(str(tmp_path / "out"), dict(k, **f))
    for name, v in dict(k, **f).items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype in (np.float32, np.float64) and np.array_equal(got, v), name
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "small"), dict(k, **f))
