"""CPU: compressed size with the plane code on (tools/hufblock_ratio.py): 2 MiB each of bf16 and fp32 weights, their XOR deltas and the seven
integer columns of tools/ediff_ratio.py, grouped, 128 KiB frames, levels 1 and 6.  A fresh run reproduces tests/golden/planecode_sizes.json;
the header's QZSTD_HUF_SEQ_EIGHTHS is the value the sweep chooses; the four float inputs are no larger than with the probe on, no input is
larger than with the probe on by more than (len >> 6) + 2 per taken block; the weights' exponent planes are taken (the feature is not a no-op)
and their frames are smaller; and for the float inputs at level 1 the tool's total is the total of qz_device.reference_frames_code's frames."""
import json
import os

import pytest

import hufblock_ratio as H
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planecode_sizes.json")


@pytest.fixture(scope="module")
def huf(tmp_path_factory):
    return H.hufblock(str(tmp_path_factory.mktemp("hufblock")))


@pytest.fixture(scope="module")
def fresh(zstd, oracle, huf):
    return H.sizes(zstd, oracle, huf)


def test_a_fresh_run_reproduces_the_stored_sizes(fresh):
    with open(GOLDEN) as f:
        assert fresh == json.load(f)


def test_the_header_holds_the_chosen_constant(fresh):
    assert fresh["chosen"] is not None and fresh["header"] == fresh["chosen"]
    assert fresh["sweep"][str(fresh["chosen"])]["ok"]
    assert all(fresh["sweep"][str(fresh["chosen"])]["sum"] <= cell["sum"] for cell in fresh["sweep"].values() if cell["ok"])


def test_the_conditions_hold_and_the_exponent_planes_are_taken(fresh):
    for name, _, _ in H.inputs():
        for level in (1, 6):
            cell = fresh[name]["level%d" % level]
            print("%s level %d: off %d, probe %d, code %d (%.4f of input), %d of %d blocks taken, %d frames without libzstd, %d fell back" % (
                name, level, cell["off"], cell["probe"], cell["code"], cell["code"] / fresh[name]["bytes"], cell["taken"], cell["blocks"],
                cell["nolib"], cell["fallback"]))
            assert cell["code"] <= cell["probe"] + (0 if name in H.FLOATS else cell["slack"]), (name, level, cell)
            if cell["taken"] == 0:
                assert cell["code"] == cell["probe"]
    for name in ("bf16", "fp32"):
        for level in (1, 6):
            cell = fresh[name]["level%d" % level]
            assert cell["taken"] == 16 and cell["nolib"] == 16 and cell["code"] < cell["probe"], (name, level, cell)


@pytest.mark.parametrize("name", H.FLOATS)
def test_the_totals_are_the_reference_frames(fresh, zstd, oracle, huf, name):
    k, data = next((k, d) for n, k, d in H.inputs() if n == name)
    counts = {}
    frames = D.reference_frames_code(zstd, oracle, huf, data, H.CHUNK, 1, k, counts=counts)
    cell = fresh[name]["level1"]
    assert sum(len(f) for f in frames) == cell["code"]
    assert (counts["taken"], counts["nolib"], counts["code_fallback"]) == (cell["taken"], cell["nolib"], cell["fallback"])
    assert all(D.ungroup_bytes(zstd.decompress(f, H.CHUNK), k) == data[c * H.CHUNK:(c + 1) * H.CHUNK] for c, f in enumerate(frames))
