"""CPU: compressed size with the plane probe on, from the reference frames (tools/probe_ratio.py) over tools/delta_ratio.py's inputs: grouped
and delta, bf16 and fp32, levels 1 and 6.  A fresh run reproduces tests/golden/probe_sizes.json.  Against the setting-off sizes of
tests/golden/delta_sizes.json the derived bound holds: a raw-predicted block costs len + 3 where libzstd needed at least
len - (len >> 6) - 2 + 3 for its literals alone, so a total exceeds the setting-off total by at most the sum of (len >> 6) + 2 over the blocks
written raw — and by nothing where no block is."""
import json
import os

import pytest

import probe_ratio as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "probe_sizes.json")
OFF = os.path.join(ROOT, "tests", "golden", "delta_sizes.json")


@pytest.fixture(scope="module")
def fresh(zstd, oracle):
    return P.sizes(zstd, oracle)


def test_a_fresh_run_reproduces_the_stored_sizes(fresh):
    with open(GOLDEN) as f:
        assert fresh == json.load(f)


@pytest.mark.parametrize("what", ("grouped", "delta"))
@pytest.mark.parametrize("level", (1, 6))
@pytest.mark.parametrize("kind", ("bf16", "fp32"))
def test_raw_blocks_cost_at_most_the_minimum_gain_each(fresh, kind, level, what):
    with open(OFF) as f:
        off = json.load(f)[kind]["level%d" % level][what]
    cell = fresh[kind]["level%d" % level][what]
    print("%s level %d %s: off %d, on %d (%+d), %d of %d blocks raw, %d frames assembled, %d fell back, bound +%d" % (
        kind, level, what, off, cell["size"], cell["size"] - off, cell["raw"], cell["blocks"], cell["assembled"], cell["fallback"], cell["slack"]))
    assert cell["size"] <= off + cell["slack"], (kind, level, what, off, cell)
    if cell["raw"] == 0:
        assert cell["size"] == off
    # weights have noise planes, and they are found (the feature is not a no-op here); the XOR of two bf16 checkpoints has none left
    if (kind, what) != ("bf16", "delta"):
        assert cell["raw"] > 0 and cell["assembled"] > 0
