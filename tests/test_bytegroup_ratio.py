"""CPU: what byte grouping buys, from the reference frames (this project's match-finder through the oracle, libzstd's entropy stage): bf16
and fp32 N(0, 0.02) weights and int32 Zipf ids, 2 MiB each, 128 KiB frames, levels 1 and 6.  A fresh run reproduces
tests/golden/bytegroup_sizes.json; grouped frames of the float inputs are at most 0.95 x the ungrouped ones (libzstd's own matcher gives
0.886 and 0.912 at level 1); the ids do not grow."""
import json
import os

import pytest

import bytegroup_ratio as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bytegroup_sizes.json")


@pytest.fixture(scope="module")
def fresh(zstd, oracle):
    return R.sizes(zstd, oracle)


def test_a_fresh_run_reproduces_the_stored_sizes(fresh):
    with open(GOLDEN) as f:
        assert fresh == json.load(f)


@pytest.mark.parametrize("level", (1, 6))
def test_grouping_pays_on_float_weights_and_costs_nothing_on_ids(fresh, level):
    for kind in ("bf16", "fp32", "ids32"):
        cell = fresh[kind]["level%d" % level]
        print("%s level %d: plain %d, grouped %d, ratio %.4f" % (kind, level, cell["plain"], cell["grouped"], cell["grouped"] / cell["plain"]))
    for kind in ("bf16", "fp32"):
        cell = fresh[kind]["level%d" % level]
        assert cell["grouped"] <= 0.95 * cell["plain"], (kind, level, cell)
    cell = fresh["ids32"]["level%d" % level]
    assert cell["grouped"] <= cell["plain"], (level, cell)
