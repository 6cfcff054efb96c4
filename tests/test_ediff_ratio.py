"""CPU: what element differences buy on integer columns, from the reference frames (this project's match-finder through the oracle,
libzstd's entropy stage): seven seeded inputs of 2 MiB each, 128 KiB frames, levels 1 and 6, as they are, byte-grouped, and differenced +
byte-grouped.  A fresh run reproduces tests/golden/ediff_sizes.json; for the offsets, the timestamps and the random walk diff + grouped is
smaller than grouped at both levels — no ratio threshold beyond "smaller": the sizes themselves are what the golden file pins; the Zipf
ids' growth is printed, not asserted away."""
import json
import os

import pytest

import ediff_ratio as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ediff_sizes.json")


@pytest.fixture(scope="module")
def fresh(zstd, oracle):
    return R.sizes(zstd, oracle)


def test_a_fresh_run_reproduces_the_stored_sizes(fresh):
    with open(GOLDEN) as f:
        assert fresh == json.load(f)


@pytest.mark.parametrize("level", (1, 6))
def test_differences_pay_on_ordered_columns(fresh, level):
    for kind, _ in R.INPUTS:
        cell, n = fresh[kind]["level%d" % level], fresh[kind]["bytes"]
        print("%s level %d: plain %.4f, grouped %.4f, diff + grouped %.4f of the input%s" % (
            kind, level, cell["plain"] / n, cell["grouped"] / n, cell["diff_grouped"] / n,
            "  (GROWS: data without order)" if cell["diff_grouped"] > cell["grouped"] else ""))
    for kind in R.ORDERED:
        cell = fresh[kind]["level%d" % level]
        assert cell["diff_grouped"] < cell["grouped"], (kind, level, cell)
