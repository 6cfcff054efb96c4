"""CPU: what a base buys, from the reference frames (this project's match-finder through the oracle, libzstd's entropy stage): 2 MiB of bf16 and
of fp32 N(0, 0.02) weights after an update drawn from N(0, 1e-5), against the weights before it, 128 KiB frames with a block per plane,
levels 1 and 6.  A fresh run reproduces tests/golden/delta_sizes.json; delta + grouped frames are at most 0.5 x the grouped ones for bf16 and
0.8 x for fp32 (libzstd's own matcher gives 0.13 and 0.62 - 0.63): conditions that keep the feature from being a no-op, not measurements —
the measured values are in the golden file."""
import json
import os

import pytest

import delta_ratio as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "delta_sizes.json")
BOUND = {"bf16": 0.5, "fp32": 0.8}


@pytest.fixture(scope="module")
def fresh(zstd, oracle):
    return R.sizes(zstd, oracle)


def test_a_fresh_run_reproduces_the_stored_sizes(fresh):
    with open(GOLDEN) as f:
        assert fresh == json.load(f)


@pytest.mark.parametrize("level", (1, 6))
@pytest.mark.parametrize("kind", ("bf16", "fp32"))
def test_a_base_pays_on_an_optimiser_sized_step(fresh, kind, level):
    cell = fresh[kind]["level%d" % level]
    print("%s level %d: grouped %d, delta + grouped %d, ratio %.4f" % (kind, level, cell["grouped"], cell["delta"], cell["delta"] / cell["grouped"]))
    assert cell["delta"] <= BOUND[kind] * cell["grouped"], (kind, level, cell)
