"""CPU: the adviser's estimate beside what the frames measure (tools/advise_ratio.py): the seven seeded columns of the element-difference
figures and sorted_ids64 / offsets32 with a share 1/64 .. 1/2 of their elements replaced by uniform values, 2 MiB each, 128 KiB frames.  A
fresh run reproduces tests/golden/advise_sizes.json — P and D from the front-end's export, grouped and differenced + grouped reference
frames at levels 1 and 6.  With QZSTD_EDIFF_ADVISE_MARGIN_SHIFT as the header sets it: (a) no input is advised whose differenced frames
are not smaller at both levels, (b) offsets, timestamps, sorted ids, the walk and the arange are advised and the Zipf ids are not; and the
header's value is the largest shift of {4, 3, 2, 1} for which both hold."""
import json
import os
import re

import pytest

import advise_ratio as A
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "advise_sizes.json")


@pytest.fixture(scope="module")
def fresh(zstd, oracle):
    return A.sizes(zstd, oracle)


def header_shift() -> int:
    with open(os.path.join(ROOT, "include", "qzstd_ediffcost.h")) as f:
        return int(re.search(r"#define QZSTD_EDIFF_ADVISE_MARGIN_SHIFT (\d+)u", f.read()).group(1))


def test_a_fresh_run_reproduces_the_stored_figures(fresh):
    with open(GOLDEN) as f:
        assert fresh == json.load(f)
    assert len(fresh) == 7 + 2 * 6


def test_the_margin_is_the_smallest_that_holds_and_the_library_applies_it(fresh):
    shift = header_shift()
    for name, cell in fresh.items():
        print("%-22s D/P %.3f  advised %d  diff_grouped/grouped level 1 %.3f level 6 %.3f" % (
            name, cell["D"] / max(cell["P"], 1), A.advised(cell, shift), cell["level1"]["diff_grouped"] / cell["level1"]["grouped"],
            cell["level6"]["diff_grouped"] / cell["level6"]["grouped"]))
    assert A.offenders(fresh, shift) == []   # (a) and (b)
    assert A.margin(fresh) == shift and shift in A.SHIFTS
    # the exported rule is the tool's restatement with that shift
    for cell in fresh.values():
        assert D.ediff_advised(cell["P"], cell["D"]) == A.advised(cell, shift)
    for name in A.MUST_ADVISE:
        assert D.ediff_advised(fresh[name]["P"], fresh[name]["D"]), name
    assert not D.ediff_advised(fresh["zipf_ids32"]["P"], fresh["zipf_ids32"]["D"])
