"""What QZSTD_frontAdviseDeviceBatch estimates beside what the frames really measure: for every input the summed order-0 plane costs
without and with element differences (P, D: include/qzstd_ediffcost.h through the front-end's export — the words the GPU computes), and the
sizes of the byte-grouped and the differenced + byte-grouped REFERENCE frames (libzstd's entropy stage over the oracle's sequences, as
tools/ediff_ratio.py takes them) at levels 1 and 6 — no GPU needed.

  sizes()   the figures of tests/golden/advise_sizes.json: the seven inputs of tools/ediff_ratio.py (2 MiB each, 128 KiB frames), and
            sorted_ids64 and offsets32 with a share q in {1/64 .. 1/2} of their elements replaced by uniform values below the column's maximum
            (positions and values from numpy's default_rng(MIX_SEED + 64 q)): where order fades, the tie must fall on the right side
  margin()  the largest shift in {4, 3, 2, 1} — the smallest margin — under which (a) no input is advised whose diff_grouped >= grouped at
            either level and (b) the ordered inputs are advised and the Zipf ids are not; None when no shift does.  QZSTD_EDIFF_ADVISE_MARGIN_SHIFT
            is that value (tests/test_advise_ratio.py holds both)

python tools/advise_ratio.py   prints the JSON and the margin."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ediff_ratio as E  # noqa: E402
import qz_bind as B  # noqa: E402
import qz_device as D  # noqa: E402

CHUNK = E.CHUNK
MIXED = ("sorted_ids64", "offsets32")
SHARES = (64, 32, 16, 8, 4, 2)  # q = 1 / these
MIX_SEED = 2000
MUST_ADVISE = ("offsets32", "timestamps64", "sorted_ids64", "walk16", "arange64")
MUST_NOT_ADVISE = ("zipf_ids32",)
SHIFTS = (4, 3, 2, 1)


def mixed(kind: str, k: int, inv_q: int) -> bytes:
    """the column with every element replaced, with probability 1 / inv_q, by a uniform value below the column's maximum"""
    x = np.frombuffer(E.column(kind, k), dtype="<u%d" % k).copy()
    rng = np.random.default_rng(MIX_SEED + 64 // inv_q)
    hit = rng.random(len(x)) < 1.0 / inv_q
    x[hit] = rng.integers(0, int(x.max()), int(hit.sum()), dtype=np.uint64).astype(x.dtype)
    return x.tobytes()


def inputs():
    """-> [(name, element size, bytes)]"""
    out = [(kind, k, E.column(kind, k)) for kind, k in E.INPUTS]
    for kind in MIXED:
        k = dict(E.INPUTS)[kind]
        out += [("%s_mix1_%d" % (kind, q), k, mixed(kind, k, q)) for q in SHARES]
    return out


def sizes(zstd, oracle, lib=None) -> dict:
    out = {}
    for name, k, data in inputs():
        diffed = b"".join(D.elem_diff(data[o:o + CHUNK], k, lib) for o in range(0, len(data), CHUNK))
        P, Dd = D.ediff_cost(data, k, CHUNK, lib)
        out[name] = {"bytes": len(data), "elem": k, "P": P, "D": Dd}
        for level in (1, 6):
            out[name]["level%d" % level] = {"grouped": E.total(D.reference_frames_grouped(zstd, oracle, data, CHUNK, level, k, lib=lib)),
                                            "diff_grouped": E.total(D.reference_frames_grouped(zstd, oracle, diffed, CHUNK, level, k, lib=lib))}
    return out


def advised(cell: dict, shift: int) -> bool:
    """the rule of QZSTD_ediffAdvised with this shift"""
    return cell["D"] + (cell["D"] >> shift) < cell["P"]


def offenders(table: dict, shift: int) -> list:
    """the inputs that break (a) or (b) under this shift: [(name, why)]"""
    bad = []
    for name, cell in table.items():
        pays = all(cell["level%d" % lv]["diff_grouped"] < cell["level%d" % lv]["grouped"] for lv in (1, 6))
        if advised(cell, shift) and not pays:
            bad.append((name, "advised, and differenced frames are not smaller at both levels"))
        if name in MUST_ADVISE and not advised(cell, shift):
            bad.append((name, "ordered, and not advised"))
        if name in MUST_NOT_ADVISE and advised(cell, shift):
            bad.append((name, "without order, and advised"))
    return bad


def margin(table: dict):
    for shift in SHIFTS:
        if not offenders(table, shift):
            return shift
    return None


if __name__ == "__main__":
    t = sizes(B.Zstd(), B.Oracle())
    print(json.dumps(t, indent=1))
    for name, cell in t.items():
        print("%-22s D/P %.3f   level 1 %.3f   level 6 %.3f" % (name, cell["D"] / max(cell["P"], 1),
                                                                 cell["level1"]["diff_grouped"] / cell["level1"]["grouped"],
                                                                 cell["level6"]["diff_grouped"] / cell["level6"]["grouped"]), file=sys.stderr)
    for s in SHIFTS:
        print("shift %d: %s" % (s, offenders(t, s) or "holds"), file=sys.stderr)
    print("margin shift: %s" % margin(t), file=sys.stderr)
