"""Compressed sizes of integer columns as they are, byte-grouped, and differenced + byte-grouped (QZSTD_ELEM_DIFF: include/qzstd_elemdiff.h),
from the REFERENCE frames (libzstd's entropy stage over the oracle's sequences — this project's match-finder: what the device calls produce) —
no GPU needed.

  sizes()   the figures of tests/golden/ediff_sizes.json: seven seeded inputs of 2 MiB each, 128 KiB frames, levels 1 and 6
            (tests/test_ediff_ratio.py holds a fresh run against the file)

python tools/ediff_ratio.py   prints the JSON."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qz_bind as B  # noqa: E402
import qz_device as D  # noqa: E402

BYTES = 2 << 20
CHUNK = 131072
INPUTS = (("offsets32", 4), ("timestamps64", 8), ("sorted_ids64", 8), ("csr_cols32", 4), ("walk16", 2), ("arange64", 8), ("zipf_ids32", 4))
ORDERED = ("offsets32", "timestamps64", "walk16")  # diff + grouped must be smaller than grouped for these (tests/test_ediff_ratio.py)


def column(kind: str, k: int, nbytes: int = BYTES, seed: int = 0) -> bytes:
    """the issue's inputs, seeded: Arrow / CSR offsets, event timestamps, sorted keys, CSR column indices, a sampled signal, row ids, and —
    the counter-example — Zipf token ids, which have no order"""
    n = nbytes // k
    rng = np.random.default_rng(1000 + seed)
    if kind == "offsets32":
        x = np.cumsum(rng.integers(5, 41, n))
    elif kind == "timestamps64":
        x = 1_700_000_000_000_000 + np.cumsum(rng.exponential(1000.0, n).astype(np.int64) + 1)
    elif kind == "sorted_ids64":
        x = np.unique(rng.integers(0, 10 ** 9, n + n // 50))[:n]
        assert len(x) == n
    elif kind == "csr_cols32":
        x = np.sort(rng.integers(0, 1 << 20, (n // 64, 64)), axis=1).reshape(-1)
    elif kind == "walk16":
        x = (30000 + np.cumsum(rng.integers(-3, 4, n))) & 0xFFFF
    elif kind == "arange64":
        x = np.arange(n)
    elif kind == "zipf_ids32":
        return D.typed_corpus("ids32", nbytes, seed)
    else:
        raise ValueError(kind)
    return x.astype("<u%d" % k).tobytes()


def total(frames) -> int:
    return sum(len(f) for f in frames)


def sizes(zstd, oracle, lib=None) -> dict:
    out = {}
    for kind, k in INPUTS:
        data = column(kind, k)
        diffed = b"".join(D.elem_diff(data[o:o + CHUNK], k, lib) for o in range(0, len(data), CHUNK))  # per chunk, as the device calls take them
        out[kind] = {"bytes": len(data), "elem": k}
        for level in (1, 6):
            out[kind]["level%d" % level] = {"plain": total(D.reference_frames(zstd, oracle, data, CHUNK, level)),
                                            "grouped": total(D.reference_frames_grouped(zstd, oracle, data, CHUNK, level, k, lib=lib)),
                                            "diff_grouped": total(D.reference_frames_grouped(zstd, oracle, diffed, CHUNK, level, k, lib=lib))}
    return out


if __name__ == "__main__":
    print(json.dumps(sizes(B.Zstd(), B.Oracle()), indent=1))
