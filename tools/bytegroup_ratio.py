"""Compressed sizes of typed data with and without byte grouping, from the REFERENCE frames (libzstd over the oracle's sequences: what the
device calls produce byte for byte) — no GPU needed.

  sizes()   the figures of tests/golden/bytegroup_sizes.json: bf16 and fp32 N(0, 0.02) weights and int32 Zipf ids, 2 MiB each, 128 KiB frames,
            levels 1 and 6, ungrouped and grouped (tests/test_bytegroup_ratio.py holds a fresh run against the file)
  table()   profiles/device_group_ratio.json: level 1, per data kind and plane size 256 B .. 64 KiB (frame = plane x element size): as is, grouped
            with the blocks every 128 KiB, grouped with a block per plane — where cutting starts to pay (QZSTD_BYTEGROUP_CUT_MIN)

python tools/bytegroup_ratio.py --golden | --table   prints the JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qz_bind as B  # noqa: E402
import qz_device as D  # noqa: E402

GOLDEN_INPUTS = (("bf16", 2), ("fp32", 4), ("ids32", 4))
TABLE_INPUTS = (("bf16", 2), ("fp16", 2), ("fp32", 4), ("ids32", 4), ("ids64", 8))
GOLDEN_BYTES = 2 << 20
TABLE_BYTES = 1 << 19


def total(frames) -> int:
    return sum(len(f) for f in frames)


def sizes(zstd, oracle, lib=None) -> dict:
    out = {}
    for kind, k in GOLDEN_INPUTS:
        data = D.typed_corpus(kind, GOLDEN_BYTES, 0)
        out[kind] = {"bytes": len(data), "elem": k}
        for level in (1, 6):
            out[kind]["level%d" % level] = {"plain": total(D.reference_frames(zstd, oracle, data, 131072, level)),
                                            "grouped": total(D.reference_frames_grouped(zstd, oracle, data, 131072, level, k, lib=lib))}
    return out


def table(zstd, oracle, lib=None) -> dict:
    rows = []
    for kind, k in TABLE_INPUTS:
        data = D.typed_corpus(kind, TABLE_BYTES, 0)
        for plane in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            chunk = plane * k
            ref = lambda cut, kk=k: total(D.reference_frames_grouped(zstd, oracle, data, chunk, 1, kk, lib=lib, cut=cut))  # noqa: E731
            plain = total(D.reference_frames_grouped(zstd, oracle, data, chunk, 1, 1, lib=lib, cut=False))
            rows.append({"data": kind, "elem": k, "frame": chunk, "plane": plane, "as_is": round(plain / len(data), 4),
                         "grouped_128k_blocks": round(ref(False) / len(data), 4), "grouped_block_per_plane": round(ref(True) / len(data), 4)})
    return {"what": "compressed size / input size, level 1, this project's match-finder (the oracle's sequences) + libzstd's entropy stage; "
                    "%d KiB of seeded data per row (tools/bytegroup_ratio.py --table)" % (TABLE_BYTES >> 10),
            "cut_min": 4096, "rows": rows}


if __name__ == "__main__":
    z, o = B.Zstd(), B.Oracle()
    print(json.dumps(table(z, o) if "--table" in sys.argv else sizes(z, o), indent=1))
