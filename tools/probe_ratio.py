"""Compressed sizes with the plane probe on (QZSTD_frontSetPlaneProbe), from the REFERENCE frames (qz_device.reference_frames_probe: the oracle's
sequences, the rule of include/qzstd_planecost.h, libzstd — what the device calls produce byte for byte with the setting on) — no GPU needed.

  sizes()   the figures of tests/golden/probe_sizes.json over tools/delta_ratio.py's inputs (2 MiB of bf16 and of fp32 weights and their XOR
            with the checkpoint before, 128 KiB frames, a block per plane, levels 1 and 6): per cell the total size, the blocks, how many
            of them the library writes raw, the frames it assembles, those that fall back, and "slack", the sum of (len >> 6) + 2 over the
            raw-predicted blocks: what the total may exceed the setting-off total of tests/golden/delta_sizes.json by at the most.
            tests/test_probe_ratio.py holds a fresh run against the file

python tools/probe_ratio.py   prints the JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_ratio as R  # noqa: E402
import qz_bind as B  # noqa: E402
import qz_device as D  # noqa: E402


def sizes(zstd, oracle, lib=None) -> dict:
    out = {}
    for kind, k in R.INPUTS:
        new, base = R.inputs(kind)
        out[kind] = {"bytes": len(new), "elem": k, "step": R.STEP}
        for level in (1, 6):
            cell = {}
            for name, data in (("grouped", new), ("delta", R.xor_bytes(new, base))):
                counts = {}
                total = sum(len(f) for f in D.reference_frames_probe(zstd, oracle, data, 131072, level, k, lib=lib, counts=counts))
                cell[name] = dict(size=total, **{key: counts[key] for key in ("blocks", "raw", "assembled", "fallback", "slack")})
            out[kind]["level%d" % level] = cell
    return out


if __name__ == "__main__":
    print(json.dumps(sizes(B.Zstd(), B.Oracle()), indent=1))
