"""Compressed sizes of a checkpoint's tensors against the previous checkpoint, from the REFERENCE frames (libzstd over the oracle's sequences:
what the device calls produce byte for byte) — no GPU needed.

  inputs()  2 MiB of bf16 and of fp32 weights: torch.Generator().manual_seed(1), N(0, 0.02) rounded to the dtype (the base), and the same after
            an update drawn from N(0, 1e-5) is added to the rounded weights and the sum rounded again (the new checkpoint)
  sizes()   the figures of tests/golden/delta_sizes.json: 128 KiB frames, a block per plane, levels 1 and 6 — the new checkpoint byte-grouped
            ("grouped": QZSTD_frontCompressDeviceBatchTyped) and its XOR with the base byte-grouped ("delta": QZSTD_frontCompressDeviceBatchDelta);
            tests/test_delta_ratio.py holds a fresh run against the file

python tools/delta_ratio.py   prints the JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qz_bind as B  # noqa: E402
import qz_device as D  # noqa: E402

INPUTS = (("bf16", 2), ("fp32", 4))
BYTES = 2 << 20
STEP = 1e-5


def inputs(kind: str, nbytes: int = BYTES, step: float = STEP, seed: int = 1):
    """-> (the new checkpoint's bytes, the base's bytes)"""
    import torch
    dtype, view = {"bf16": (torch.bfloat16, torch.int16), "fp32": (torch.float32, torch.int32)}[kind]
    g = torch.Generator().manual_seed(seed)
    n = nbytes // torch.empty((), dtype=dtype).element_size()
    base = (torch.randn(n, generator=g) * 0.02).to(dtype)
    new = (base.float() + torch.randn(n, generator=g) * step).to(dtype)
    return new.view(view).numpy().tobytes(), base.view(view).numpy().tobytes()


def xor_bytes(a: bytes, b: bytes) -> bytes:
    return (int.from_bytes(a, "little") ^ int.from_bytes(b, "little")).to_bytes(len(a), "little")


def sizes(zstd, oracle, lib=None) -> dict:
    out = {}
    for kind, k in INPUTS:
        new, base = inputs(kind)
        out[kind] = {"bytes": len(new), "elem": k, "step": STEP}
        for level in (1, 6):
            total = lambda data: sum(len(f) for f in D.reference_frames_grouped(zstd, oracle, data, 131072, level, k, lib=lib))  # noqa: E731
            out[kind]["level%d" % level] = {"grouped": total(new), "delta": total(xor_bytes(new, base))}
    return out


if __name__ == "__main__":
    print(json.dumps(sizes(B.Zstd(), B.Oracle()), indent=1))
