"""Compressed sizes with the plane code on (QZSTD_frontSetPlaneCode), from the REFERENCE's parts (the oracle's sequences, the rule of
include/qzstd_planecost.h, include/qzstd_hufblock.h alone through tests/hufblock/hufblock_check.c, libzstd for every frame that is not
assembled from raw-predicted and taken blocks alone — what the device calls produce byte for byte) — no GPU needed.

  inputs()  2 MiB each of bf16 and fp32 N(0, 0.02) weights and their XOR with the checkpoint an N(0, 1e-5) step before (tools/delta_ratio.py),
            and the seven integer columns of tools/ediff_ratio.py; byte-grouped, 128 KiB frames, levels 1 and 6
  sizes()   the figures of tests/golden/planecode_sizes.json: per input and level the size with the setting off, with the probe on and with
            the plane code on at QZSTD_HUF_SEQ_EIGHTHS, the blocks taken, the frames assembled without libzstd and those that fell back; and
            "sweep": for every value 16 .. 32 of the constant the summed size over all inputs and levels and whether the conditions hold
            (no float input larger than with the probe on; no input larger than with the probe on by more than (len >> 6) + 2 per taken
            block).  "chosen" is the value with the smallest sum among those that hold — on a tie the one nearest to 24, three bytes a
            sequence, the value the rule started from — and what the header must say (tests/test_planecode_ratio.py)

python tools/hufblock_ratio.py   prints the JSON."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_ratio as R  # noqa: E402
import ediff_ratio as E  # noqa: E402
import qz_bind as B  # noqa: E402
import qz_device as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 131072
SWEEP = tuple(range(16, 33))
FLOATS = ("bf16", "fp32", "bf16 delta", "fp32 delta")


def hufblock(workdir: str | None = None):
    """include/qzstd_hufblock.h alone, built from tests/hufblock/hufblock_check.c"""
    so = os.path.join(workdir or tempfile.mkdtemp(prefix="hufblock"), "libhufblock.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "hufblock", "hufblock_check.c")])
    return D.bind_hufblock(C.CDLL(so))


def inputs():
    """-> [(name, element size, bytes)]"""
    out = []
    for kind, k in R.INPUTS:
        new, base = R.inputs(kind)
        out += [(kind, k, new), (kind + " delta", k, R.xor_bytes(new, base))]
    return out[0::2] + out[1::2] + [(kind, k, E.column(kind, k)) for kind, k in E.INPUTS]


def frames_of(zstd, oracle, huf, data: bytes, level: int, k: int, lib=None) -> list:
    """per frame: (size with the setting off, size with the probe on, bytes of the library's frame header,
    [(len, raw-predicted, size word, body bytes or 0, litBytes, count)] of its blocks)"""
    prof = oracle.profile(level, CHUNK)
    cap = B.sequence_bound(CHUNK)
    out = []
    for o in range(0, len(data), CHUNK):
        piece = data[o:o + CHUNK]
        off = len(D.reference_frames_grouped(zstd, oracle, piece, CHUNK, level, k, lib=lib)[0])
        probe = len(D.reference_frames_probe(zstd, oracle, piece, CHUNK, level, k, lib=lib)[0])
        g = D.group_bytes(piece, k, lib)
        blocks, start = [], 0
        for end in D.group_blocks(len(g), k, lib):
            b = g[start:end]
            n, sq = oracle.find(prof, b, cap=cap)
            lit = sum(s.litLength for s in sq[:n])
            raw = D.plane_is_raw(D.plane_cost(b, lib), len(b), len(b) - lit, lib)
            size, body = (0, 0)
            if not raw and D.HUF_LEN_MIN <= len(b) <= D.HUF_LEN_MAX:
                nbits = (C.c_ubyte * 256)()
                if huf.hb_lengths(b, len(b), nbits):
                    streams = C.create_string_buffer(len(b))
                    size = huf.hb_size_word(huf.hb_streams(b, len(b), nbits, streams, len(b)), len(b))
                    if size:
                        dst = C.create_string_buffer(len(b) + 256)
                        body = huf.hb_body(nbits, len(b), streams.raw[:size], size, dst, len(b) + 256, 0)
            blocks.append((len(b), raw, size, body, lit, n))
            start = end
        out.append((off, probe, len(D.frame_header(len(g))), blocks))
    return out


def at(huf, frames: list, eighths: int) -> dict:
    """the plane code's totals over frames_of()'s frames with the constant at `eighths`"""
    size = taken = nolib = fallback = slack = 0
    for _, probe, head, blocks in frames:
        t = [(not raw) and bool(body) and bool(huf.hb_takes_at(sz, body, n, lit, cnt, eighths)) for n, raw, sz, body, lit, cnt in blocks]
        if any(t) and all(tk or b[1] for tk, b in zip(t, blocks)):
            size += head + sum(3 + (b[0] if b[1] else b[3]) for b in blocks)
            taken += sum(t)
            nolib += 1
            slack += sum((b[0] >> 6) + 2 for tk, b in zip(t, blocks) if tk)
        else:
            size += probe
            fallback += 1 if any(t) else 0
            nolib += 1 if all(b[1] for b in blocks) else 0
    return {"code": size, "taken": taken, "nolib": nolib, "fallback": fallback, "slack": slack}


def sizes(zstd, oracle, huf=None, lib=None) -> dict:
    huf = huf or hufblock()
    const = huf.hb_seq_eighths()
    out, sweep = {}, {e: {"sum": 0, "ok": True} for e in SWEEP}
    for name, k, data in inputs():
        out[name] = {"bytes": len(data), "elem": k}
        for level in (1, 6):
            frames = frames_of(zstd, oracle, huf, data, level, k, lib)
            off, probe = sum(f[0] for f in frames), sum(f[1] for f in frames)
            out[name]["level%d" % level] = dict(off=off, probe=probe, blocks=sum(len(f[3]) for f in frames), **at(huf, frames, const))
            for e in SWEEP:
                cell = at(huf, frames, e)
                sweep[e]["sum"] += cell["code"]
                if cell["code"] > probe + (0 if name in FLOATS else cell["slack"]):
                    sweep[e]["ok"] = False
    good = [e for e in SWEEP if sweep[e]["ok"]]
    out["sweep"] = {str(e): sweep[e] for e in SWEEP}
    out["chosen"] = min(good, key=lambda e: (sweep[e]["sum"], abs(e - 24), e)) if good else None
    out["header"] = const
    return out


if __name__ == "__main__":
    print(json.dumps(sizes(B.Zstd(), B.Oracle()), indent=1))
