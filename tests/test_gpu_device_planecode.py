"""GPU: the plane code end to end on the real kernels (QZSTD_frontSetPlaneCode: include/qzstd_frontend_device.h).  Four small tensors — bf16
with 4096 elements, bf16 with 65536 + 3 elements, fp32 with 32768 elements, N(0, 0.02) weights, and one whose high bytes are bf16's and whose
low bytes are a tiled row (a taken block beside one that is neither taken nor raw: its frame falls back) — through
QZSTD_frontCompressDeviceBatchTyped with the setting on, at levels 1 and 6, checksums off and on: every frame is byte for byte the CPU
reference's (qz_device.reference_frames_code: the oracle's sequences, the probe's rule, include/qzstd_hufblock.h alone, libzstd for the
probe's frames) and decodes to the grouped content; with the setting off the same tensors give today's frames; a delta call against a base a
small step away (a high plane of zero runs) followed by the delta restore and the verify call reproduces the tensors; and
QZSTD_frontPlaneCodeStats [1] and [2] are above zero — the path under test really ran."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 131072
SPEC = (("bf16", 4096, 2), ("bf16", 65536 + 3, 2), ("fp32", 32768, 4), ("mixed", 40000, 2))
ELEMS = [k for _, _, k in SPEC]


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def huf(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hufblock") / "libhufblock.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "hufblock", "hufblock_check.c")])
    return D.bind_hufblock(C.CDLL(so))


def weights(kind, n, seed):
    """n elements as float32 values"""
    raw = np.frombuffer(D.typed_corpus("bf16" if kind == "mixed" else kind, n * (4 if kind == "fp32" else 2), seed), dtype=np.uint8)
    return raw.view(np.float32).copy() if kind == "fp32" else (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bytes(kind, w):
    if kind == "fp32":
        return w.astype(np.float32).tobytes()
    v = (w.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()
    if kind == "mixed":
        v[0::2] = np.arange(len(v) // 2) % 256
    return v.tobytes()


@pytest.fixture(scope="module")
def tensors():
    """-> (the tensors, their bases: the same weights an N(0, 1e-5) step earlier, the tensors' bytes, the bases' bytes)"""
    ts, bs = [], []
    for i, (kind, n, k) in enumerate(SPEC):
        w = weights(kind, n, 50 + i)
        step = np.random.default_rng(70 + i).normal(0.0, 1e-5, n).astype(np.float32)
        dt = torch.float32 if kind == "fp32" else torch.bfloat16
        for arr, out in ((w, ts), (w - step, bs)):
            out.append(torch.from_numpy(np.frombuffer(to_bytes(kind, arr), dtype=np.uint8).copy()).to("cuda:0").view(dt))
    return ts, bs, [t.view(torch.uint8).cpu().numpy().tobytes() for t in ts], [b.view(torch.uint8).cpu().numpy().tobytes() for b in bs]


def bufs_of(ts):
    return [(t.data_ptr(), t.numel() * t.element_size()) for t in ts]


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
@pytest.mark.parametrize("level", (1, 6))
def test_coded_frames_equal_the_reference(front_lib, zstd, oracle, huf, tensors, level, checksum):
    ts, bs, datas, bdatas = tensors
    stream = torch.cuda.current_stream().cuda_stream
    counts = {}
    on = [D.reference_frames_code(zstd, oracle, huf, d, CHUNK, level, k, checksum=checksum, lib=front_lib, counts=counts) for d, k in zip(datas, ELEMS)]
    off = [D.reference_frames_grouped(zstd, oracle, d, CHUNK, level, k, checksum=checksum, lib=front_lib) for d, k in zip(datas, ELEMS)]
    assert counts["taken"] > 0 and counts["nolib"] > 0 and counts["code_fallback"] > 0
    fr = D.DeviceFront(4, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(checksum) == 0
        # off: today's frames, nothing coded
        assert fr.get_plane_code() == 0
        assert fr.compress_device_batch_typed(bufs_of(ts), ELEMS, stream) == off
        assert fr.plane_code_stats() == [0, 0, 0, 0] and fr.plane_probe_stats() == [0, 0, 0, 0]
        # on: the reference's frames
        assert fr.set_plane_code(True) == 0
        got = fr.compress_device_batch_typed(bufs_of(ts), ELEMS, stream)
        for i, (g, w) in enumerate(zip(got, on)):
            assert g == w, "tensor %d %s: frames differ from the CPU reference's" % (i, SPEC[i])
        for g, d, k in zip(got, datas, ELEMS):
            for c, f in enumerate(g):
                assert bool(f[4] & 4) == checksum
                assert D.ungroup_bytes(zstd.decompress(f, CHUNK), k, front_lib) == d[c * CHUNK:(c + 1) * CHUNK]  # (libzstd verifies a checksum)
        st = fr.plane_code_stats()
        assert st == [counts["coded"], counts["taken"], counts["nolib"], counts["code_fallback"]] and st[1] > 0 and st[2] > 0
        assert fr.plane_probe_stats() == [counts["blocks"], counts["raw"], counts["assembled"], counts["fallback"]]
        # delta frames against a base a small step away, and back
        xored = [(np.frombuffer(d, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes() for d, b in zip(datas, bdatas)]
        dcounts = {}
        want = [D.reference_frames_code(zstd, oracle, huf, x, CHUNK, level, k, checksum=checksum, lib=front_lib, counts=dcounts)
                for x, k in zip(xored, ELEMS)]
        frames = fr.compress_device_batch_delta(bufs_of(ts), bufs_of(bs), ELEMS, stream)
        assert frames == want
        assert fr.plane_code_stats() == [st[0] + dcounts["coded"], st[1] + dcounts["taken"], st[2] + dcounts["nolib"], st[3] + dcounts["code_fallback"]]
        outs = [torch.zeros_like(t) for t in ts]
        assert fr.restore_batch_delta(frames, bufs_of(outs), bufs_of(bs), ELEMS, stream) == sum(len(x) for x in frames)
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.uint8), t.view(torch.uint8)) for o, t in zip(outs, ts))
        assert fr.verify(frames, bufs_of(ts), bufs_of(bs), ELEMS) == []
        # off again: today's frames
        assert fr.set_plane_code(False) == 0
        assert fr.compress_device_batch_typed(bufs_of(ts), ELEMS, stream) == off
    finally:
        fr.close()
    assert [t.view(torch.uint8).cpu().numpy().tobytes() for t in ts] == datas  # only read
