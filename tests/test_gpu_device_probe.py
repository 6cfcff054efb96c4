"""GPU: the plane probe end to end on the real kernels (QZSTD_frontSetPlaneProbe: include/qzstd_frontend_device.h).  Three small tensors —
bf16 with 4096 elements, bf16 with 65536 + 3 elements, fp32 with 32768 elements, N(0, 0.02) weights — through
QZSTD_frontCompressDeviceBatchTyped with the setting on, at levels 1 and 6, checksums off and on: every frame is byte for byte the CPU
reference's (qz_device.reference_frames_probe: the oracle's sequences, the rule of include/qzstd_planecost.h, libzstd) and decodes to the
grouped content; with the setting off the same tensors give today's frames (qz_device.reference_frames_grouped); a delta call against a base
followed by the delta restore reproduces the tensors; and QZSTD_frontPlaneProbeStats [1] is above zero — the path under test really ran."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
SPEC = (("bf16", 4096, 2), ("bf16", 65536 + 3, 2), ("fp32", 32768, 4))
ELEMS = [k for _, _, k in SPEC]


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def tensors():
    """-> (the tensors, their bases: the same weights a small step earlier, the tensors' bytes, the bases' bytes)"""
    ts, bs = [], []
    for i, (kind, n, k) in enumerate(SPEC):
        raw = np.frombuffer(D.typed_corpus(kind, n * k, 50 + i), dtype=np.uint8)
        step = np.frombuffer(D.typed_corpus(kind, n * k, 70 + i), dtype=np.uint8)
        dt = torch.bfloat16 if kind == "bf16" else torch.float32
        ts.append(torch.from_numpy(raw.copy()).to("cuda:0").view(dt))
        bs.append(torch.from_numpy(step.copy()).to("cuda:0").view(dt))
    return ts, bs, [t.view(torch.uint8).cpu().numpy().tobytes() for t in ts], [b.view(torch.uint8).cpu().numpy().tobytes() for b in bs]


def bufs_of(ts):
    return [(t.data_ptr(), t.numel() * t.element_size()) for t in ts]


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
@pytest.mark.parametrize("level", (1, 6))
def test_probed_frames_equal_the_reference(front_lib, zstd, oracle, tensors, level, checksum):
    ts, bs, datas, bdatas = tensors
    stream = torch.cuda.current_stream().cuda_stream
    counts = {}
    on = [D.reference_frames_probe(zstd, oracle, d, CHUNK, level, k, checksum=checksum, lib=front_lib, counts=counts) for d, k in zip(datas, ELEMS)]
    off = [D.reference_frames_grouped(zstd, oracle, d, CHUNK, level, k, checksum=checksum, lib=front_lib) for d, k in zip(datas, ELEMS)]
    assert counts["raw"] > 0 and counts["assembled"] > 0
    fr = D.DeviceFront(4, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(checksum) == 0
        # off: today's frames, nothing probed
        assert fr.get_plane_probe() == 0
        assert fr.compress_device_batch_typed(bufs_of(ts), ELEMS, stream) == off
        assert fr.plane_probe_stats() == [0, 0, 0, 0]
        # on: the reference's frames
        assert fr.set_plane_probe(True) == 0
        got = fr.compress_device_batch_typed(bufs_of(ts), ELEMS, stream)
        for i, (g, w) in enumerate(zip(got, on)):
            assert g == w, "tensor %d %s: frames differ from the CPU reference's" % (i, SPEC[i])
        for g, d, k in zip(got, datas, ELEMS):
            for c, f in enumerate(g):
                assert bool(f[4] & 4) == checksum
                assert D.ungroup_bytes(zstd.decompress(f, CHUNK), k, front_lib) == d[c * CHUNK:(c + 1) * CHUNK]  # (libzstd verifies a checksum)
        st = fr.plane_probe_stats()
        assert st == [counts["blocks"], counts["raw"], counts["assembled"], counts["fallback"]] and st[1] > 0
        # delta frames against a base, and back
        xored = [(np.frombuffer(d, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes() for d, b in zip(datas, bdatas)]
        dcounts = {}
        want = [D.reference_frames_probe(zstd, oracle, x, CHUNK, level, k, checksum=checksum, lib=front_lib, counts=dcounts) for x, k in zip(xored, ELEMS)]
        frames = fr.compress_device_batch_delta(bufs_of(ts), bufs_of(bs), ELEMS, stream)
        assert frames == want
        assert fr.plane_probe_stats()[1] == st[1] + dcounts["raw"] and dcounts["raw"] > 0
        outs = [torch.zeros_like(t) for t in ts]
        assert fr.restore_batch_delta(frames, bufs_of(outs), bufs_of(bs), ELEMS, stream) == sum(len(x) for x in frames)
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.uint8), t.view(torch.uint8)) for o, t in zip(outs, ts))
        # off again: today's frames
        assert fr.set_plane_probe(False) == 0
        assert fr.compress_device_batch_typed(bufs_of(ts), ELEMS, stream) == off
    finally:
        fr.close()
    assert [t.view(torch.uint8).cpu().numpy().tobytes() for t in ts] == datas  # only read
