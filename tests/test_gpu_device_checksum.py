"""GPU: content checksums for frames built from device-resident input (QZSTD_frontSetChecksum, include/qzstd_frontend_device.h).  With the
setting on, the frames of QZSTD_frontCompressDevice and QZSTD_frontCompressDeviceBatch carry the Content_Checksum_Flag, decode (the
decoder verifies the hash the GPU computed) and are byte for byte the frames QZSTD_frontCompress builds from the tensors' host copies with
the setting on.  No tolerance anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B
import qz_corpus as K

torch = D.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 131072


def on_gpu(data: bytes):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")


def tensor_bytes(t) -> bytes:
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


def flagged(frame: bytes) -> bool:
    return frame[:4] == b"\x28\xb5\x2f\xfd" and bool(frame[4] & 4)


def mixed_tensors(seed):
    """tensors of 1 byte .. 1 MiB, of mixed dtypes, every third a view at an odd byte offset of a larger tensor (gathered parts), and
    last one aligned tensor of 2 MiB (whole chunks: a part read in place when it is compressed alone)"""
    sizes = [1, 15, 16, 4097, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 777, 40000, 1 << 20]
    dtypes = [torch.uint8, torch.float16, torch.float32, torch.int64]
    big = on_gpu(K.by_name("system", 300000, seed=seed))
    out = []
    for i, n in enumerate(sizes):
        dt = dtypes[i % 4]
        n -= n % torch.empty(0, dtype=dt).element_size()
        if n == 0:
            dt, n = torch.uint8, sizes[i]
        out.append(on_gpu(K.by_name(("system", "mix", "text")[i % 3], n, seed=seed + i)).view(dt))
        if i % 3 == 0:
            out.append(big[1 + 2 * i:1 + 2 * i + 5000 * (i + 1) + i])
    out.append(on_gpu(K.by_name("system", 2 << 20, seed=seed + 50)))
    return out


def host_frames(front_lib, level, datas, checksum=True, threads=8):
    fr = D.DeviceFront(threads, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(checksum) == 0
        return [fr.compress_host(d) for d in datas]
    finally:
        fr.close()


def check_frames(zstd, got, want, datas, flag=True):
    assert len(got) == len(want) == len(datas)
    for i, (g, w, d) in enumerate(zip(got, want, datas)):
        assert len(g) == len(w) == (len(d) + CHUNK - 1) // CHUNK, i
        for c, f in enumerate(g):
            assert flagged(f) == flag, (i, c)
            assert f == w[c], "tensor %d frame %d differs from QZSTD_frontCompress's" % (i, c)
            assert zstd.decompress(f, CHUNK) == d[c * CHUNK:(c + 1) * CHUNK], (i, c)


@pytest.mark.parametrize("level", [1, 6, 12])
def test_checksummed_frames_equal_the_host_path(front_lib, zstd, level):
    tensors = mixed_tensors(seed=level)
    assert any(t.data_ptr() % 2 for t in tensors) and tensors[-1].data_ptr() % 16 == 0
    datas = [tensor_bytes(t) for t in tensors]
    want = host_frames(front_lib, level, datas)
    n = sum(len(w) for w in want)
    fr = D.DeviceFront(8, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(1) == 0
        check_frames(zstd, D.compress_tensors(fr, tensors), want, datas)  # one gathered part
        st, ck = fr.stats(), fr.checksum_stats()
        assert ck == st[:2] and sum(ck) == n, (st, ck)
        check_frames(zstd, [D.compress_tensor(fr, t) for t in tensors], want, datas)  # the last one: a part read in place
        assert fr.checksum_stats() == fr.stats()[:2] and sum(fr.checksum_stats()) == 2 * n
    finally:
        fr.close()


def test_counters_and_the_setting_turned_off_again(front_lib, zstd):
    """compressible input: every checksum the GPU's, exactly 8 bytes more device->host per frame than the same call without; random
    input moves frames to libzstd's count; off again, the frames are a fresh front's"""
    text = on_gpu(K.by_name("text", 9 * CHUNK + 4321, seed=3))
    rnd = on_gpu(np.random.default_rng(4).integers(0, 256, 3 * CHUNK + 99, dtype=np.uint8).tobytes())
    datas = [tensor_bytes(text), tensor_bytes(rnd)]
    fresh = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    fr = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    try:
        plain = D.compress_tensors(fresh, [text, rnd])
        assert fresh.checksum_stats() == [0, 0]
        s0 = fr.stats()
        off = D.compress_tensor(fr, text)
        s1 = fr.stats()
        assert fr.set_checksum(1) == 0
        on = D.compress_tensor(fr, text)
        s2 = fr.stats()
        assert len(on) == 10 and fr.checksum_stats() == [10, 0] and s2[0] - s1[0] == 10
        assert (s2[2] - s1[2]) - (s1[2] - s0[2]) == 8 * 10, (s0, s1, s2)
        check_frames(zstd, [on], host_frames(front_lib, 1, datas[:1]), datas[:1])
        got = D.compress_tensors(fr, [text, rnd])
        check_frames(zstd, got, host_frames(front_lib, 1, datas), datas)
        ck = fr.checksum_stats()
        assert ck[0] == 20 and ck[1] >= 3 and sum(ck) == 24, ck
        assert fr.set_checksum(0) == 0
        again = D.compress_tensors(fr, [text, rnd])
        assert again == plain and [off] == plain[:1] and not any(flagged(f) for t in again for f in t)
        assert fr.checksum_stats() == ck
    finally:
        fresh.close()
        fr.close()


def test_small_parts_hash_on_both_slots(front_lib):
    """QZSTD_FRONT_DEVICE_PART small (a process of its own): five parts and more, alternating between the two slots, every frame with
    the hash of its own bytes"""
    script = """
import json, sys
sys.path[:0] = [%r, %r]
import qz_device as D, qz_bind as B, qz_corpus as K
import test_gpu_device_checksum as T
z = B.Zstd()
lib = B.Front().lib
tensors = [T.on_gpu(K.by_name("text", 9 * T.CHUNK + 77, seed=1))[0:], T.on_gpu(b"x" + K.by_name("mix", 5 * T.CHUNK + 5, seed=2))[1:],
           T.on_gpu(K.by_name("system", 8 * T.CHUNK, seed=3))]
datas = [T.tensor_bytes(t) for t in tensors]
want = T.host_frames(lib, 1, datas)
fr = D.DeviceFront(8, 1, T.CHUNK, lib=lib)
fr.set_checksum(1)
T.check_frames(z, D.compress_tensors(fr, tensors), want, datas)
T.check_frames(z, [D.compress_tensor(fr, t) for t in tensors], want, datas)
print(json.dumps({"frames": sum(len(w) for w in want), "cksum": fr.checksum_stats()}))
""" % (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=240,
                         env=dict(os.environ, QZSTD_FRONT_DEVICE_PART=str(4 * CHUNK)))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == 24 and sum(res["cksum"]) == 48 and res["cksum"][0] >= 40, res
