"""CPU: the fingerprint (include/qzstd_fingerprint.h) and the calls that take it on device buffers (QZSTD_frontFingerprintDeviceBatch /
QZSTD_frontCheckDeviceBatch: include/qzstd_frontend_device.h) under the sanitizers — the stand-alone checker tests/fingerprint/fingerprint_check.c,
the front-end, qatseqprod.c and the mock device layer (tests/mock/, mock_hip_fingerprint.c included) compiled into ONE executable with
-fsanitize=address,undefined and run as a process of its own: the definition at the edge lengths, its properties on given inputs, the two
calls on a mixed batch.  And the second specification: tools/qz_device.py's fingerprint_ref, written from the definition's text, equals the
front-end's export QZSTD_fingerprintOf on the checker's inputs and on every changed copy the checker asserts to differ."""
import os
import subprocess

import pytest

import qz_bind as B
import qz_device as D
import test_device_fingerprint_mock as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]


def test_standalone_fingerprint_checker_under_asan_ubsan(tmp_path):
    zlib = B.find_libzstd()
    exe = str(tmp_path / "fingerprint_check")
    obj = str(tmp_path / "mock_hip.o")
    flags = ["-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-DQZ_TEST_HOOKS", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-pthread"] + INC
    # mock_hip.c alone with its match-finder renamed, as mock_fail_block.c expects it (see that file)
    subprocess.check_call(["gcc"] + flags + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"),
                                             "-o", obj])
    srcs = [os.path.join(ROOT, "tests", "fingerprint", "fingerprint_check.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
            os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c"), obj]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_hip_ungroup.c",
                                             "mock_fail_block.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_diff.c",
                                             "mock_hip_fingerprint.c")]
    subprocess.check_call(["gcc"] + flags + ["-o", exe] + srcs + [zlib, "-ldl", "-Wl,-rpath," + os.path.dirname(zlib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])


@pytest.fixture(scope="module")
def front(oracle, zstd):
    """the front-end's export, from the mock pair of tests/test_device_fingerprint_mock.py (plain builds: no sanitized code in this process)"""
    return FM.load(zstd.path)[1]


def test_restatement_equals_the_export_on_the_checkers_inputs(front):
    seen = set()
    for k, n in enumerate(D.FP_LENS):
        data = D.fp_corpus(n, 11 + k)
        v = D.fingerprint_of(data.tobytes(), lib=front)
        assert D.fingerprint_ref(data.tobytes()) == v, n
        seen.add(v)
        for name, d in D.fp_variants(data):
            w = D.fingerprint_of(d.tobytes(), lib=front)
            assert D.fingerprint_ref(d.tobytes()) == w, (n, name)
            assert w != v, (n, name)  # (the pairs the checker asserts under the plain-C function)
    assert len(seen) == len(D.FP_LENS)
    assert D.fingerprint_ref(b"") == D.fingerprint_of(b"", lib=front) == D.fp_fold_ref([], 0)


def test_restatement_on_tiles_and_longer_rows(front):
    """a tile digest is the fingerprint's only ingredient: the fold of the restated tiles is the export at lengths of many tiles too"""
    for n, seed in ((65791, 3), (131072, 4), (131072 + 255, 5)):
        data = D.fp_corpus(n, seed).tobytes()
        tiles = [D.fp_tile_ref(data[o:o + 16384]) for o in range(0, n, 16384)]
        assert len(tiles) == D.fp_tiles(n)
        assert D.fp_fold_ref(tiles, n) == D.fingerprint_of(data, lib=front)
        assert D.fp_fold_ref(tiles, n + 1) != D.fp_fold_ref(tiles, n) and D.fp_fold_ref(tiles[::-1], n) != D.fp_fold_ref(tiles, n)
