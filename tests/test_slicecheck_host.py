"""CPU: QZSTD_frontFingerprintDeviceSlices, QZSTD_frontCheckDeviceSlices and QZSTD_frontVerifyDeviceSlices (include/qzstd_frontend_device.h)
under the sanitizers — the stand-alone checker tests/slicecheck/slicecheck_check.c, the front-end, qatseqprod.c and the mock device layer
(tests/mock/, mock_hip_fingerprint_pieces.c and mock_hip_ungroup_cmp_pieces.c included) compiled into ONE executable with
-fsanitize=address,undefined and run as a process of its own: random cuttings whose pieces are packed back to front into a heap block of
exactly their size, against the contiguous calls on the contiguous bytes — fingerprint for fingerprint, flag for flag, offset for offset —
with delta skip off and on, a planted byte, several parts, and refusals with nothing counted."""
import os
import subprocess

import qz_bind as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]


def test_standalone_slicecheck_checker_under_asan_ubsan(tmp_path):
    zlib = B.find_libzstd()
    exe = str(tmp_path / "slicecheck_check")
    srcs = [os.path.join(ROOT, "tests", "slicecheck", "slicecheck_check.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
            os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    flags = ["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-DQZ_TEST_HOOKS", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"] + INC
    obj = str(tmp_path / "mock_hip.o")  # (compiled alone, its match-finder renamed: mock_fail_block.c wraps it)
    subprocess.check_call(flags + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs += [obj] + [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c",
                                             "mock_hip_group_xor.c", "mock_hip_diff.c", "mock_fail_block.c", "mock_hip_group_pieces.c",
                                             "mock_hip_pointer_extent.c", "mock_hip_ungroup_cmp.c", "mock_hip_fingerprint.c",
                                             "mock_hip_fingerprint_pieces.c", "mock_hip_ungroup_cmp_pieces.c")]
    subprocess.check_call(flags + ["-o", exe] + srcs + [zlib, "-ldl", "-Wl,-rpath," + os.path.dirname(zlib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])
