"""CPU: QZSTD_frontVerifyDeviceBatch (include/qzstd_frontend_device.h) under the sanitizers — the stand-alone checker
tests/verify/verify_check.c, the front-end, qatseqprod.c and the mock device layer (tests/mock/, mock_hip_ungroup_cmp.c included) compiled
into ONE executable with -fsanitize=address,undefined and run as a process of its own: the frame table and the part planning, ZERO rows, the
all-same and the all-different call, and the undecodable frame."""
import os
import subprocess

import qz_bind as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]


def test_standalone_verify_checker_under_asan_ubsan(tmp_path):
    zlib = B.find_libzstd()
    exe = str(tmp_path / "verify_check")
    obj = str(tmp_path / "mock_hip.o")
    flags = ["-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-DQZ_TEST_HOOKS", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-pthread"] + INC
    # mock_hip.c alone with its match-finder renamed, as mock_fail_block.c expects it (see that file)
    subprocess.check_call(["gcc"] + flags + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"),
                                             "-o", obj])
    srcs = [os.path.join(ROOT, "tests", "verify", "verify_check.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
            os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c"), obj]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_hip_ungroup.c",
                                             "mock_fail_block.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_diff.c",
                                             "mock_hip_ungroup_cmp.c")]
    subprocess.check_call(["gcc"] + flags + ["-o", exe] + srcs + [zlib, "-ldl", "-Wl,-rpath," + os.path.dirname(zlib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])
