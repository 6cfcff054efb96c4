"""CPU: the slots a front keeps between device calls, under the sanitizers — the stand-alone checker tests/slots/slots_check.c, the
front-end, qatseqprod.c and the mock device layer (tests/mock/) compiled into ONE executable with -fsanitize=address,undefined and run as a
process of its own with leak detection on: one front serves device 0, device 1 and device 0 again (compress, restore, verify, fingerprint +
check, advise, every setting on), so that both slot families are freed and rebuilt on a change of device and not only by QZSTD_freeFront;
every round's frames, restored bytes and fingerprints equal the first round's, and nothing is leaked."""
import os
import subprocess

import qz_bind as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]


def test_standalone_slots_checker_under_asan_ubsan(tmp_path):
    zlib = B.find_libzstd()
    exe = str(tmp_path / "slots_check")
    srcs = [os.path.join(ROOT, "tests", "slots", "slots_check.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
            os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    flags = ["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-DQZ_TEST_HOOKS", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"] + INC
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip.c", "mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c",
                                             "mock_hip_group_xor.c", "mock_hip_diff.c", "mock_hip_plane_cost.c", "mock_hip_huf_code.c",
                                             "mock_hip_ungroup.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_cmp.c",
                                             "mock_hip_fingerprint.c", "mock_hip_ediff_cost.c")]
    subprocess.check_call(flags + ["-o", exe] + srcs + [zlib, "-ldl", "-Wl,-rpath," + os.path.dirname(zlib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])
