"""CPU: the whole checkpoint cycle (tools/qz_cycle.py: fingerprint, QZSTD_frontCompressDeviceBatchDelta, restore fresh and in place, restore
slices, verify, check — include/qzstd_frontend_device.h) over the mock device layer, at chunk sizes that are NOT 128 KiB and with the
settings together — the mock pair of tests/test_device_fingerprint_mock.py plus tests/mock/mock_hip_plane_cost.c, the first pair with both
the fingerprint and the plane cost.  Chunks 4080 (planes below QZSTD_BYTEGROUP_CUT_MIN), 16400 (a tile and 16 bytes), 100003 (odd: tails
behind the planes of every element size, frames of one buffer at changing addresses mod 16), 300001 and 393216 (frames of several
match-finder blocks, zero frames of several RLE blocks); checksum, plane probe and delta skip off, on, and at 100003 / 393216 in all eight
combinations; levels 1, 6 and 12.  Three chunks per part, so that both slots are used again.  What the front-end computes from the chunk
size on the host — rows, stage offsets, tile sums, plane cuts, zero frames, the harvest of the verify words, slice windows — is what this
module pins: every frame is the reference's, every restored byte and every guard is checked, every comparison is exact."""
import ctypes as C
import os
import subprocess

import pytest

import qz_bind as B
import qz_cycle as Q
import qz_device as D
import test_device_checksum_mock as T
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_cyclemock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_cyclemock.so")


def build_pair(zstd_path, mock_so, front_so):
    """the fingerprint test's mock pair with the plane cost's stand-in: every device entry point of the checkpoint calls"""
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c", "mock_hip_fingerprint.c", "mock_hip_plane_cost.c")]
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def cyclemock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    S.bind_hooks(plug)
    plug.lib.qzstd_mock_ungroup_cmp_zero_rows.restype = C.c_ulonglong
    return plug, F


@pytest.mark.parametrize("case", Q.MATRIX, ids=Q.case_id)
def test_cycle(cyclemock, zstd, oracle, monkeypatch, case):
    plug, F = cyclemock
    chunk, level, (checksum, probe, skip) = case
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    L = plug.lib
    before = (L.qzstd_mock_plane_cost_launches(), L.qzstd_mock_diff_launches(), L.qzstd_mock_ungroup_cmp_zero_rows(), L.qzstd_mock_xxh64_launches())
    n_frames = Q.cycle(F, zstd, oracle, Q.HostMem(plug), chunk, level, checksum, probe, skip)
    after = (L.qzstd_mock_plane_cost_launches(), L.qzstd_mock_diff_launches(), L.qzstd_mock_ungroup_cmp_zero_rows(), L.qzstd_mock_xxh64_launches())
    # the settings reached the device layer: the probe, the comparison, the verify call's ZERO rows and the hash ran exactly when asked for
    assert [a > b for a, b in zip(after, before)] == [probe, skip, skip, checksum] and n_frames == 36
