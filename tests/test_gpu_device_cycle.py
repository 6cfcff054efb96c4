"""GPU: the whole checkpoint cycle (tools/qz_cycle.py: fingerprint, QZSTD_frontCompressDeviceBatchDelta, restore fresh and in place, restore
slices, verify, check — include/qzstd_frontend_device.h) end to end on the real library and the real kernels, over the matrix of
tests/test_device_cycle_mock.py: chunk sizes 4080, 16400, 100003, 300001 and 393216 — frames that are not 8 tiles of qzstd_ungroup_cmp,
qzstd_diff and qzstd_fingerprint, not one match-finder block, that end inside an element and start at changing addresses mod 16 —,
checksum, plane probe and delta skip off, on, and at 100003 / 393216 in all eight combinations, levels 1, 6 and 12 (the repeat-aware window
parse over grouped and delta content).  Every frame is the CPU reference's (the oracle's sequences, the rule of include/qzstd_planecost.h,
libzstd), every restored byte and every guard byte of one arena tensor is compared with its host shadow, verify and the fingerprint check
name exactly the frames whose bits were flipped.  Three chunks per part; under 8 MiB of buffers per case; every comparison is exact."""
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B
import qz_cycle as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.mark.parametrize("case", Q.MATRIX, ids=Q.case_id)
def test_cycle(front_lib, zstd, oracle, monkeypatch, case):
    chunk, level, (checksum, probe, skip) = case
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    assert Q.cycle(front_lib, zstd, oracle, Q.TorchMem("cuda:0"), chunk, level, checksum, probe, skip, threads=8) == 36
    D.torch.cuda.synchronize()
