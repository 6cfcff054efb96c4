"""ctypes bindings of the front-end's device-resident input (include/qzstd_frontend_device.h: QZSTD_frontCompressDevice,
QZSTD_frontCompressDeviceBatch, QZSTD_frontDeviceStats, QZSTD_frontSetChecksum, QZSTD_frontSetByteGroup, QZSTD_frontCompressDeviceBatchTyped)
and of the way back (QZSTD_frontRestoreDeviceBatchTyped, QZSTD_frontRestoreDevice, QZSTD_frontRestoreStats: DeviceFront.restore_batch),
the delta calls against a base per buffer (QZSTD_frontCompressDeviceBatchDelta, QZSTD_frontRestoreDeviceBatchDelta, QZSTD_frontDeltaStats:
DeviceFront.compress_device_batch_delta / restore_batch_delta), delta skip (QZSTD_frontSetDeltaSkip, QZSTD_frontDeltaSkipStats:
DeviceFront.set_delta_skip / delta_skip_stats; qzstd_hip_diff's row, binding and numpy reference; zero_frame()), the verify call
(QZSTD_frontVerifyDeviceBatch, QZSTD_frontVerifyStats: DeviceFront.verify / verify_stats, verify_tensors(); qzstd_hip_ungroup_cmp's row, binding and
numpy reference ungroup_cmp_ref()), the fingerprint calls (QZSTD_frontFingerprintDeviceBatch, QZSTD_frontCheckDeviceBatch,
QZSTD_frontFingerprintStats: DeviceFront.fingerprint / check / fingerprint_stats, fingerprint_tensors() / check_tensors(); qzstd_hip_fingerprint's
row and binding; fingerprint_ref(), the restatement of include/qzstd_fingerprint.h, and fingerprint_of(), that header's own function),
slices of the written buffers (QZSTD_frontRestoreDeviceSlices,
QZSTD_frontSliceStats: DeviceFront.restore_slices, restore_slices(), shard_slices() and restore_shards() for shards of 2-D tensors),
the plane probe (QZSTD_frontSetPlaneProbe, QZSTD_frontPlaneProbeStats: DeviceFront.set_plane_probe / plane_probe_stats; qzstd_hip_plane_cost's row and
binding; plane_cost() / plane_is_raw(), the rule of include/qzstd_planecost.h; reference_frames_probe(): what the calls must produce with the setting on),
the plane code (QZSTD_frontSetPlaneCode, QZSTD_frontPlaneCodeStats: DeviceFront.set_plane_code / plane_code_stats; qzstd_hip_huf_code's binding over
the plane rows; bind_hufblock() / huf_block(): include/qzstd_hufblock.h alone; reference_frames_code(): what the calls must produce with the setting on),
compress_tensor() for a contiguous GPU tensor of any dtype, compress_tensors() for a list of them in one call (group="dtype": byte-grouped by
each tensor's element size), restore_tensors() for the way back in one call and restore_tensor() for it on the host; the byte-grouped layout itself (include/qzstd_bytegroup.h) as group_bytes /
ungroup_bytes / group_blocks, and reference_frames_grouped(): what the grouped device calls must produce.

Element differences (include/qzstd_elemdiff.h, QZSTD_ELEM_DIFF, QZSTD_frontElemDiffStats): elem_diff / elem_sum, the rows and bindings of
qzstd_hip_group_ediff and qzstd_hip_esum, DeviceFront.elem_diff_stats, and diff= on compress_tensors() / restore_tensors().
The adviser (include/qzstd_ediffcost.h, QZSTD_frontAdviseDeviceBatch, QZSTD_frontAdviseStats): DeviceFront.advise / advise_raw / advise_stats,
advise_tensors(), ediff_cost_of / ediff_cost / ediff_advised (the header's functions through the exports), qzstd_hip_ediff_cost's row and binding.

torch is imported before the library is loaded, so that the process has ONE HIP runtime (the one torch brought)."""
import ctypes as C
import os
import sys

try:
    import torch  # noqa: F401  (first: the HIP runtime the library then binds to)
except ImportError:  # the CPU suite's mock front-end needs no torch
    torch = None

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qz_bind as B  # noqa: E402

ERROR = C.c_size_t(-1).value


class DeviceBuf(C.Structure):
    """QZSTD_DeviceBuf"""
    _fields_ = [("d_ptr", C.c_void_p), ("size", C.c_size_t)]


class GatherRow(C.Structure):
    """qzstd_hip_gather_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("dstOff", C.c_uint64), ("len", C.c_uint32), ("pad", C.c_uint32)]


class GroupRow(C.Structure):
    """qzstd_hip_group_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("dstOff", C.c_uint64), ("len", C.c_uint32), ("pad", C.c_uint32), ("elem", C.c_uint32),
                ("reserved", C.c_uint32)]


class UngroupRow(C.Structure):
    """qzstd_hip_ungroup_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("dst", C.c_uint64), ("srcOff", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32)]


class GroupXorRow(C.Structure):
    """qzstd_hip_group_xor_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("base", C.c_uint64), ("dstOff", C.c_uint64), ("len", C.c_uint32), ("pad", C.c_uint32),
                ("elem", C.c_uint32), ("reserved", C.c_uint32)]


class UngroupXorRow(C.Structure):
    """qzstd_hip_ungroup_xor_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("dst", C.c_uint64), ("base", C.c_uint64), ("srcOff", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32)]


class UngroupWinRow(C.Structure):
    """qzstd_hip_ungroup_win_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("dst", C.c_uint64), ("base", C.c_uint64), ("srcOff", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32),
                ("winOff", C.c_uint32), ("winLen", C.c_uint32), ("tile0", C.c_uint32), ("reserved", C.c_uint32)]


class DiffRow(C.Structure):
    """qzstd_hip_diff_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("a", C.c_uint64), ("b", C.c_uint64), ("len", C.c_uint32), ("tile0", C.c_uint32)]


def bind_diff_kernel(L):
    """qzstd_hip_diff on a loaded device layer (libqatseqprod)"""
    L.qzstd_hip_diff.restype = C.c_int
    L.qzstd_hip_diff.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def diff_flags_ref(pairs):
    """what qzstd_hip_diff must leave in d_flags: per (a, b) — two numpy uint8 arrays of one length — 1 when any byte differs, else 0"""
    import numpy as np
    return np.array([1 if len(a) and not np.array_equal(a, b) else 0 for a, b in pairs], dtype=np.uint32)


def diff_tile0_ref(lens):
    """the tile0 the launcher writes: workgroups (16 KiB tiles) of the rows before each one"""
    out, total = [], 0
    for n in lens:
        out.append(total)
        total += (n + 16383) >> 14
    return out


class FpRow(C.Structure):
    """qzstd_hip_fp_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("len", C.c_uint32), ("tile0", C.c_uint32)]


def bind_fingerprint_kernel(L):
    """qzstd_hip_fingerprint on a loaded device layer (libqatseqprod)"""
    L.qzstd_hip_fingerprint.restype = C.c_int
    L.qzstd_hip_fingerprint.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def fp_tiles(n: int) -> int:
    """QZSTD_HIP_FP_TILES: workgroups of a row = its tile digests (16 KiB each)"""
    return (n + 16383) >> 14


_FP_M = (1 << 64) - 1
_FP_P1, _FP_P2, _FP_P3, _FP_P4, _FP_P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                                          0x27D4EB2F165667C5)  # XXH64's five primes


def _fp_round(acc, x):
    """round(acc, in) = rotl(acc + in * P2, 31) * P1, on numpy uint64 arrays (arithmetic mod 2^64)"""
    import numpy as np
    acc = acc + x * np.uint64(_FP_P2)
    return ((acc << np.uint64(31)) | (acc >> np.uint64(33))) * np.uint64(_FP_P1)


def _fp_merge(h, v):
    """merge(h, v) = (h ^ round(0, v)) * P1 + P4"""
    import numpy as np
    return (h ^ _fp_round(np.zeros_like(v), v)) * np.uint64(_FP_P1) + np.uint64(_FP_P4)


def fp_tile_ref(data) -> int:
    """the tile digest restated (a second specification, written from the definition's text, not from include/qzstd_fingerprint.h): n bytes,
    0 < n <= 16384, as 16-byte little-endian words, bytes at or beyond n read as 0; 256 lanes, lane t from P5 + t * P1 over the words
    t, t + 256, t + 512, t + 768 that start below n — low half, then high half, one round each; the lanes folded by the fixed binary tree
    acc[t] = merge(acc[t], acc[t + s]) for s = 1, 2, ..., 128 and t a multiple of 2 s; the digest is lane 0"""
    import numpy as np
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(raw)
    assert 0 < n <= 16384
    buf = np.zeros(16384, dtype=np.uint8)
    buf[:n] = raw
    halves = buf.view("<u8").astype(np.uint64).reshape(4, 256, 2)  # [k][t] = word t + 256 k: (low, high)
    lanes = np.arange(256, dtype=np.uint64)
    with np.errstate(over="ignore"):
        acc = np.uint64(_FP_P5) + lanes * np.uint64(_FP_P1)
        for k in range(4):
            took = _fp_round(_fp_round(acc, halves[k, :, 0]), halves[k, :, 1])
            acc = np.where(16 * (np.arange(256) + 256 * k) < n, took, acc)
        s = 1
        while s < 256:
            t = np.arange(0, 256, 2 * s)
            acc[t] = _fp_merge(acc[t], acc[t + s])
            s *= 2
    return int(acc[0])


def fp_fold_ref(tiles, n: int) -> int:
    """the row fingerprint from its tile digests: h = P5 + len; h = merge(h, tile) for every tile in order; the final avalanche"""
    rotl = lambda v, r: ((v << r) | (v >> (64 - r))) & _FP_M  # noqa: E731
    h = (_FP_P5 + n) & _FP_M
    for v in tiles:
        h = ((h ^ (rotl(int(v) * _FP_P2 & _FP_M, 31) * _FP_P1 & _FP_M)) * _FP_P1 + _FP_P4) & _FP_M
    h ^= h >> 33
    h = h * _FP_P2 & _FP_M
    h ^= h >> 29
    h = h * _FP_P3 & _FP_M
    return h ^ (h >> 32)


def fingerprint_ref(data) -> int:
    """QZSTD_fingerprint restated: the row cut into 16 KiB tiles from its start, fp_tile_ref of each, fp_fold_ref over them with the length"""
    data = bytes(data)
    return fp_fold_ref([fp_tile_ref(data[o:o + 16384]) for o in range(0, len(data), 16384)], len(data))


FP_LENS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 5)  # the edge lengths of the fingerprint tests


def fp_corpus(n: int, seed: int):
    """the fingerprint tests' input of n bytes (tests/fingerprint/fingerprint_check.c: fill) as a numpy uint8 array: byte i is the low byte
    of a 32-bit mix of i and the seed — the host checker and the GPU tests assert their properties on the SAME bytes"""
    import numpy as np
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed * 2246822519 & 0xFFFFFFFF)
        x ^= x >> np.uint32(15)
        x *= np.uint32(2246822519)
        x ^= x >> np.uint32(13)
    return x.astype(np.uint8)


def fp_variants(data):
    """the pairs the host checker asserts to differ under the plain-C definition, as (name, changed copy of `data`) — one bit in the first
    byte, the last byte and either side of the 4096 and 16384 boundaries, words w and w + 256 swapped (one lane), neighbouring words swapped
    (neighbouring lanes), two tiles swapped, a zero byte appended; only the ones the length allows"""
    import numpy as np
    n, out = len(data), []

    def changed(name, fn):
        d = data.copy()
        fn(d)
        out.append((name, d))

    def flip(at, bit):
        def fn(d):
            d[at] ^= bit
        return fn

    def swap(a, b, ln):
        def fn(d):
            t = d[a:a + ln].copy()
            d[a:a + ln] = d[b:b + ln]
            d[b:b + ln] = t
        return fn

    if n:
        changed("first byte", flip(0, 0x01))
        changed("last byte", flip(n - 1, 0x80))
    for at in (4095, 4096, 16383, 16384):
        if at < n:
            changed("byte %d" % at, flip(at, 0x10))
    if n >= 16 * 260:
        changed("words 3 and 259", swap(48, 16 * 259, 16))
        changed("words 3 and 4", swap(48, 64, 16))
    if n >= 2 * 16384:
        changed("tiles 0 and 1", swap(0, 16384, 16384))
    out.append(("a zero byte appended", np.concatenate([data, np.zeros(1, dtype=np.uint8)])))
    return out


def fingerprint_of(data, lib=None) -> int:
    """QZSTD_fingerprintOf: include/qzstd_fingerprint.h's own function through the front-end library's export"""
    L = lib if lib is not None else B.Front().lib
    L.QZSTD_fingerprintOf.restype = C.c_ulonglong
    L.QZSTD_fingerprintOf.argtypes = [C.c_char_p, C.c_size_t]
    data = bytes(data)
    return L.QZSTD_fingerprintOf(data, len(data))


class PlaneRow(C.Structure):
    """qzstd_hip_plane_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("srcOff", C.c_uint64), ("len", C.c_uint32), ("reserved", C.c_uint32)]


def bind_plane_kernel(L):
    """qzstd_hip_plane_cost on a loaded device layer (libqatseqprod)"""
    L.qzstd_hip_plane_cost.restype = C.c_int
    L.qzstd_hip_plane_cost.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


HUF_LEN_MIN, HUF_LEN_MAX, HUF_LENGTHS_BYTES = 1024, 131072, 128  # include/qzstd_hufblock.h


def huf_row_bytes(n: int) -> int:
    """QZSTD_HIP_HUF_ROW_BYTES: what a row of n bytes can take in the dense area of qzstd_hip_huf_code at the most"""
    return ((n + 15) & ~15) + HUF_LENGTHS_BYTES if HUF_LEN_MIN <= n <= HUF_LEN_MAX else 0


def huf_scratch_bytes(rows: int, dense: int) -> int:
    """QZSTD_HIP_HUF_SCRATCH_BYTES"""
    return (((rows + 1) * 4 + 15) & ~15) + dense


def bind_huf_kernel(L):
    """qzstd_hip_huf_code and qzstd_hip_huf_code_bytes on a loaded device layer (libqatseqprod; rows: PlaneRow)"""
    L.qzstd_hip_huf_code_bytes.restype = C.c_size_t
    L.qzstd_hip_huf_code_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.qzstd_hip_huf_code.restype = C.c_int
    L.qzstd_hip_huf_code.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    return L


def plane_cost(block: bytes, lib=None) -> int:
    """QZSTD_planeCost (include/qzstd_planecost.h, through the front-end library's export) of a block's byte histogram: its order-0 cost in bytes"""
    import numpy as np
    hist = np.bincount(np.frombuffer(block, dtype=np.uint8), minlength=256).astype(np.uint32)
    return _bg(lib).QZSTD_planeCostOf(hist.ctypes.data_as(C.POINTER(C.c_uint)), len(block))


def plane_is_raw(cost: int, n: int, matched: int, lib=None) -> bool:
    """QZSTD_planeIsRaw: the block (n bytes, `matched` of them covered by matches) is predicted to be a Raw_Block"""
    return bool(_bg(lib).QZSTD_planeIsRawOf(cost, n, matched))


class UngroupCmpRow(C.Structure):
    """qzstd_hip_ungroup_cmp_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("ref", C.c_uint64), ("base", C.c_uint64), ("srcOff", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32),
                ("flags", C.c_uint32), ("tile0", C.c_uint32)]


CMP_SAME = 0xFFFFFFFF  # QZSTD_HIP_CMP_SAME: a tile word of a tile that matches
CMP_ZERO = 1           # QZSTD_HIP_CMP_ZERO: flags bit 0
VERIFY_SAME = C.c_size_t(-1).value       # QZSTD_VERIFY_SAME
VERIFY_UNDECODED = C.c_size_t(-2).value  # QZSTD_VERIFY_UNDECODED


def bind_cmp_kernel(L):
    """qzstd_hip_ungroup_cmp on a loaded device layer (libqatseqprod)"""
    L.qzstd_hip_ungroup_cmp.restype = C.c_int
    L.qzstd_hip_ungroup_cmp.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def cmp_tiles(n: int, k: int) -> int:
    """QZSTD_HIP_CMP_TILES: workgroups of a row = its tile words (16 KiB of the ungrouped content each, the tail with the last one)"""
    e = n // k
    return -(-e // (16384 // k)) if e else (1 if n else 0)


def ungroup_cmp_ref(rows):
    """what qzstd_hip_ungroup_cmp must leave in d_tiles: rows = [(staged frame or None for a ZERO row, base or None, ref, elem), ...], the
    three as numpy uint8 arrays of one length -> the tile words of all rows, row after row (numpy uint32): CMP_SAME, or the lowest row
    offset inside the tile at which ungrouped(frame) ^ base differs from ref"""
    import numpy as np
    out = []
    for frame, base, ref, k in rows:
        n = len(ref)
        e = n // k
        if frame is None:
            u = np.zeros(n, dtype=np.uint8)
        else:
            u = np.concatenate([np.ascontiguousarray(frame[:e * k].reshape(k, e).T).reshape(-1), frame[e * k:]]) if e else frame.copy()
        if base is not None:
            u = u ^ base
        tiles = cmp_tiles(n, k)
        words = np.full(tiles, CMP_SAME, dtype=np.uint32)
        for p in np.flatnonzero(u != ref)[::-1]:
            words[min(int(p) >> 14, tiles - 1)] = p
        out.append(words)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


def zero_frame(n: int, checksum: bool = False) -> bytes:
    """THE CANONICAL ZERO FRAME of a chunk of n > 0 bytes (include/qzstd_frontend_device.h, QZSTD_frontSetDeltaSkip), without its checksum
    field: magic, Single_Segment with the smallest Frame_Content_Size field that holds n (Content_Checksum_Flag when `checksum`), RLE blocks
    of the byte 0 every 128 KiB, Last_Block on the final one.  With `checksum` the caller appends XXH64(n zero bytes) & 0xFFFFFFFF, little-endian"""
    code = 0 if n <= 255 else (1 if n <= 65791 else (2 if n <= 0xFFFFFFFF else 3))
    out = bytearray(b"\x28\xb5\x2f\xfd")
    out.append(code << 6 | 0x20 | (4 if checksum else 0))
    out += (n - 256 if code == 1 else n).to_bytes((1, 2, 4, 8)[code], "little")
    left = n
    while left:
        b = min(left, 131072)
        out += (b << 3 | 2 | (1 if b == left else 0)).to_bytes(3, "little") + b"\0"
        left -= b
    return bytes(out)


class DeviceSlice(C.Structure):
    """QZSTD_DeviceSlice (include/qzstd_frontend_device.h)"""
    _fields_ = [("buf", C.c_size_t), ("offset", C.c_size_t), ("size", C.c_size_t), ("d_dst", C.c_void_p), ("d_base", C.c_void_p)]


class DeviceSrcSlice(C.Structure):
    """QZSTD_DeviceSrcSlice (include/qzstd_frontend_device.h)"""
    _fields_ = [("buf", C.c_size_t), ("offset", C.c_size_t), ("size", C.c_size_t), ("d_src", C.c_void_p), ("d_base", C.c_void_p)]


class GroupPiece(C.Structure):
    """qzstd_hip_group_piece_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("base", C.c_uint64), ("off", C.c_uint32), ("len", C.c_uint32)]


class GroupPiecesRow(C.Structure):
    """qzstd_hip_group_pieces_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("dstOff", C.c_uint64), ("len", C.c_uint32), ("pad", C.c_uint32), ("elem", C.c_uint32), ("piece0", C.c_uint32),
                ("nPieces", C.c_uint32), ("reserved", C.c_uint32)]


def bind_pieces_kernel(L):
    """qzstd_hip_group_pieces on a loaded device layer (libqatseqprod, or a mock of it)"""
    L.qzstd_hip_group_pieces.restype = C.c_int
    L.qzstd_hip_group_pieces.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_size_t]
    return L


class FpPiecesRow(C.Structure):
    """qzstd_hip_fp_pieces_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("len", C.c_uint32), ("tile0", C.c_uint32), ("piece0", C.c_uint32), ("nPieces", C.c_uint32)]


class UngroupCmpPiecesRow(C.Structure):
    """qzstd_hip_ungroup_cmp_pieces_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("srcOff", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32), ("flags", C.c_uint32), ("tile0", C.c_uint32),
                ("piece0", C.c_uint32), ("nPieces", C.c_uint32)]


def bind_check_pieces_kernels(L):
    """qzstd_hip_fingerprint_pieces / qzstd_hip_ungroup_cmp_pieces on a loaded device layer (libqatseqprod, or a mock of it)"""
    L.qzstd_hip_fingerprint_pieces.restype = C.c_int
    L.qzstd_hip_fingerprint_pieces.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.qzstd_hip_ungroup_cmp_pieces.restype = C.c_int
    L.qzstd_hip_ungroup_cmp_pieces.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_size_t, C.c_void_p]
    return L


def bind_window_kernel(L):
    """qzstd_hip_ungroup_window on a loaded device layer (libqatseqprod)"""
    L.qzstd_hip_ungroup_window.restype = C.c_int
    L.qzstd_hip_ungroup_window.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def bind_xor_kernels(L):
    """qzstd_hip_group_xor / qzstd_hip_ungroup_xor on a loaded device layer (libqatseqprod)"""
    for fn in (L.qzstd_hip_group_xor, L.qzstd_hip_ungroup_xor):
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


class DeviceOutBuf(C.Structure):
    """QZSTD_DeviceOutBuf"""
    _fields_ = [("d_ptr", C.c_void_p), ("size", C.c_size_t)]


class HashRow(C.Structure):
    """qzstd_hip_hash_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("srcOff", C.c_uint64), ("len", C.c_uint64)]


def bind(F):
    """the front-end's C surface, the device entry points included, on a loaded library"""
    F.QZSTD_createFront.restype = C.c_void_p
    F.QZSTD_createFront.argtypes = [C.POINTER(B.FrontParams)]
    F.QZSTD_frontFrameStride.restype = C.c_size_t
    F.QZSTD_frontFrameStride.argtypes = [C.c_void_p]
    F.QZSTD_frontCompress.restype = C.c_size_t
    F.QZSTD_frontCompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    F.QZSTD_frontCompressDevice.restype = C.c_size_t
    F.QZSTD_frontCompressDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]
    if hasattr(F, "QZSTD_frontCompressDeviceBatch"):  # (absent from an older library: tools/device_bench.py measures one)
        F.QZSTD_frontDeviceBatchFrames.restype = C.c_size_t
        F.QZSTD_frontDeviceBatchFrames.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.c_size_t]
        F.QZSTD_frontCompressDeviceBatch.restype = C.c_size_t
        F.QZSTD_frontCompressDeviceBatch.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    F.QZSTD_frontDeviceStats.restype = None
    F.QZSTD_frontDeviceStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    F.QZSTD_freeFront.argtypes = [C.c_void_p]
    if hasattr(F, "QZSTD_frontSetChecksum"):  # (absent from an older library)
        F.QZSTD_frontSetChecksum.restype = C.c_int
        F.QZSTD_frontSetChecksum.argtypes = [C.c_void_p, C.c_int]
        F.QZSTD_frontGetChecksum.restype = C.c_int
        F.QZSTD_frontGetChecksum.argtypes = [C.c_void_p]
        F.QZSTD_frontChecksumStats.restype = None
        F.QZSTD_frontChecksumStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontSetByteGroup"):  # (absent from an older library)
        F.QZSTD_frontSetByteGroup.restype = C.c_int
        F.QZSTD_frontSetByteGroup.argtypes = [C.c_void_p, C.c_uint]
        F.QZSTD_frontGetByteGroup.restype = C.c_uint
        F.QZSTD_frontGetByteGroup.argtypes = [C.c_void_p]
        F.QZSTD_frontByteGroupStats.restype = None
        F.QZSTD_frontByteGroupStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        F.QZSTD_frontCompressDeviceBatchTyped.restype = C.c_size_t
        F.QZSTD_frontCompressDeviceBatchTyped.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                          C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        bind_bytegroup(F)
    if hasattr(F, "QZSTD_frontRestoreDeviceBatchTyped"):  # (absent from an older library)
        F.QZSTD_frontRestoreDeviceBatchTyped.restype = C.c_size_t
        F.QZSTD_frontRestoreDeviceBatchTyped.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                                                         C.POINTER(DeviceOutBuf), C.c_char_p, C.c_size_t, C.c_void_p]
        F.QZSTD_frontRestoreDevice.restype = C.c_size_t
        F.QZSTD_frontRestoreDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.c_void_p, C.c_size_t,
                                               C.c_void_p]
        F.QZSTD_frontRestoreStats.restype = None
        F.QZSTD_frontRestoreStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        F.QZSTD_frontCompact.restype = C.c_size_t
        F.QZSTD_frontCompact.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t]
    if hasattr(F, "QZSTD_frontCompressDeviceBatchDelta"):  # (absent from an older library)
        F.QZSTD_frontCompressDeviceBatchDelta.restype = C.c_size_t
        F.QZSTD_frontCompressDeviceBatchDelta.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.POINTER(DeviceBuf), C.c_char_p, C.c_size_t, C.c_void_p,
                                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        F.QZSTD_frontRestoreDeviceBatchDelta.restype = C.c_size_t
        F.QZSTD_frontRestoreDeviceBatchDelta.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                                                         C.POINTER(DeviceOutBuf), C.POINTER(DeviceBuf), C.c_char_p, C.c_size_t, C.c_void_p]
        F.QZSTD_frontDeltaStats.restype = None
        F.QZSTD_frontDeltaStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        F.QZSTD_byteXor.restype = None
        F.QZSTD_byteXor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(F, "QZSTD_frontRestoreDeviceSlices"):  # (absent from an older library)
        F.QZSTD_frontRestoreDeviceSlices.restype = C.c_size_t
        F.QZSTD_frontRestoreDeviceSlices.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_size_t),
                                                     C.c_char_p, C.c_size_t, C.POINTER(DeviceSlice), C.c_size_t, C.c_void_p]
        F.QZSTD_frontSliceStats.restype = None
        F.QZSTD_frontSliceStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontCompressDeviceSlices"):  # (absent from an older library)
        F.QZSTD_frontCompressDeviceSlices.restype = C.c_size_t
        F.QZSTD_frontCompressDeviceSlices.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t, C.POINTER(DeviceSrcSlice), C.c_size_t,
                                                      C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        F.QZSTD_frontSrcSliceStats.restype = None
        F.QZSTD_frontSrcSliceStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontSetDeltaSkip"):  # (absent from an older library)
        F.QZSTD_frontSetDeltaSkip.restype = C.c_int
        F.QZSTD_frontSetDeltaSkip.argtypes = [C.c_void_p, C.c_int]
        F.QZSTD_frontGetDeltaSkip.restype = C.c_int
        F.QZSTD_frontGetDeltaSkip.argtypes = [C.c_void_p]
        F.QZSTD_frontDeltaSkipStats.restype = None
        F.QZSTD_frontDeltaSkipStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontSetPlaneCode"):  # (absent from an older library)
        F.QZSTD_frontSetPlaneCode.restype = C.c_int
        F.QZSTD_frontSetPlaneCode.argtypes = [C.c_void_p, C.c_int]
        F.QZSTD_frontGetPlaneCode.restype = C.c_int
        F.QZSTD_frontGetPlaneCode.argtypes = [C.c_void_p]
        F.QZSTD_frontPlaneCodeStats.restype = None
        F.QZSTD_frontPlaneCodeStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        F.QZSTD_hufBlockBodyOf.restype = C.c_size_t
        F.QZSTD_hufBlockBodyOf.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        F.QZSTD_hufTakesOf.restype = C.c_int
        F.QZSTD_hufTakesOf.argtypes = [C.c_uint] * 5
    if hasattr(F, "QZSTD_frontSetPlaneProbe"):  # (absent from an older library)
        F.QZSTD_frontSetPlaneProbe.restype = C.c_int
        F.QZSTD_frontSetPlaneProbe.argtypes = [C.c_void_p, C.c_int]
        F.QZSTD_frontGetPlaneProbe.restype = C.c_int
        F.QZSTD_frontGetPlaneProbe.argtypes = [C.c_void_p]
        F.QZSTD_frontPlaneProbeStats.restype = None
        F.QZSTD_frontPlaneProbeStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontVerifyDeviceBatch"):  # (absent from an older library)
        F.QZSTD_frontVerifyDeviceBatch.restype = C.c_size_t
        F.QZSTD_frontVerifyDeviceBatch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(DeviceBuf),
                                                   C.POINTER(DeviceBuf), C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
        F.QZSTD_frontVerifyStats.restype = None
        F.QZSTD_frontVerifyStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontFingerprintDeviceBatch"):  # (absent from an older library)
        F.QZSTD_fingerprintOf.restype = C.c_ulonglong
        F.QZSTD_fingerprintOf.argtypes = [C.c_char_p, C.c_size_t]
        F.QZSTD_frontFingerprintDeviceBatch.restype = C.c_size_t
        F.QZSTD_frontFingerprintDeviceBatch.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.c_size_t, C.c_void_p, C.POINTER(C.c_ulonglong),
                                                        C.POINTER(C.c_size_t)]
        F.QZSTD_frontCheckDeviceBatch.restype = C.c_size_t
        F.QZSTD_frontCheckDeviceBatch.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.c_size_t, C.c_void_p, C.POINTER(C.c_ulonglong), C.c_size_t,
                                                  C.c_void_p]
        F.QZSTD_frontFingerprintStats.restype = None
        F.QZSTD_frontFingerprintStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontFingerprintDeviceSlices"):  # (absent from an older library)
        F.QZSTD_frontFingerprintDeviceSlices.restype = C.c_size_t
        F.QZSTD_frontFingerprintDeviceSlices.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(DeviceSrcSlice), C.c_size_t, C.c_void_p,
                                                         C.POINTER(C.c_ulonglong), C.POINTER(C.c_size_t)]
        F.QZSTD_frontCheckDeviceSlices.restype = C.c_size_t
        F.QZSTD_frontCheckDeviceSlices.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(DeviceSrcSlice), C.c_size_t, C.c_void_p,
                                                   C.POINTER(C.c_ulonglong), C.c_size_t, C.c_void_p]
        F.QZSTD_frontVerifyDeviceSlices.restype = C.c_size_t
        F.QZSTD_frontVerifyDeviceSlices.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_size_t),
                                                    C.c_char_p, C.c_size_t, C.POINTER(DeviceSrcSlice), C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
        F.QZSTD_frontSliceCheckStats.restype = None
        F.QZSTD_frontSliceCheckStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontElemDiffStats"):  # (absent from an older library)
        F.QZSTD_frontElemDiffStats.restype = None
        F.QZSTD_frontElemDiffStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    if hasattr(F, "QZSTD_frontAdviseDeviceBatch"):  # (absent from an older library)
        F.QZSTD_frontAdviseDeviceBatch.restype = C.c_size_t
        F.QZSTD_frontAdviseDeviceBatch.argtypes = [C.c_void_p, C.POINTER(DeviceBuf), C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.POINTER(C.c_ulonglong)]
        F.QZSTD_frontAdviseStats.restype = None
        F.QZSTD_frontAdviseStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        F.QZSTD_ediffCostOf.restype = None
        F.QZSTD_ediffCostOf.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.POINTER(C.c_ulonglong)]
        F.QZSTD_ediffAdvisedOf.restype = C.c_int
        F.QZSTD_ediffAdvisedOf.argtypes = [C.c_ulonglong, C.c_ulonglong]
    return F


def bind_bytegroup(L):
    """include/qzstd_bytegroup.h on a loaded library (libqzstdfront, or qzstd_bytegroup.c built alone)"""
    for fn in (L.QZSTD_byteGroup, L.QZSTD_byteUngroup):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint]
    L.QZSTD_byteGroupBlocks.restype = C.c_size_t
    L.QZSTD_byteGroupBlocks.argtypes = [C.c_size_t, C.c_uint, C.POINTER(C.c_size_t), C.c_size_t]
    if hasattr(L, "QZSTD_planeCostOf"):  # (absent from an older library, and from qzstd_bytegroup.c built alone)
        L.QZSTD_planeCostOf.restype = C.c_uint
        L.QZSTD_planeCostOf.argtypes = [C.POINTER(C.c_uint), C.c_uint]
        L.QZSTD_planeIsRawOf.restype = C.c_int
        L.QZSTD_planeIsRawOf.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    return L


_bytegroup_lib = None


def _bg(lib):
    global _bytegroup_lib
    if lib is not None:
        return lib
    if _bytegroup_lib is None:
        _bytegroup_lib = bind_bytegroup(B.Front().lib)
    return _bytegroup_lib


def _regroup(fn, data: bytes, k: int) -> bytes:
    src = C.create_string_buffer(bytes(data), max(len(data), 1))
    dst = C.create_string_buffer(max(len(data), 1))
    if fn(dst, src, len(data), k) != len(data):
        raise ValueError("element size %r: 1, 2, 4 or 8" % (k,))
    return dst.raw[:len(data)]


def group_bytes(data: bytes, k: int, lib=None) -> bytes:
    """QZSTD_byteGroup: one frame's bytes in the byte-grouped layout for element size k"""
    return _regroup(_bg(lib).QZSTD_byteGroup, data, k)


def ungroup_bytes(data: bytes, k: int, lib=None) -> bytes:
    """QZSTD_byteUngroup: the inverse of group_bytes"""
    return _regroup(_bg(lib).QZSTD_byteUngroup, data, k)


class GroupEdiffRow(C.Structure):
    """qzstd_hip_group_ediff_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("dstOff", C.c_uint64), ("len", C.c_uint32), ("pad", C.c_uint32), ("elem", C.c_uint32),
                ("flags", C.c_uint32)]


class EsumRow(C.Structure):
    """qzstd_hip_esum_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("dst", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32), ("tile0", C.c_uint32), ("reserved", C.c_uint32)]


EDIFF_DIFF = 1  # QZSTD_HIP_EDIFF_DIFF


def bind_ediff_kernels(L):
    """qzstd_hip_group_ediff and qzstd_hip_esum on a loaded device layer (libqatseqprod)"""
    L.qzstd_hip_group_ediff.restype = C.c_int
    L.qzstd_hip_group_ediff.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    L.qzstd_hip_esum.restype = C.c_int
    L.qzstd_hip_esum.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def esum_tiles(n: int, k: int) -> int:
    """QZSTD_HIP_ESUM_TILES: 16 KiB tiles of a row's n // k elements"""
    return (n // k + 16384 // k - 1) // (16384 // k)


def esum_scratch_bytes(tiles: int) -> int:
    """QZSTD_HIP_ESUM_SCRATCH_BYTES"""
    return tiles * 24


class EdiffCostRow(C.Structure):
    """qzstd_hip_ediff_cost_row_t (include/qzstd_hip_device.h)"""
    _fields_ = [("src", C.c_uint64), ("len", C.c_uint32), ("elem", C.c_uint32), ("tile0", C.c_uint32), ("reserved", C.c_uint32)]


def bind_ediff_cost_kernel(L):
    """qzstd_hip_ediff_cost on a loaded device layer (libqatseqprod, or tests/mock/mock_hip_ediff_cost.c built alone)"""
    L.qzstd_hip_ediff_cost.restype = C.c_int
    L.qzstd_hip_ediff_cost.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def ediff_cost_of(data: bytes, k: int, lib=None) -> tuple:
    """QZSTD_ediffCostOf: (P, D) of one chunk — the summed order-0 plane costs of its k-byte elements as they are and differenced
    (include/qzstd_ediffcost.h's own function through the front-end library's export)"""
    L = lib if lib is not None else bind(B.Front().lib)
    s = (C.c_ulonglong * 2)()
    L.QZSTD_ediffCostOf(bytes(data), len(data), k, s)
    return int(s[0]), int(s[1])


def ediff_cost(data: bytes, k: int, chunk: int, lib=None) -> tuple:
    """(P, D) of a buffer: ediff_cost_of summed over its chunks, as QZSTD_frontAdviseDeviceBatch sums them"""
    P = D = 0
    for o in range(0, len(data), chunk):
        p, d = ediff_cost_of(data[o:o + chunk], k, lib)
        P, D = P + p, D + d
    return P, D


def ediff_advised(P: int, D: int, lib=None) -> bool:
    """QZSTD_ediffAdvisedOf: the rule that flags a buffer"""
    L = lib if lib is not None else bind(B.Front().lib)
    return bool(L.QZSTD_ediffAdvisedOf(P, D))


def bind_elemdiff(L):
    """include/qzstd_elemdiff.h on a loaded library (libqzstdfront, or qzstd_elemdiff.c built alone)"""
    for fn in (L.QZSTD_elemDiff, L.QZSTD_elemSum):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint]
    return L


_elemdiff_lib = None


def _ed(lib):
    global _elemdiff_lib
    if lib is not None:
        return lib
    if _elemdiff_lib is None:
        _elemdiff_lib = bind_elemdiff(B.Front().lib)
    return _elemdiff_lib


def elem_diff(data: bytes, k: int, lib=None) -> bytes:
    """QZSTD_elemDiff: one chunk's zigzagged element differences for element size k"""
    return _regroup(_ed(lib).QZSTD_elemDiff, data, k)


def elem_sum(data: bytes, k: int, lib=None) -> bytes:
    """QZSTD_elemSum: the inverse of elem_diff"""
    return _regroup(_ed(lib).QZSTD_elemSum, data, k)


def group_blocks(n: int, k: int, lib=None) -> list:
    """QZSTD_byteGroupBlocks: the block ends of a grouped frame of n bytes"""
    L = _bg(lib)
    cnt = L.QZSTD_byteGroupBlocks(n, k, None, 0)
    if cnt == ERROR:
        raise ValueError("element size %r: 1, 2, 4 or 8" % (k,))
    ends = (C.c_size_t * max(cnt, 1))()
    assert L.QZSTD_byteGroupBlocks(n, k, ends, cnt) == cnt
    return list(ends[:cnt])


class DeviceFront:
    """one QZSTD_Front (threads, level, chunk) with both ways in: host bytes (QZSTD_frontCompress) and a device address
    (QZSTD_frontCompressDevice).  `lib`: an already loaded front-end library (tests: a mock build), else lib/libqzstdfront.so."""

    def __init__(self, threads: int, level: int, chunk: int, ext_rep: int = 0, use_producer: int = 1, lib=None, segment: int = 0):
        self.lib = bind(lib if lib is not None else B.Front().lib)
        self.chunk = chunk
        self.f = self.lib.QZSTD_createFront(C.byref(B.FrontParams(threads, level, chunk, segment, ext_rep, use_producer)))
        if not self.f:
            raise RuntimeError("QZSTD_createFront failed")
        self.stride = self.lib.QZSTD_frontFrameStride(self.f)
        self._dst = None

    def reserve(self, size: int):
        """size the destination for inputs of up to `size` bytes once (timed loops: no allocation inside the window)"""
        self._buffers(size)

    def frames(self, n: int, sizes) -> list:
        """the frames the last call left in the destination"""
        return self._frames(n, sizes)

    def call_host(self, addr: int, size: int):
        """QZSTD_frontCompress alone -> (return value, sizes); frames stay in the destination (frames())"""
        n, sizes = self._buffers(size)
        return self.lib.QZSTD_frontCompress(self.f, C.c_void_p(addr), size, self._dst, len(self._dst), sizes), sizes

    def call_device(self, d_src: int, size: int, stream: int | None = None):
        """QZSTD_frontCompressDevice alone -> (return value, sizes); frames stay in the destination (frames())"""
        n, sizes = self._buffers(size)
        return self.lib.QZSTD_frontCompressDevice(self.f, C.c_void_p(d_src), size, C.c_void_p(stream or None), self._dst,
                                                  len(self._dst), sizes), sizes

    def _buffers(self, size: int):
        return self._frame_buffers((size + self.chunk - 1) // self.chunk)

    def _frame_buffers(self, n: int):
        if self._dst is None or len(self._dst) < max(n, 1) * self.stride:
            self._dst = C.create_string_buffer(max(n, 1) * self.stride)
        return n, (C.c_size_t * max(n, 1))()

    def batch(self, ptrs_and_sizes):
        """-> (QZSTD_DeviceBuf array, its length, frames the batch yields) for [(device address, bytes), ...]"""
        bufs = (DeviceBuf * max(len(ptrs_and_sizes), 1))()
        for i, (p, n) in enumerate(ptrs_and_sizes):
            bufs[i].d_ptr, bufs[i].size = p or None, n
        return bufs, len(ptrs_and_sizes), self.lib.QZSTD_frontDeviceBatchFrames(self.f, bufs, len(ptrs_and_sizes))

    def reserve_frames(self, n: int):
        """size the destination for n frames once (timed loops)"""
        self._frame_buffers(n)

    def call_device_batch(self, bufs, n_bufs: int, n_frames: int, stream: int | None = None):
        """QZSTD_frontCompressDeviceBatch alone on a prepared array (batch()) -> (return value, sizes); frames stay in the destination"""
        _, sizes = self._frame_buffers(n_frames)
        return self.lib.QZSTD_frontCompressDeviceBatch(self.f, bufs, n_bufs, C.c_void_p(stream or None), self._dst, len(self._dst), sizes,
                                                       None), sizes

    def compress_device_batch_raw(self, ptrs_and_sizes, stream: int | None = None, dst_capacity: int | None = None):
        """-> (return value of QZSTD_frontCompressDeviceBatch, per buffer its list of frames or None, firstFrame as a list)"""
        bufs, nb, n = self.batch(ptrs_and_sizes)
        _, sizes = self._frame_buffers(n)
        first = (C.c_size_t * (nb + 1))()
        cap = len(self._dst) if dst_capacity is None else dst_capacity
        r = self.lib.QZSTD_frontCompressDeviceBatch(self.f, bufs, nb, C.c_void_p(stream or None), self._dst, cap, sizes, first)
        if r != n:
            return r, None, list(first)
        fr = self._frames(n, sizes)
        return r, [fr[first[i]:first[i + 1]] for i in range(nb)], list(first)

    def compress_device_batch_typed_raw(self, ptrs_and_sizes, elem_sizes, stream: int | None = None):
        """QZSTD_frontCompressDeviceBatchTyped -> (return value, per buffer its list of frames or None); elem_sizes: one of 0 (the front's
        setting), 1, 2, 4, 8 per buffer, or None"""
        bufs, nb, n = self.batch(ptrs_and_sizes)
        _, sizes = self._frame_buffers(n)
        first = (C.c_size_t * (nb + 1))()
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        r = self.lib.QZSTD_frontCompressDeviceBatchTyped(self.f, bufs, es, nb, C.c_void_p(stream or None), self._dst, len(self._dst), sizes, first)
        self.last = (n, sizes)  # (restore_last: the frames where this call left them)
        if r != n:
            return r, None
        fr = self._frames(n, sizes)
        return r, [fr[first[i]:first[i + 1]] for i in range(nb)]

    def compress_device_batch_typed(self, ptrs_and_sizes, elem_sizes, stream: int | None = None) -> list:
        r, frames = self.compress_device_batch_typed_raw(ptrs_and_sizes, elem_sizes, stream)
        if frames is None:
            raise RuntimeError("QZSTD_frontCompressDeviceBatchTyped failed (%d)" % (r if r != ERROR else -1))
        return frames

    def compress_device_batch_delta_raw(self, ptrs_and_sizes, bases, elem_sizes, stream: int | None = None):
        """QZSTD_frontCompressDeviceBatchDelta -> (return value, per buffer its list of frames or None); bases: per buffer (device address,
        bytes), or None / (0, 0) for a buffer without one; or None for no array at all"""
        bufs, nb, n = self.batch(ptrs_and_sizes)
        _, sizes = self._frame_buffers(n)
        first = (C.c_size_t * (nb + 1))()
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        bs = None if bases is None else self.batch([b or (0, 0) for b in bases])[0]
        r = self.lib.QZSTD_frontCompressDeviceBatchDelta(self.f, bufs, bs, es, nb, C.c_void_p(stream or None), self._dst, len(self._dst), sizes,
                                                         first)
        self.last = (n, sizes)
        if r != n:
            return r, None
        fr = self._frames(n, sizes)
        return r, [fr[first[i]:first[i + 1]] for i in range(nb)]

    def compress_device_batch_delta(self, ptrs_and_sizes, bases, elem_sizes, stream: int | None = None) -> list:
        r, frames = self.compress_device_batch_delta_raw(ptrs_and_sizes, bases, elem_sizes, stream)
        if frames is None:
            raise RuntimeError("QZSTD_frontCompressDeviceBatchDelta failed (%d)" % (r if r != ERROR else -1))
        return frames

    def src_slice_array(self, slices):
        """-> QZSTD_DeviceSrcSlice array for [(buffer index, offset, size, source address, base address or None), ...]"""
        arr = (DeviceSrcSlice * max(len(slices), 1))()
        for a, (buf, off, size, src, base) in zip(arr, slices):
            a.buf, a.offset, a.size, a.d_src, a.d_base = buf, off, size, src or None, base or None
        return arr

    def call_compress_slices(self, buf_sizes, n_bufs: int, elem_sizes, slice_arr, n_slices: int, sizes, first, stream: int | None = None):
        """QZSTD_frontCompressDeviceSlices alone on prepared arguments (a c_size_t array of sizes, src_slice_array(), reserve_frames()) -> its
        return value; frames stay in the destination"""
        return self.lib.QZSTD_frontCompressDeviceSlices(self.f, buf_sizes, elem_sizes, n_bufs, slice_arr, n_slices, C.c_void_p(stream or None),
                                                        self._dst, len(self._dst), sizes, first)

    def compress_device_slices_raw(self, buf_sizes, elem_sizes, slices, stream: int | None = None):
        """QZSTD_frontCompressDeviceSlices -> (return value, per buffer its list of frames or None); buf_sizes: the logical buffers' sizes (or
        None for no array), slices: [(buffer index, offset, size, source address, base address or None), ...] (or None for no array)"""
        nb = 0 if buf_sizes is None else len(buf_sizes)
        n = sum(-(-b // self.chunk) for b in buf_sizes or ())
        _, sizes = self._frame_buffers(n)
        first = (C.c_size_t * (nb + 1))()
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        bs = None if buf_sizes is None else (C.c_size_t * max(nb, 1))(*buf_sizes)
        r = self.call_compress_slices(bs, nb, es, None if slices is None else self.src_slice_array(slices), 0 if slices is None else len(slices),
                                      sizes, first, stream)
        self.last = (n, sizes)
        if r != n:
            return r, None
        fr = self._frames(n, sizes)
        return r, [fr[first[i]:first[i + 1]] for i in range(nb)]

    def compress_device_slices(self, buf_sizes, elem_sizes, slices, stream: int | None = None) -> list:
        r, frames = self.compress_device_slices_raw(buf_sizes, elem_sizes, slices, stream)
        if frames is None:
            raise RuntimeError("QZSTD_frontCompressDeviceSlices failed (%d)" % (r if r != ERROR else -1))
        return frames

    def src_slice_stats(self) -> list:
        """QZSTD_frontSrcSliceStats: [0] non-empty slices of the calls that succeeded, [1] their bytes, [2] frames assembled from more than
        one piece, [3] qzstd_hip_group_pieces launches"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontSrcSliceStats(self.f, st)
        return list(st)

    def restore_batch_delta_raw(self, frames_per_buffer, ptrs_and_sizes, bases, elem_sizes=None, stream: int | None = None, compact: bool = False,
                                n_frames: int | None = None):
        """QZSTD_frontRestoreDeviceBatchDelta: restore_batch_raw with a base per buffer (as compress_device_batch_delta_raw's) -> its return value"""
        flat = [f for fr in frames_per_buffer for f in fr]
        buf, stride, sizes = self.pack_frames(flat, compact)
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        bs = None if bases is None else self.batch([b or (0, 0) for b in bases])[0]
        return self.lib.QZSTD_frontRestoreDeviceBatchDelta(self.f, buf, stride, sizes, len(flat) if n_frames is None else n_frames,
                                                           self.out_batch(ptrs_and_sizes), bs, es, len(ptrs_and_sizes), C.c_void_p(stream or None))

    def restore_batch_delta(self, frames_per_buffer, ptrs_and_sizes, bases, elem_sizes=None, stream: int | None = None, compact: bool = False) -> int:
        r = self.restore_batch_delta_raw(frames_per_buffer, ptrs_and_sizes, bases, elem_sizes, stream, compact)
        if r != sum(len(fr) for fr in frames_per_buffer):
            raise RuntimeError("QZSTD_frontRestoreDeviceBatchDelta failed (%d)" % (r if r != ERROR else -1))
        return r

    def elem_diff_stats(self) -> list:
        """QZSTD_frontElemDiffStats: flagged frames [0] differenced on the GPU, [1] of those differenced again on the host (a failed block),
        [2] summed by a restore; [3] qzstd_hip_esum launches"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontElemDiffStats(self.f, st)
        return list(st)

    def delta_stats(self) -> list:
        """frames with a base built from [0] sequences + literals, [1] rebuilt content, [2] both buffers copied back; [3] frames restored onto a base"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontDeltaStats(self.f, st)
        return list(st)

    def set_delta_skip(self, on) -> int:
        """QZSTD_frontSetDeltaSkip: the delta calls that follow find chunks equal to their base chunk on the GPU and skip them -> 0, or -1
        while a call runs"""
        return self.lib.QZSTD_frontSetDeltaSkip(self.f, 1 if on else 0)

    def get_delta_skip(self) -> int:
        return self.lib.QZSTD_frontGetDeltaSkip(self.f)

    def delta_skip_stats(self) -> list:
        """[0] frames compared with their base chunk, [1] of them found equal (written as zero frames), [2] bytes compared, [3] zero frames
        a restore recognised"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontDeltaSkipStats(self.f, st)
        return list(st)

    def set_plane_probe(self, on) -> int:
        """QZSTD_frontSetPlaneProbe: the grouped and delta calls that follow find their noise planes on the GPU and write them as raw blocks
        -> 0, or -1 while a call runs"""
        return self.lib.QZSTD_frontSetPlaneProbe(self.f, 1 if on else 0)

    def get_plane_probe(self) -> int:
        return self.lib.QZSTD_frontGetPlaneProbe(self.f)

    def set_plane_code(self, on) -> int:
        """QZSTD_frontSetPlaneCode: as with the plane probe on, and the blocks QZSTD_hufTakes takes are Huffman-coded on the GPU; a frame of
        raw-predicted and taken blocks alone is assembled without any libzstd call"""
        return self.lib.QZSTD_frontSetPlaneCode(self.f, 1 if on else 0)

    def get_plane_code(self) -> int:
        return self.lib.QZSTD_frontGetPlaneCode(self.f)

    def plane_code_stats(self) -> list:
        """[rows the kernel coded, blocks taken, frames assembled without libzstd, frames with a taken block that fell back]"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontPlaneCodeStats(self.f, st)
        return list(st)

    def plane_probe_stats(self) -> list:
        """[0] blocks probed, [1] blocks written raw by the library, [2] frames assembled by the library, [3] frames that fell back"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontPlaneProbeStats(self.f, st)
        return list(st)

    def compress_device_batch(self, ptrs_and_sizes, stream: int | None = None) -> list:
        """frames of every buffer of [(device address, bytes), ...], a list of lists: one QZSTD_frontCompressDeviceBatch call"""
        r, frames, _ = self.compress_device_batch_raw(ptrs_and_sizes, stream)
        if frames is None:
            raise RuntimeError("QZSTD_frontCompressDeviceBatch failed (%d)" % (r if r != ERROR else -1))
        return frames

    def _frames(self, n, sizes):
        raw = self._dst.raw
        return [raw[c * self.stride:c * self.stride + sizes[c]] for c in range(n)]

    def compress_host(self, data) -> list:
        src = (C.c_char * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        return self.compress_host_ptr(C.addressof(src), len(data))

    def compress_host_ptr(self, addr: int, size: int) -> list:
        n, sizes = self._buffers(size)
        if self.lib.QZSTD_frontCompress(self.f, C.c_void_p(addr), size, self._dst, len(self._dst), sizes) != n:
            raise RuntimeError("QZSTD_frontCompress failed")
        return self._frames(n, sizes)

    def compress_device_raw(self, d_src: int, size: int, stream: int | None = None, dst_capacity: int | None = None):
        """-> (return value of QZSTD_frontCompressDevice, frames or None)"""
        n, sizes = self._buffers(size)
        cap = len(self._dst) if dst_capacity is None else dst_capacity
        r = self.lib.QZSTD_frontCompressDevice(self.f, C.c_void_p(d_src), size, C.c_void_p(stream or None), self._dst, cap, sizes)
        return r, (self._frames(n, sizes) if r == n else None)

    def compress_device(self, d_src: int, size: int, stream: int | None = None) -> list:
        r, frames = self.compress_device_raw(d_src, size, stream)
        if frames is None:
            raise RuntimeError("QZSTD_frontCompressDevice failed (%d)" % (r if r != ERROR else -1))
        return frames

    def stats(self) -> list:
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontDeviceStats(self.f, st)
        return list(st)

    def set_checksum(self, on) -> int:
        """QZSTD_frontSetChecksum: content checksums in every frame of the calls that follow -> 0, or -1 while a call runs"""
        return self.lib.QZSTD_frontSetChecksum(self.f, 1 if on else 0)

    def get_checksum(self) -> int:
        return self.lib.QZSTD_frontGetChecksum(self.f)

    def checksum_stats(self) -> list:
        """frames whose checksum [0] the GPU computed, [1] libzstd computed"""
        st = (C.c_ulonglong * 2)()
        self.lib.QZSTD_frontChecksumStats(self.f, st)
        return list(st)

    def set_byte_group(self, k: int) -> int:
        """QZSTD_frontSetByteGroup: the element size (1: off, 2, 4, 8) of every device call that follows -> 0, or -1 (another value, or
        while a call runs)"""
        return self.lib.QZSTD_frontSetByteGroup(self.f, k)

    def get_byte_group(self) -> int:
        return self.lib.QZSTD_frontGetByteGroup(self.f)

    def byte_group_stats(self) -> list:
        """byte-grouped frames built from [0] sequences + literals, [1] rebuilt content, [2] copied-back content"""
        st = (C.c_ulonglong * 3)()
        self.lib.QZSTD_frontByteGroupStats(self.f, st)
        return list(st)

    def pack_frames(self, frames, compact: bool = False):
        """frames (a flat list of bytes) in host memory as the restore calls read them -> (buffer, frameStride, sizes array): at the
        front's stride, as the compress calls leave them, or compact=True back to back with frameStride 0, as QZSTD_frontCompact leaves them"""
        sizes = (C.c_size_t * max(len(frames), 1))(*[len(f) for f in frames])
        if compact:
            return C.create_string_buffer(b"".join(frames), max(sum(len(f) for f in frames), 1)), 0, sizes
        stride = max([self.stride] + [len(f) for f in frames])
        buf = C.create_string_buffer(max(len(frames), 1) * stride)
        for c, f in enumerate(frames):
            C.memmove(C.addressof(buf) + c * stride, f, len(f))
        return buf, stride, sizes

    def out_batch(self, ptrs_and_sizes):
        """-> QZSTD_DeviceOutBuf array for [(device address, bytes), ...]"""
        bufs = (DeviceOutBuf * max(len(ptrs_and_sizes), 1))()
        for i, (p, n) in enumerate(ptrs_and_sizes):
            bufs[i].d_ptr, bufs[i].size = p or None, n
        return bufs

    def call_restore(self, packed, n_frames: int, bufs, n_bufs: int, elem_sizes=None, stream: int | None = None):
        """QZSTD_frontRestoreDeviceBatchTyped alone on prepared arguments (pack_frames(), out_batch()) -> its return value"""
        buf, stride, sizes = packed
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        return self.lib.QZSTD_frontRestoreDeviceBatchTyped(self.f, buf, stride, sizes, n_frames, bufs, es, n_bufs, C.c_void_p(stream or None))

    def restore_last(self, n_frames: int, sizes, ptrs_and_sizes, elem_sizes=None, stream: int | None = None, compacted: bool = False):
        """the frames the last compress call left in the destination, restored from where they lie -> the restore's return value;
        compacted=True: QZSTD_frontCompact first, then frameStride 0"""
        if compacted:
            self.lib.QZSTD_frontCompact(self.f, self._dst, sizes, n_frames)
        return self.call_restore((self._dst, 0 if compacted else self.stride, sizes), n_frames, self.out_batch(ptrs_and_sizes),
                                 len(ptrs_and_sizes), elem_sizes, stream)

    def restore_batch_raw(self, frames_per_buffer, ptrs_and_sizes, elem_sizes=None, stream: int | None = None, compact: bool = False,
                          n_frames: int | None = None):
        """per buffer its list of frames (what the compress helpers return) restored into [(device address, bytes), ...] by ONE
        QZSTD_frontRestoreDeviceBatchTyped call -> its return value (the frame count, or ERROR); elem_sizes: one of 0 (the front's
        setting), 1, 2, 4, 8 per buffer, or None; n_frames: what to pass as nFrames instead of the frames' count"""
        flat = [f for fr in frames_per_buffer for f in fr]
        return self.call_restore(self.pack_frames(flat, compact), len(flat) if n_frames is None else n_frames, self.out_batch(ptrs_and_sizes),
                                 len(ptrs_and_sizes), elem_sizes, stream)

    def restore_batch(self, frames_per_buffer, ptrs_and_sizes, elem_sizes=None, stream: int | None = None, compact: bool = False) -> int:
        r = self.restore_batch_raw(frames_per_buffer, ptrs_and_sizes, elem_sizes, stream, compact)
        if r != sum(len(fr) for fr in frames_per_buffer):
            raise RuntimeError("QZSTD_frontRestoreDeviceBatchTyped failed (%d)" % (r if r != ERROR else -1))
        return r

    def restore_device_raw(self, frames, d_dst: int, size: int, stream: int | None = None, compact: bool = False):
        """QZSTD_frontRestoreDevice: one buffer's frames, the front's element size -> its return value"""
        buf, stride, sizes = self.pack_frames(list(frames), compact)
        return self.lib.QZSTD_frontRestoreDevice(self.f, buf, stride, sizes, len(frames), C.c_void_p(d_dst or None), size,
                                                 C.c_void_p(stream or None))

    def slice_array(self, slices):
        """-> QZSTD_DeviceSlice array for [(buffer index, offset, size, destination address, base address or None), ...]"""
        arr = (DeviceSlice * max(len(slices), 1))()
        for a, (buf, off, size, dst, base) in zip(arr, slices):
            a.buf, a.offset, a.size, a.d_dst, a.d_base = buf, off, size, dst or None, base or None
        return arr

    def call_restore_slices(self, packed, n_frames: int, buf_sizes, elem_sizes, slice_arr, n_slices: int, stream: int | None = None):
        """QZSTD_frontRestoreDeviceSlices alone on prepared arguments (pack_frames(), slice_array()) -> its return value"""
        buf, stride, sizes = packed
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        bs = None if buf_sizes is None else (C.c_size_t * max(len(buf_sizes), 1))(*buf_sizes)
        return self.lib.QZSTD_frontRestoreDeviceSlices(self.f, buf, stride, sizes, n_frames, bs, es, 0 if buf_sizes is None else len(buf_sizes),
                                                       slice_arr, n_slices, C.c_void_p(stream or None))

    def restore_slices_raw(self, frames_per_buffer, buf_sizes, elem_sizes, slices, stream: int | None = None, compact: bool = False,
                           n_frames: int | None = None):
        """QZSTD_frontRestoreDeviceSlices: the WHOLE frame list of the buffers as they were written (per buffer its frames; buf_sizes: the
        written sizes), and slices [(buffer index, offset, size, destination address, base address or None), ...] in ascending order
        -> its return value (the frames decoded, or ERROR)"""
        flat = [f for fr in frames_per_buffer for f in fr]
        return self.call_restore_slices(self.pack_frames(flat, compact), len(flat) if n_frames is None else n_frames, buf_sizes, elem_sizes,
                                        None if slices is None else self.slice_array(slices), 0 if slices is None else len(slices), stream)

    def restore_slices(self, frames_per_buffer, buf_sizes, elem_sizes, slices, stream: int | None = None, compact: bool = False) -> int:
        r = self.restore_slices_raw(frames_per_buffer, buf_sizes, elem_sizes, slices, stream, compact)
        if r == ERROR:
            raise RuntimeError("QZSTD_frontRestoreDeviceSlices failed")
        return r

    def slice_stats(self) -> list:
        """[0] non-empty slices restored, [1] bytes written to destinations, [2] frames decoded for them, [3] rows launched"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontSliceStats(self.f, st)
        return list(st)

    def call_verify(self, packed, n_frames: int, bufs, bases, n_bufs: int, elem_sizes=None, stream: int | None = None, first_diff=None):
        """QZSTD_frontVerifyDeviceBatch alone on prepared arguments (pack_frames(), batch()[0] for the live buffers and for the bases, a
        c_size_t array or None for firstDiff) -> its return value"""
        buf, stride, sizes = packed
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        return self.lib.QZSTD_frontVerifyDeviceBatch(self.f, buf, stride, sizes, n_frames, bufs, bases, es, n_bufs, C.c_void_p(stream or None),
                                                     first_diff)

    def verify_raw(self, frames_per_buffer, ptrs_and_sizes, bases=None, elem_sizes=None, stream: int | None = None, compact: bool = False,
                   n_frames: int | None = None, want_offsets: bool = True):
        """QZSTD_frontVerifyDeviceBatch: per buffer its list of frames, compared with the LIVE buffers [(device address, bytes), ...] (bases
        as compress_device_batch_delta_raw's) -> (return value: the number of differing frames or ERROR, firstDiff as a flat list or None)"""
        flat = [f for fr in frames_per_buffer for f in fr]
        first = (C.c_size_t * max(len(flat), 1))(*([7] * max(len(flat), 1))) if want_offsets else None
        bs = None if bases is None else self.batch([b or (0, 0) for b in bases])[0]
        r = self.call_verify(self.pack_frames(flat, compact), len(flat) if n_frames is None else n_frames, self.batch(ptrs_and_sizes)[0], bs,
                             len(ptrs_and_sizes), elem_sizes, stream, first)
        return r, (list(first)[:len(flat)] if want_offsets else None)

    def verify(self, frames_per_buffer, ptrs_and_sizes, bases=None, elem_sizes=None, stream: int | None = None, compact: bool = False) -> list:
        """-> [(buffer index, frame index inside the buffer, byte offset inside that frame's chunk), ...] for the frames that do NOT reproduce
        the live buffers; []: the checkpoint is good.  Raises when the call fails (a frame that does not decode included)"""
        r, first = self.verify_raw(frames_per_buffer, ptrs_and_sizes, bases, elem_sizes, stream, compact)
        if r == ERROR:
            raise RuntimeError("QZSTD_frontVerifyDeviceBatch failed")
        out, c = [], 0
        for i, fr in enumerate(frames_per_buffer):
            for j in range(len(fr)):
                if first[c] != VERIFY_SAME:
                    out.append((i, j, first[c]))
                c += 1
        assert len(out) == r
        return out

    def verify_stats(self) -> list:
        """[0] frames compared, [1] of them differing, [2] content bytes compared, [3] qzstd_hip_ungroup_cmp launches"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontVerifyStats(self.f, st)
        return list(st)

    def fingerprint_raw(self, ptrs_and_sizes, stream: int | None = None, null_fp: bool = False):
        """QZSTD_frontFingerprintDeviceBatch -> (return value, the fingerprints as a flat list or None, firstFrame as a list)"""
        bufs, nb, n = self.batch(ptrs_and_sizes)
        fp = (C.c_ulonglong * max(n if n != ERROR else 0, 1))()
        first = (C.c_size_t * (nb + 1))()
        r = self.lib.QZSTD_frontFingerprintDeviceBatch(self.f, bufs, nb, C.c_void_p(stream or None), None if null_fp else fp, first)
        return r, (list(fp)[:n] if r == n else None), list(first)

    def fingerprint(self, ptrs_and_sizes, stream: int | None = None) -> list:
        """per buffer the fingerprints of its chunks (8 bytes per frame: what the caller keeps with the frames)"""
        r, fp, first = self.fingerprint_raw(ptrs_and_sizes, stream)
        if fp is None:
            raise RuntimeError("QZSTD_frontFingerprintDeviceBatch failed")
        return [fp[first[i]:first[i + 1]] for i in range(len(ptrs_and_sizes))]

    def check_raw(self, ptrs_and_sizes, expected, stream: int | None = None, n_frames: int | None = None, want_flags: bool = True):
        """QZSTD_frontCheckDeviceBatch against a flat list of fingerprints (None: a null pointer) -> (return value: the number of differing
        frames or ERROR, differs as a flat list or None)"""
        bufs, nb, _ = self.batch(ptrs_and_sizes)
        n = len(expected) if expected is not None else 0
        ex = None if expected is None else (C.c_ulonglong * max(n, 1))(*expected)
        flags = C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1)) if want_flags else None
        r = self.lib.QZSTD_frontCheckDeviceBatch(self.f, bufs, nb, C.c_void_p(stream or None), ex, n if n_frames is None else n_frames, flags)
        return r, (list(flags.raw[:n]) if want_flags else None)

    def check(self, ptrs_and_sizes, fingerprints_per_buffer, stream: int | None = None) -> list:
        """-> [(buffer index, frame index inside the buffer), ...] for the chunks whose fingerprint is another one now; []: the buffers are
        what was fingerprinted.  Raises when the call fails"""
        r, flags = self.check_raw(ptrs_and_sizes, [v for fp in fingerprints_per_buffer for v in fp], stream)
        if r == ERROR:
            raise RuntimeError("QZSTD_frontCheckDeviceBatch failed")
        out, c = [], 0
        for i, fp in enumerate(fingerprints_per_buffer):
            for j in range(len(fp)):
                if flags[c]:
                    out.append((i, j))
                c += 1
        assert len(out) == r
        return out

    def fingerprint_stats(self) -> list:
        """[0] frames fingerprinted, [1] bytes read on the device, [2] qzstd_hip_fingerprint launches, [3] frames a check found differing"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontFingerprintStats(self.f, st)
        return list(st)

    def _slice_args(self, buf_sizes, slices):
        nb = 0 if buf_sizes is None else len(buf_sizes)
        bs = None if buf_sizes is None else (C.c_size_t * max(nb, 1))(*buf_sizes)
        return bs, nb, (None if slices is None else self.src_slice_array(slices)), (0 if slices is None else len(slices))

    def fingerprint_slices_raw(self, buf_sizes, slices, stream: int | None = None, null_fp: bool = False):
        """QZSTD_frontFingerprintDeviceSlices (buf_sizes and slices as compress_device_slices_raw's) -> (return value, the fingerprints as a
        flat list or None, firstFrame as a list)"""
        bs, nb, arr, ns = self._slice_args(buf_sizes, slices)
        n = sum(-(-b // self.chunk) for b in buf_sizes or ())
        fp = (C.c_ulonglong * max(n, 1))()
        first = (C.c_size_t * (nb + 1))()
        r = self.lib.QZSTD_frontFingerprintDeviceSlices(self.f, bs, nb, arr, ns, C.c_void_p(stream or None), None if null_fp else fp, first)
        return r, (list(fp)[:n] if r == n else None), list(first)

    def fingerprint_slices(self, buf_sizes, slices, stream: int | None = None) -> list:
        """per logical buffer the fingerprints of its chunks"""
        r, fp, first = self.fingerprint_slices_raw(buf_sizes, slices, stream)
        if fp is None:
            raise RuntimeError("QZSTD_frontFingerprintDeviceSlices failed")
        return [fp[first[i]:first[i + 1]] for i in range(len(buf_sizes))]

    def check_slices_raw(self, buf_sizes, slices, expected, stream: int | None = None, n_frames: int | None = None, want_flags: bool = True):
        """QZSTD_frontCheckDeviceSlices against a flat list of fingerprints (None: a null pointer) -> (return value: the number of differing
        frames or ERROR, differs as a flat list or None)"""
        bs, nb, arr, ns = self._slice_args(buf_sizes, slices)
        n = len(expected) if expected is not None else 0
        ex = None if expected is None else (C.c_ulonglong * max(n, 1))(*expected)
        flags = C.create_string_buffer(b"\x07" * max(n, 1), max(n, 1)) if want_flags else None
        r = self.lib.QZSTD_frontCheckDeviceSlices(self.f, bs, nb, arr, ns, C.c_void_p(stream or None), ex, n if n_frames is None else n_frames, flags)
        return r, (list(flags.raw[:n]) if want_flags else None)

    def verify_slices_raw(self, frames_per_buffer, buf_sizes, elem_sizes, slices, stream: int | None = None, compact: bool = False,
                          n_frames: int | None = None, want_offsets: bool = True):
        """QZSTD_frontVerifyDeviceSlices: per buffer its list of frames, compared with the LIVE slices [(buffer index, offset, size, source
        address, base address or None), ...] -> (return value: the number of differing frames or ERROR, firstDiff as a flat list or None)"""
        flat = [f for fr in frames_per_buffer for f in fr]
        first = (C.c_size_t * max(len(flat), 1))(*([7] * max(len(flat), 1))) if want_offsets else None
        bs, nb, arr, ns = self._slice_args(buf_sizes, slices)
        buf, stride, sizes = self.pack_frames(flat, compact)
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        r = self.lib.QZSTD_frontVerifyDeviceSlices(self.f, buf, stride, sizes, len(flat) if n_frames is None else n_frames, bs, es, nb, arr, ns,
                                                   C.c_void_p(stream or None), first)
        return r, (list(first)[:len(flat)] if want_offsets else None)

    def slice_check_stats(self) -> list:
        """QZSTD_frontSliceCheckStats: [0] non-empty slices of the calls that succeeded, [1] their bytes, [2] frames assembled from more than
        one piece, [3] launches of qzstd_hip_fingerprint_pieces and qzstd_hip_ungroup_cmp_pieces"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontSliceCheckStats(self.f, st)
        return list(st)

    def advise_raw(self, ptrs_and_sizes, elem_sizes=None, stream: int | None = None, null_advised: bool = False, want_est: bool = True):
        """QZSTD_frontAdviseDeviceBatch -> (return value: the number of flagged buffers or ERROR, advised as a list of ints — 0x07 where
        the call wrote nothing —, est as [(P, D), ...] or None); elem_sizes: one of 0 (the front's setting), 1, 2, 4, 8 per buffer, or None"""
        bufs, nb, _ = self.batch(ptrs_and_sizes)
        es = None if elem_sizes is None else bytes(bytearray(elem_sizes)) + b"\0"
        adv = C.create_string_buffer(b"\x07" * max(nb, 1), max(nb, 1))
        est = (C.c_ulonglong * max(2 * nb, 1))() if want_est else None
        r = self.lib.QZSTD_frontAdviseDeviceBatch(self.f, bufs, es, nb, C.c_void_p(stream or None), None if null_advised else adv, est)
        return r, list(adv.raw[:nb]), ([(int(est[2 * i]), int(est[2 * i + 1])) for i in range(nb)] if want_est else None)

    def advise(self, ptrs_and_sizes, elem_sizes=None, stream: int | None = None):
        """-> (the elemSizes array to pass to the Typed compress and restore calls: each buffer's element size, with ELEM_DIFF where element
        differences are advised; [(P, D), ...]: the estimated order-0 sizes without and with differences).  Raises when the call fails"""
        r, adv, est = self.advise_raw(ptrs_and_sizes, elem_sizes, stream)
        if r == ERROR:
            raise RuntimeError("QZSTD_frontAdviseDeviceBatch failed")
        assert r == sum(1 for a in adv if a & ELEM_DIFF)
        return adv, est

    def advise_stats(self) -> list:
        """[0] buffers advised on, [1] of them flagged, [2] bytes read on the device, [3] qzstd_hip_ediff_cost launches"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontAdviseStats(self.f, st)
        return list(st)

    def restore_stats(self) -> list:
        """[0] frames decoded, [1] bytes of content, [2] bytes copied host->device, [3] ungroup launches"""
        st = (C.c_ulonglong * 4)()
        self.lib.QZSTD_frontRestoreStats(self.f, st)
        return list(st)

    def close(self):
        if self.f:
            self.lib.QZSTD_freeFront(self.f)
            self.f = None


def compress_tensor(front: DeviceFront, t, stream=None) -> list:
    """frames of a contiguous CUDA/HIP tensor's bytes (any dtype), as QZSTD_frontCompress frames the same bytes.  `stream`: the
    torch.cuda.Stream (or raw hipStream_t) that produced t; default: the current stream of t's device."""
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("compress_tensor: a contiguous GPU tensor")
    if stream is None:
        stream = torch.cuda.current_stream(t.device)
    handle = getattr(stream, "cuda_stream", stream)
    return front.compress_device(t.data_ptr(), t.numel() * t.element_size(), handle)


def element_group(t) -> int:
    """the byte-group element size of a tensor: its element size when that is 2, 4 or 8, else 1"""
    return t.element_size() if t.element_size() in (2, 4, 8) else 1


ELEM_DIFF = 0x80  # QZSTD_ELEM_DIFF


def _diff_flags(what: str, tensors, diff):
    """diff: None / False (no tensor), True (every tensor), or one bool per tensor -> per tensor QZSTD_ELEM_DIFF or 0"""
    if diff is None or diff is False:
        return [0] * len(tensors)
    if diff is True:
        return [ELEM_DIFF] * len(tensors)
    diff = list(diff)
    if len(diff) != len(tensors):
        raise ValueError(what + ": diff is a bool, or one bool per tensor")
    return [ELEM_DIFF if d else 0 for d in diff]


def compress_tensors(front: DeviceFront, tensors, stream=None, group=None, diff=None) -> list:
    """per tensor the frames of its bytes, all tensors in ONE call (QZSTD_frontCompressDeviceBatch): contiguous GPU tensors of any dtypes
    and sizes, views with a storage offset included, all on one device.  `stream`: the torch.cuda.Stream (or raw hipStream_t) that
    produced them; default: the current stream of their device.  group="dtype": every tensor byte-grouped by its own element size
    (QZSTD_frontCompressDeviceBatchTyped; restore_tensor() undoes it); None: the front's setting.  diff (with group="dtype" only; off by
    default): True, or one bool per tensor — element differences (QZSTD_ELEM_DIFF) for integer columns with order; unordered data grows."""
    if group not in (None, "dtype"):
        raise ValueError("compress_tensors: group is None or \"dtype\"")
    tensors = list(tensors)
    flags = _diff_flags("compress_tensors", tensors, diff)
    if any(flags) and group != "dtype":
        raise ValueError("compress_tensors: diff needs group=\"dtype\" (differences are taken with each tensor's own element size)")
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("compress_tensors: contiguous GPU tensors")
        if t.device != tensors[0].device:
            raise ValueError("compress_tensors: tensors on one device")
    if not tensors:
        return []
    if stream is None:
        stream = torch.cuda.current_stream(tensors[0].device)
    handle = getattr(stream, "cuda_stream", stream)
    bufs = [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]
    if group == "dtype":
        return front.compress_device_batch_typed(bufs, [element_group(t) | fl for t, fl in zip(tensors, flags)], handle)
    return front.compress_device_batch(bufs, handle)


def restore_tensors(front: DeviceFront, frames_per_tensor, tensors, stream=None, group=None, diff=None) -> int:
    """the way back of compress_tensors(): per tensor its frames, restored INTO the given contiguous GPU tensors (same sizes, same `group`) in ONE
    call (QZSTD_frontRestoreDeviceBatchTyped: decoded by the front's workers, ungrouped on the GPU) -> the frame count"""
    if group not in (None, "dtype"):
        raise ValueError("restore_tensors: group is None or \"dtype\"")
    tensors = list(tensors)
    flags = _diff_flags("restore_tensors", tensors, diff)  # (the values compress_tensors() was given: the frames do not hold them)
    if any(flags) and group != "dtype":
        raise ValueError("restore_tensors: diff needs group=\"dtype\"")
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous() or t.device != tensors[0].device:
            raise ValueError("restore_tensors: contiguous GPU tensors on one device")
    if not tensors:
        return 0
    if stream is None:
        stream = torch.cuda.current_stream(tensors[0].device)
    handle = getattr(stream, "cuda_stream", stream)
    bufs = [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]
    return front.restore_batch(frames_per_tensor, bufs, [element_group(t) | fl for t, fl in zip(tensors, flags)] if group == "dtype" else None, handle)


def verify_tensors(front: DeviceFront, frames_per_tensor, tensors, bases=None, stream=None, group=None) -> list:
    """do the frames compress_tensors() (or a delta call against `bases`) left reproduce the tensors as they are NOW?  ONE
    QZSTD_frontVerifyDeviceBatch call: nothing is written, no temporary of the tensors' size -> [(tensor, frame, byte offset inside the
    frame's chunk), ...] for the frames that differ; []: safe to drop the previous checkpoint.  bases: per tensor a tensor of the same
    byte size or None; group as compress_tensors()'s"""
    if group not in (None, "dtype"):
        raise ValueError("verify_tensors: group is None or \"dtype\"")
    tensors = list(tensors)
    for t in tensors + [b for b in (bases or []) if b is not None]:
        if not t.is_cuda or not t.is_contiguous() or t.device != tensors[0].device:
            raise ValueError("verify_tensors: contiguous GPU tensors on one device")
    if not tensors:
        return []
    if stream is None:
        stream = torch.cuda.current_stream(tensors[0].device)
    handle = getattr(stream, "cuda_stream", stream)
    bufs = [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]
    bs = None if bases is None else [None if b is None else (b.data_ptr(), b.numel() * b.element_size()) for b in bases]
    return front.verify(frames_per_tensor, bufs, bs, [element_group(t) for t in tensors] if group == "dtype" else None, handle)


def _tensor_bufs(what: str, tensors, stream):
    tensors = list(tensors)
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous() or t.device != tensors[0].device:
            raise ValueError("%s: contiguous GPU tensors on one device" % what)
    if tensors and stream is None:
        stream = torch.cuda.current_stream(tensors[0].device)
    return [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors], getattr(stream, "cuda_stream", stream)


def fingerprint_tensors(front: DeviceFront, tensors, stream=None) -> list:
    """per tensor the fingerprints of its chunks, all tensors in ONE QZSTD_frontFingerprintDeviceBatch call: 8 bytes per frame, to be kept
    with the frames; independent of dtype, base and every setting of the front"""
    bufs, handle = _tensor_bufs("fingerprint_tensors", tensors, stream)
    return front.fingerprint(bufs, handle) if bufs else []


def check_tensors(front: DeviceFront, tensors, fingerprints_per_tensor, stream=None) -> list:
    """are the tensors — restored, perhaps weeks later — the tensors that were fingerprinted?  ONE QZSTD_frontCheckDeviceBatch call ->
    [(tensor, frame), ...] for the chunks that differ; []: the load is good"""
    bufs, handle = _tensor_bufs("check_tensors", tensors, stream)
    return front.check(bufs, fingerprints_per_tensor, handle) if bufs else []


def advise_tensors(front: DeviceFront, tensors, stream=None) -> list:
    """per tensor whether element differences are advised (ONE QZSTD_frontAdviseDeviceBatch call over the tensors' own bytes, each with its
    dtype's element size): the list to pass as diff= to compress_tensors() / restore_tensors() with group="dtype", and to keep with the frames"""
    bufs, handle = _tensor_bufs("advise_tensors", tensors, stream)
    if not bufs:
        return []
    adv, _ = front.advise(bufs, [element_group(t) for t in tensors], handle)
    return [bool(a & ELEM_DIFF) for a in adv]


def restore_slices(front: DeviceFront, frames, buf_sizes, elems, slices, stream=None) -> int:
    """QZSTD_frontRestoreDeviceSlices: `frames` per buffer as the compress helpers return them (ALL of them), the buffers' written sizes and
    element sizes, and slices [(buffer index, offset, size, destination address, base address or None), ...] in ascending order -> the number
    of frames decoded: only those a non-empty slice intersects"""
    return front.restore_slices(frames, buf_sizes, elems, slices, getattr(stream, "cuda_stream", stream))


def shard_slices(index: int, shape, itemsize: int, dim: int, start: int, length: int, dst: int, base: int | None = None) -> list:
    """the slices of rows / columns [start, start + length) along `dim` of the 2-D row-major tensor number `index` (shape [R, C], written
    whole), into a CONTIGUOUS destination at device address dst ([length, C] for dim 0: one slice; [R, length] for dim 1: R slices); base:
    the device address of the same shard of the base, laid out as the destination, or None"""
    R, Cc = shape
    if dim not in (0, 1) or start < 0 or length < 0 or start + length > (R, Cc)[dim]:
        raise ValueError("shard_slices: [start, start + length) inside dimension 0 or 1 of a 2-D tensor")
    if dim == 0:
        return [(index, start * Cc * itemsize, length * Cc * itemsize, dst, base)]
    row = length * itemsize
    return [(index, (r * Cc + start) * itemsize, row, dst + r * row, None if base is None else base + r * row) for r in range(R)]


def restore_shards(front: DeviceFront, frames_per_tensor, shapes, dtypes, shards, bases=None, stream=None, device="cuda:0", elems=None) -> list:
    """a resharded load: tensors written whole by compress_tensors(group="dtype") (frames_per_tensor, their 2-D shapes and dtypes, all of them),
    of which this loader wants shards [(tensor index, dim, start, length), ...] (ascending, at most one per tensor) -> per shard a new contiguous
    tensor on `device`, restored by ONE QZSTD_frontRestoreDeviceSlices call; bases: per shard the same shard of the base tensor (contiguous, on
    `device`) or None; elems: the element sizes the tensors were written with, when they are not their dtypes'"""
    itemsizes = [torch.empty((), dtype=dt).element_size() for dt in dtypes]
    outs, slices = [], []
    for s, (index, dim, start, length) in enumerate(shards):
        R, Cc = shapes[index]
        out = torch.empty((length, Cc) if dim == 0 else (R, length), dtype=dtypes[index], device=device)
        b = bases[s] if bases is not None else None
        if b is not None and (not b.is_contiguous() or b.shape != out.shape or b.dtype != out.dtype or b.device != out.device):
            raise ValueError("restore_shards: a base is the shard's shape, dtype and device, contiguous")
        slices += shard_slices(index, shapes[index], itemsizes[index], dim, start, length, out.data_ptr(), None if b is None else b.data_ptr())
        outs.append(out)
    if stream is None:
        stream = torch.cuda.current_stream(torch.device(device))
    sizes = [sh[0] * sh[1] * it for sh, it in zip(shapes, itemsizes)]
    if elems is None:
        elems = [it if it in (2, 4, 8) else 1 for it in itemsizes]
    restore_slices(front, frames_per_tensor, sizes, elems, slices, stream)
    return outs


def restore_tensor(frames, dtype, shape, k: int, device=None, zstd=None, lib=None):
    """the tensor whose byte-grouped frames (element size k, as compress_tensors(group="dtype") built them) these are: every frame decoded
    on the host, ungrouped (the layout follows from the frame's content size and k), the bytes uploaded to `device`"""
    import math
    z = zstd or B.Zstd()
    left = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    out = bytearray()
    for fr in frames:
        content = z.decompress(fr, left)
        out += ungroup_bytes(content, k, lib)
        left -= len(content)
    if left != 0:
        raise ValueError("restore_tensor: the frames hold %d bytes fewer than the shape needs" % left)
    t = torch.frombuffer(out, dtype=torch.uint8).view(dtype).reshape(shape) if out else torch.empty(shape, dtype=dtype)
    return t.to(device) if device is not None else t.clone()


def foreign_frames(zstd, data: bytes, chunk: int, k: int, level: int = 3, checksum: bool = False, lib=None) -> list:
    """frames a reader may meet that this library did not build: plain ZSTD_compress2 (libzstd's own match-finder, its own blocks) over the
    byte-grouped content (group_bytes, element size k) of every chunk"""
    zc = zstd.cctx(level, checksumFlag=1 if checksum else 0)
    try:
        return [zstd.compress2(zc, group_bytes(data[o:o + chunk], k, lib)) for o in range(0, len(data), chunk)]
    finally:
        zstd.free(zc)


def reference_frames(zstd, oracle, data: bytes, chunk: int, level: int, ext_rep: bool = False) -> list:
    """what QZSTD_frontCompressDevice must produce: libzstd's ZSTD_compress2 frames from the ORACLE's sequences, one 128 KiB block per
    delimiter (ZSTD_c_blockSplitterLevel 1) above 128 KiB chunks; ext_rep: the repeat-aware profile (level | 0x100) with
    ZSTD_c_searchForExternalRepcodes on, what QZSTD_HIP_EXT_REPCODES=1 and extRepcodes = 1 ask for"""
    params = {"blockSplitterLevel": 1} if chunk > 131072 else {}
    prof = None
    if ext_rep:
        prof = oracle.profile(level | 0x100, min(chunk, 131072))
        zc = zstd.cctx(level, producer=oracle.producer_addr, state=C.addressof(prof), validate=True, ext_repcodes=1, **params)
    else:
        zc = zstd.cctx(level, producer=oracle.producer_addr, state=None, validate=True, **params)
    try:
        return zstd.compress_chunks(zc, data, chunk)[1]
    finally:
        zstd.free(zc)
        del prof


def typed_corpus(kind: str, nbytes: int, seed: int = 0) -> bytes:
    """seeded typed data, nbytes of it: "bf16" / "fp16" / "fp32" N(0, 0.02) weights, "ids32" Zipf token ids (int32), "ids64" ascending
    ids (int64, random small steps)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind in ("bf16", "fp16", "fp32"):
        size = {"bf16": 2, "fp16": 2, "fp32": 4}[kind]
        w = rng.normal(0.0, 0.02, (nbytes + size - 1) // size).astype(np.float32)
        if kind == "bf16":
            raw = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
        else:
            raw = w.astype(np.float16).tobytes() if kind == "fp16" else w.tobytes()
    elif kind == "ids32":
        raw = np.minimum(rng.zipf(1.2, (nbytes + 3) // 4), 50000).astype(np.int32).tobytes()
    elif kind == "ids64":
        raw = np.cumsum(rng.integers(1, 40, (nbytes + 7) // 8)).astype(np.int64).tobytes()
    else:
        raise ValueError(kind)
    return raw[:nbytes]


def blocks_with_cuts(n: int, k: int, cut: bool) -> list:
    """block ends of a grouped frame of n bytes with the plane cuts forced on or off, whatever QZSTD_BYTEGROUP_CUT_MIN says (measurements)"""
    pieces = [((j * (n // k)) & ~15) for j in range(1, k)] if cut and k > 1 else []
    ends, start = [], 0
    for piece_end in pieces + [n]:
        while start < piece_end:
            start = min(start + 131072, piece_end)
            ends.append(start)
    return ends


def reference_frames_grouped(zstd, oracle, data: bytes, chunk: int, level: int, k: int, checksum: bool = False, lib=None,
                             counts: dict | None = None, cut: bool | None = None) -> list:
    """what the device calls must produce with element size k: per frame (chunk) group_bytes, the ORACLE's sequences for each block of
    group_blocks (every block matched on its own, the last entry its delimiter), then ZSTD_compressSequences with explicit block delimiters
    and sequence validation on a context with the workers' parameters (the level; checksum: ZSTD_c_checksumFlag).  counts: a dict that
    receives "blocks" and "entries" (sequences, delimiters included) of all frames; cut: None for the library's block rule, True / False to
    force the plane cuts on / off (measurements: blocks_with_cuts)"""
    L = zstd.lib
    L.ZSTD_compressSequences.restype = C.c_size_t
    L.ZSTD_compressSequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(B.Sequence), C.c_size_t, C.c_void_p, C.c_size_t]
    blk = min(chunk, 131072)
    prof = oracle.profile(level, blk)
    cap = B.sequence_bound(blk)
    # (a producer is registered, as on the workers' contexts, though ZSTD_compressSequences never calls it: with one, libzstd's validation
    # admits matches of 3 bytes at every level, which the chain levels' profiles produce)
    zc = zstd.cctx(level, producer=oracle.producer_addr, state=None, fallback=True, validate=True, checksumFlag=1 if checksum else 0)
    zstd.set(zc, 1008, 1)  # ZSTD_c_blockDelimiters = ZSTD_sf_explicitBlockDelimiters
    out = []
    try:
        dst = C.create_string_buffer(L.ZSTD_compressBound(chunk))
        for o in range(0, len(data), chunk):
            g = group_bytes(data[o:o + chunk], k, lib)
            seqs, start = [], 0
            for end in (group_blocks(len(g), k, lib) if cut is None else blocks_with_cuts(len(g), k, cut)):
                n, sq = oracle.find(prof, g[start:end], cap=cap)
                if n == B.SEQ_ERROR:
                    raise RuntimeError("the oracle failed a block")
                seqs += [(s.offset, s.litLength, s.matchLength, 0) for s in sq[:n]]
                start = end
                if counts is not None:
                    counts["blocks"] = counts.get("blocks", 0) + 1
                    counts["entries"] = counts.get("entries", 0) + n
            arr = (B.Sequence * max(len(seqs), 1))(*seqs)
            src = C.create_string_buffer(g, max(len(g), 1))
            L.ZSTD_CCtx_reset(zc, 1)  # ZSTD_reset_session_only
            r = L.ZSTD_compressSequences(zc, dst, len(dst), arr, len(seqs), src, len(g))
            if zstd.is_error(r):
                raise RuntimeError("ZSTD_compressSequences: " + zstd.err(r))
            out.append(dst.raw[:r])
    finally:
        zstd.free(zc)
    return out


def frame_header(n: int, checksum: bool = False) -> bytes:
    """magic and frame header of a frame the library writes itself: Single_Segment, the smallest Frame_Content_Size field that holds n"""
    code = 0 if n <= 255 else (1 if n <= 65791 else (2 if n <= 0xFFFFFFFF else 3))
    return b"\x28\xb5\x2f\xfd" + bytes([code << 6 | 0x20 | (4 if checksum else 0)]) + (n - 256 if code == 1 else n).to_bytes((1, 2, 4, 8)[code], "little")


def frame_blocks(frame: bytes) -> list:
    """the blocks of a zstd frame -> [(type, whole block: 3-byte header + body)], type 0 Raw, 1 RLE, 2 Compressed"""
    fhd = frame[4]
    single = (fhd >> 5) & 1
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + (single if fhd >> 6 == 0 else (0, 2, 4, 8)[fhd >> 6])
    out = []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        t = (h >> 1) & 3
        whole = 3 + (1 if t == 1 else h >> 3)
        out.append((t, frame[pos:pos + whole]))
        pos += whole
        if h & 1:
            return out


def reference_frames_probe(zstd, oracle, data: bytes, chunk: int, level: int, k: int, checksum: bool = False, lib=None,
                           counts: dict | None = None) -> list:
    """what the grouped device calls must produce with the plane probe on (QZSTD_frontSetPlaneProbe), the counterpart of
    reference_frames_grouped: per frame the ORACLE's sequences for each block of group_blocks, the rule of include/qzstd_planecost.h over
    each block's histogram and matched bytes, and libzstd.  A frame without a raw-predicted block — or with a plane of one value, or whose
    sub-frame fails or holds a block libzstd would store raw — is reference_frames_grouped's frame; every other frame is assembled: the
    library's frame header, a Raw_Block per raw-predicted block, and between them the blocks of ONE ZSTD_compressSequencesAndLiterals call
    over the remaining blocks' entries and literals, Last_Block on the frame's final block only; with `checksum` the four bytes libzstd
    appends to the same content.  counts: a dict that receives "blocks", "raw" (blocks written raw), "assembled", "allraw" (assembled
    without a libzstd call: every block raw) and "fallback" (frames),
    and "slack": the sum of (len >> 6) + 2 over the raw-predicted blocks of assembled frames"""
    L = zstd.lib
    L.ZSTD_compressSequencesAndLiterals.restype = C.c_size_t
    L.ZSTD_compressSequencesAndLiterals.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(B.Sequence), C.c_size_t, C.c_void_p, C.c_size_t,
                                                    C.c_size_t, C.c_size_t]
    blk = min(chunk, 131072)
    prof = oracle.profile(level, blk)
    cap = B.sequence_bound(blk)
    counts = counts if counts is not None else {}
    for key in ("blocks", "raw", "assembled", "allraw", "fallback", "slack"):
        counts.setdefault(key, 0)
    zc = zstd.cctx(level, producer=oracle.producer_addr, state=None, fallback=True, validate=False)
    zstd.set(zc, 1008, 1)  # ZSTD_c_blockDelimiters = ZSTD_sf_explicitBlockDelimiters
    out = []
    try:
        dst = C.create_string_buffer(L.ZSTD_compressBound(chunk))
        for o in range(0, len(data), chunk):
            piece = data[o:o + chunk]
            plain = reference_frames_grouped(zstd, oracle, piece, chunk, level, k, checksum=checksum, lib=lib)[0]
            g = group_bytes(piece, k, lib)
            blocks, start = [], 0
            for end in group_blocks(len(g), k, lib):
                b = g[start:end]
                n, sq = oracle.find(prof, b, cap=cap)
                if n == B.SEQ_ERROR:
                    raise RuntimeError("the oracle failed a block")
                ent = [(s.offset, s.litLength, s.matchLength, 0) for s in sq[:n]]
                lits, p = bytearray(), 0
                for _, ll, ml, _ in ent:
                    lits += b[p:p + ll]
                    p += ll + ml
                raw = plane_is_raw(plane_cost(b, lib), len(b), len(b) - len(lits), lib)
                blocks.append((b, ent, bytes(lits), raw))
                start = end
            counts["blocks"] += len(blocks)
            n_raw = sum(1 for b in blocks if b[3])
            if n_raw == 0:
                out.append(plain)
                continue
            maybe_rle = any(len(b[1]) < 5 and len(b[2]) < 10 for b in blocks[1:]) and k > 1
            sub = None
            if not maybe_rle and n_raw < len(blocks):
                ent = [e for b in blocks if not b[3] for e in b[1]]
                lit = b"".join(b[2] for b in blocks if not b[3])
                size = sum(len(b[0]) for b in blocks if not b[3])
                arr = (B.Sequence * len(ent))(*ent)
                lbuf = C.create_string_buffer(lit, len(lit) + 64)
                L.ZSTD_CCtx_reset(zc, 1)  # ZSTD_reset_session_only
                r = L.ZSTD_compressSequencesAndLiterals(zc, dst, len(dst), arr, len(ent), lbuf, len(lit), len(lit) + 64, size)
                if not zstd.is_error(r):
                    sub = frame_blocks(dst.raw[:r])
                    lens = [len(b[0]) for b in blocks if not b[3]]
                    if len(sub) != len(lens) or any(t == 2 and len(w) - 3 + (n >> 6) + 2 >= n for (t, w), n in zip(sub, lens)):
                        sub = None
            if maybe_rle or (sub is None and n_raw < len(blocks)):
                counts["fallback"] += 1
                out.append(plain)
                continue
            fr, it = bytearray(frame_header(len(g), checksum)), iter(sub or ())
            for i, (b, _, _, raw) in enumerate(blocks):
                last = 1 if i + 1 == len(blocks) else 0
                if raw:
                    fr += (len(b) << 3 | last).to_bytes(3, "little") + b
                    counts["slack"] += (len(b) >> 6) + 2
                else:
                    w = bytearray(next(it)[1])
                    w[0] = (w[0] & ~1) | last
                    fr += w
            if checksum:
                fr += plain[-4:]
            counts["raw"] += n_raw
            counts["assembled"] += 1
            counts["allraw"] += 1 if n_raw == len(blocks) else 0
            out.append(bytes(fr))
    finally:
        zstd.free(zc)
    return out


def bind_hufblock(H):
    """tests/hufblock/hufblock_check.c built -shared: include/qzstd_hufblock.h alone (hb_lengths, hb_streams, hb_size_word, hb_body, hb_takes)"""
    H.hb_lengths.restype = C.c_uint
    H.hb_lengths.argtypes = [C.c_char_p, C.c_uint, C.c_void_p]
    H.hb_streams.restype = C.c_size_t
    H.hb_streams.argtypes = [C.c_char_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t]
    H.hb_size_word.restype = C.c_uint
    H.hb_size_word.argtypes = [C.c_uint, C.c_uint]
    H.hb_body.restype = C.c_size_t
    H.hb_body.argtypes = [C.c_void_p, C.c_uint, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    H.hb_takes.restype = C.c_int
    H.hb_takes.argtypes = [C.c_uint] * 5
    H.hb_takes_at.restype = C.c_int
    H.hb_takes_at.argtypes = [C.c_uint] * 6
    H.hb_seq_eighths.restype = C.c_uint
    return H


def huf_block(huf, block: bytes, lit_bytes: int, count: int):
    """(size word, block body or None) of one block by include/qzstd_hufblock.h alone (huf: bind_hufblock): the size word qzstd_hip_huf_code
    leaves for it, and its QZSTD_hufBlockBody when QZSTD_hufTakes takes it given its compaction header's litBytes and count"""
    n = len(block)
    if not HUF_LEN_MIN <= n <= HUF_LEN_MAX:
        return 0, None
    nbits = (C.c_ubyte * 256)()
    if not huf.hb_lengths(block, n, nbits):
        return 0, None
    streams = C.create_string_buffer(n)
    size = huf.hb_size_word(huf.hb_streams(block, n, nbits, streams, n), n)
    if not size:
        return 0, None
    body = C.create_string_buffer(n + 256)
    b = huf.hb_body(nbits, n, streams.raw[:size], size, body, n + 256, 0)
    if not b or not huf.hb_takes(size, b, n, lit_bytes, count):
        return size, None
    return size, body.raw[:b]


def reference_frames_code(zstd, oracle, huf, data: bytes, chunk: int, level: int, k: int, checksum: bool = False, lib=None,
                          counts: dict | None = None) -> list:
    """what the grouped device calls must produce with the plane code on (QZSTD_frontSetPlaneCode), beside reference_frames_probe: per frame
    the ORACLE's sequences for each block, the probe's rule, and include/qzstd_hufblock.h alone (huf: bind_hufblock) for the size word, the
    block body and QZSTD_hufTakes.  A frame whose every block is raw-predicted or taken, one at least taken, is the library's frame header,
    a Raw_Block per raw-predicted block and a Compressed_Block of the body per taken one, with `checksum` the four bytes libzstd appends to
    the same content; every other frame is reference_frames_probe's.  counts receives reference_frames_probe's keys (a frame assembled here
    counts in "assembled", its raw blocks in "raw") and "coded" (blocks with a size word), "taken" (blocks), "nolib" (frames assembled
    without a libzstd call: these and the probe's all-raw ones), "code_fallback" (frames with a taken block that are the probe's)"""
    blk = min(chunk, 131072)
    prof = oracle.profile(level, blk)
    cap = B.sequence_bound(blk)
    counts = counts if counts is not None else {}
    for key in ("blocks", "raw", "assembled", "allraw", "fallback", "slack", "coded", "taken", "nolib", "code_fallback"):
        counts.setdefault(key, 0)
    out = []
    for o in range(0, len(data), chunk):
        piece = data[o:o + chunk]
        g = group_bytes(piece, k, lib)
        blocks, start = [], 0
        for end in group_blocks(len(g), k, lib):
            b = g[start:end]
            n, sq = oracle.find(prof, b, cap=cap)
            if n == B.SEQ_ERROR:
                raise RuntimeError("the oracle failed a block")
            lit_bytes = sum(s.litLength for s in sq[:n])
            raw = plane_is_raw(plane_cost(b, lib), len(b), len(b) - lit_bytes, lib)
            size, body = huf_block(huf, b, lit_bytes, n)
            counts["coded"] += 1 if size else 0
            blocks.append((b, raw, None if raw else body))
            start = end
        n_taken = sum(1 for b in blocks if b[2] is not None)
        if not n_taken or any(not raw and body is None for _, raw, body in blocks):
            sub = {}
            out.append(reference_frames_probe(zstd, oracle, piece, chunk, level, k, checksum=checksum, lib=lib, counts=sub)[0])
            for key, v in sub.items():
                counts[key] += v
            counts["nolib"] += sub["allraw"]
            counts["code_fallback"] += 1 if n_taken else 0
            continue
        fr = bytearray(frame_header(len(g), checksum))
        for i, (b, raw, body) in enumerate(blocks):
            last = 1 if i + 1 == len(blocks) else 0
            if raw:
                fr += (len(b) << 3 | last).to_bytes(3, "little") + b
                counts["slack"] += (len(b) >> 6) + 2
            else:
                fr += (len(body) << 3 | 2 << 1 | last).to_bytes(3, "little") + body
        if checksum:
            fr += reference_frames_grouped(zstd, oracle, piece, chunk, level, k, checksum=True, lib=lib)[0][-4:]
        counts["blocks"] += len(blocks)
        counts["raw"] += sum(1 for b in blocks if b[1])
        counts["assembled"] += 1
        counts["taken"] += n_taken
        counts["nolib"] += 1
        out.append(bytes(fr))
    return out
