"""CPU: QZSTD_frontFingerprintDeviceSlices, QZSTD_frontCheckDeviceSlices and QZSTD_frontVerifyDeviceSlices (include/qzstd_frontend_device.h)
over the mock device layer — the source-slices test's mock pair plus tests/mock/mock_hip_fingerprint_pieces.c and
mock_hip_ungroup_cmp_pieces.c.  The oracle is code that exists: every answer of a call whose buffers are lists of source slices, scattered
over "device" memory at every misalignment and in another order than the buffers', must be exactly what the contiguous call gives for the
same bytes held contiguously — fingerprints, the frame a check flags, the verify call's count and firstDiff[] — for that test's buffers,
element sizes, chunk sizes (16400, 100003) and cuttings (one, w1, w17, w2048, frame, random, empties; w1 narrowed to the buffers up to
2 x 16400 + 5 bytes as there), with frames from the slices call and from the Delta call alike, at levels 1 and 6, with checksum, plane probe
and delta skip off and on.  Also: one slice per buffer launch for launch the contiguous calls, the whole cycle on slices, every refusal with
nothing queued and nothing counted, and a device layer without the two new entry points.  Every comparison is exact.
The tests run in ONE child process (this file again, under pytest) and the suite's process only reads their outcomes: the module maps
some 60 MiB of "device" memory in arenas of the source-slices test's sizes, and where the kernel places the mappings of the modules that run
afterwards in the same process — and with it what happens to lie behind an arena's last byte there — must not depend on this one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import qz_bind as B
import qz_device as D
import test_device_checksum_mock as T
import test_device_slices_mock as S
import test_device_srcslices_mock as SS

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_slicecheckmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_slicecheckmock.so")
OLD_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nocheckpiecesmock.so")
OLD_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nocheckpiecesmock.so")
SIZES, ELEMS, BASED, CHUNKS, CUTTINGS, FILL = SS.SIZES, SS.ELEMS, SS.BASED, SS.CHUNKS, SS.CUTTINGS, SS.FILL
PLANT = (5, 300001 // 2 + 4321)  # (buffer, offset): inside a slice in the middle of a frame at both chunk sizes
CHILD = os.environ.get("QZ_SLICECHECK_CHILD") == "1"  # this process is the child: the tests run here
_outcomes = {}


def delegated() -> bool:
    """in the suite's process: asserts the running test's outcome in the child process (started once, for the whole module) and says that
    the caller is done; in the child: False, the test runs"""
    if CHILD:
        return False
    if not _outcomes:
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rA", "-p", "no:cacheprovider", os.path.abspath(__file__)], capture_output=True,
                             text=True, timeout=1500, cwd=T.ROOT, env=dict(os.environ, QZ_SLICECHECK_CHILD="1"))
        for line in out.stdout.splitlines():
            word, _, rest = line.partition(" ")
            if word in ("PASSED", "FAILED", "ERROR", "SKIPPED", "XFAIL", "XPASS") and "::" in rest:
                _outcomes[rest.split("::", 1)[1].split(" - ")[0].strip()] = word
        _outcomes["(output)"] = out.stdout[-6000:] + out.stderr[-2000:]
    name = os.environ["PYTEST_CURRENT_TEST"].split("::", 1)[1].rsplit(" (", 1)[0]
    assert _outcomes.get(name) == "PASSED", (name, _outcomes.get(name), _outcomes["(output)"])
    return True



def build_pair(zstd_path, mock_so, front_so, check_pieces: bool):
    """the source-slices test's mock pair (gather from pieces and extents included), with the two kernels from pieces or — an older device
    layer — without"""
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle"), "-I" + os.path.join(B.PKG_DIR, "frontend")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_bytegroup.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c", "mock_hip_fingerprint.c", "mock_hip_plane_cost.c",
                                             "mock_hip_group_pieces.c", "mock_hip_pointer_extent.c")]
    if check_pieces:
        srcs += [os.path.join(MOCK, "mock_hip_fingerprint_pieces.c"), os.path.join(MOCK, "mock_hip_ungroup_cmp_pieces.c")]
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


ULL_HOOKS = ("qzstd_mock_group_pieces_rows", "qzstd_mock_group_pieces_pieces", "qzstd_mock_diff_rows", "qzstd_mock_xxh64_rows",
             "qzstd_mock_plane_cost_rows", "qzstd_mock_gather_rows", "qzstd_mock_fingerprint_rows", "qzstd_mock_fingerprint_tiles",
             "qzstd_mock_ungroup_cmp_rows", "qzstd_mock_ungroup_cmp_zero_rows", "qzstd_mock_ungroup_cmp_stage_bytes",
             "qzstd_mock_fingerprint_pieces_rows", "qzstd_mock_fingerprint_pieces_pieces", "qzstd_mock_ungroup_cmp_pieces_rows",
             "qzstd_mock_ungroup_cmp_pieces_zero_rows", "qzstd_mock_ungroup_cmp_pieces_pieces")


@pytest.fixture(scope="module")
def chkmock(oracle, zstd):
    if not CHILD:
        return None, None
    build_pair(zstd.path, MOCK_SO, FRONT_SO, check_pieces=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    S.bind_hooks(plug)
    for n in ULL_HOOKS:
        getattr(plug.lib, n).restype = C.c_ulonglong
    return plug, F


@pytest.fixture(scope="module")
def world(chkmock):
    """the source-slices test's corpus: contiguous in one pool (the contiguous calls' input) and cut every way at both chunk sizes, built once"""
    plug, F = chkmock
    if not CHILD:
        return None
    datas, bases = SS.corpus()
    whole = SS.Arena(plug, 2 * sum(SIZES) + 4096, 0)
    bufs = [(whole.put(d, (5 * i + 1) % 16), len(d)) for i, d in enumerate(datas)]
    bbufs = [(whole.put(b, (3 * i + 2) % 16), len(b)) for i, b in enumerate(bases)]
    cases = {(name, chunk): SS.Case(plug, datas, bases, name, chunk, 1 + k) for k, (name, chunk) in
             enumerate((n, c) for c in CHUNKS for n in CUTTINGS)}
    return dict(datas=datas, bases=bases, bufs=bufs, bbufs=bbufs, cases=cases, whole=whole)


def counters(plug):
    L = plug.lib
    return dict(fp=L.qzstd_mock_fingerprint_launches(), fp_rows=L.qzstd_mock_fingerprint_rows(), fp_tiles=L.qzstd_mock_fingerprint_tiles(),
                cmp=L.qzstd_mock_ungroup_cmp_launches(), cmp_rows=L.qzstd_mock_ungroup_cmp_rows(), cmp_zero=L.qzstd_mock_ungroup_cmp_zero_rows(),
                cmp_stage=L.qzstd_mock_ungroup_cmp_stage_bytes(), fpp=L.qzstd_mock_fingerprint_pieces_launches(),
                fpp_rows=L.qzstd_mock_fingerprint_pieces_rows(), cmpp=L.qzstd_mock_ungroup_cmp_pieces_launches(),
                cmpp_rows=L.qzstd_mock_ungroup_cmp_pieces_rows(), cmpp_zero=L.qzstd_mock_ungroup_cmp_pieces_zero_rows(),
                waits=L.qzstd_mock_event_waits(), find=L.qzstd_mock_launches(), diff=L.qzstd_mock_diff_launches(),
                pieces=L.qzstd_mock_group_pieces_launches(), un=L.qzstd_mock_ungroup_launches(), unxor=L.qzstd_mock_ungroup_xor_launches())


def grown(a, b):
    return {k: ([y - x for x, y in zip(a[k], b[k])] if isinstance(a[k], list) else b[k] - a[k]) for k in a}


class Poke:
    """one byte of buffer `i` at offset `o` changed on both sides — in the slice that holds it (or in its base slice) and in the contiguous
    copy — for the length of a with block"""

    def __init__(self, world, case, i, o, base=False, bit=0x40):
        at = next(k for k, (b, off, s) in enumerate(case.flat) if b == i and s and off <= o < off + s)
        self.addrs = [(case.bas if base else case.src)[at] + (o - case.flat[at][1]), (world["bbufs"] if base else world["bufs"])[i][0] + o]
        self.bit = bit

    def flip(self):
        for a in self.addrs:
            c = C.c_ubyte.from_address(a)
            c.value ^= self.bit

    def __enter__(self):
        self.flip()

    def __exit__(self, *exc):
        self.flip()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_fingerprints_and_check_equal_the_contiguous_calls(chkmock, world, chunk):
    if delegated():
        return
    plug, F = chkmock
    fr = D.DeviceFront(2, 1, chunk, use_producer=0, lib=F)  # (a front without a producer serves the calls)
    host = C.create_string_buffer(64)
    try:
        s0, w0 = fr.fingerprint_stats(), counters(plug)
        want = fr.fingerprint(world["bufs"])
        s1, w1 = fr.fingerprint_stats(), counters(plug)
        assert [len(x) for x in want] == [-(-n // chunk) for n in SIZES]
        flat = [v for fp in want for v in fp]
        assert flat == [D.fingerprint_of(d[o:o + chunk], F) for d in world["datas"] for o in range(0, len(d), chunk)]
        hit = sum(-(-n // chunk) for n in SIZES[:PLANT[0]]) + PLANT[1] // chunk
        for name in CUTTINGS:
            case = world["cases"][(name, chunk)]
            # d_base is ignored: the compress call's list, a list without bases, and one whose bases are mixed and no device memory at all
            mixed = [(i, o, s, p, (C.addressof(host) if k % 2 else None)) for k, (i, o, s, p, _) in enumerate(case.slices(BASED))]
            multi = case.multi_frames(chunk)
            for sl in (case.slices(BASED), case.slices((False,) * len(SIZES)), mixed):
                c0, t0, p0, e0 = counters(plug), fr.fingerprint_stats(), fr.slice_check_stats(), plug.lib.qzstd_mock_extent_lookups()
                assert fr.fingerprint_slices(SIZES, sl) == want, name
                c1, t1, p1 = counters(plug), fr.fingerprint_stats(), fr.slice_check_stats()
                assert plug.lib.qzstd_mock_extent_lookups() - e0 == 1, name  # the slices lie in ONE allocation; no base is looked up
                assert [b - a for a, b in zip(t0, t1)] == [b - a for a, b in zip(s0, s1)], name
                assert [b - a for a, b in zip(p0, p1)] == [sum(1 for x in sl if x[2]), sum(SIZES), multi, 1 if multi else 0], name
                d = grown(c0, c1)
                assert (d["fpp"], d["fp"]) == ((1, 0) if multi else (0, 1)) and d["waits"] == grown(w0, w1)["waits"], name
                assert d["fpp_rows"] == (len(flat) if multi else 0) and d["cmp"] == d["cmpp"] == d["find"] == 0, name
            sl = case.slices(BASED)
            assert fr.check_slices_raw(SIZES, sl, flat) == (0, [0] * len(flat)), name
            with Poke(world, case, *PLANT):
                r, flags = fr.check_slices_raw(SIZES, sl, flat)
                assert r == 1 and flags == [int(c == hit) for c in range(len(flat))], name
                assert (r, flags) == fr.check_raw(world["bufs"], flat), name
                assert fr.check_slices_raw(SIZES, sl, flat, want_flags=False) == (1, None), name
            with Poke(world, case, *PLANT, base=True):  # a base is not part of a fingerprint
                assert fr.check_slices_raw(SIZES, sl, flat)[0] == 0, name
            assert case.arena.snapshot() == case.before, name  # the sources are only read
            if name == "one":
                assert multi == 0
            elif name in ("w17", "frame", "random"):
                assert multi > 0
    finally:
        fr.close()


@pytest.mark.parametrize("with_bases", (False, True), ids=("nobase", "bases"))
@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
@pytest.mark.parametrize("level", (1, 6))
@pytest.mark.parametrize("chunk", CHUNKS)
def test_verify_equals_the_contiguous_call(chkmock, world, monkeypatch, chunk, level, settings, with_bases):
    if delegated():
        return
    plug, F = chkmock
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    based = BASED if with_bases else (False,) * len(SIZES)
    given = [b if on else None for b, on in zip(world["bbufs"], based)]
    fr = D.DeviceFront(3, level, chunk, lib=F)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        frames = fr.compress_device_batch_delta(world["bufs"], given, ELEMS)
        assert fr.compress_device_slices(SIZES, ELEMS, world["cases"][("random", chunk)].slices(based)) == frames  # from either call alike
        n = sum(len(x) for x in frames)
        first = np.cumsum([0] + [len(x) for x in frames]).tolist()
        hit = first[PLANT[0]] + PLANT[1] // chunk
        s0 = fr.verify_stats()
        assert fr.verify_raw(frames, world["bufs"], given, ELEMS) == (0, [D.VERIFY_SAME] * n)
        s1 = fr.verify_stats()
        for name in CUTTINGS:
            case = world["cases"][(name, chunk)]
            sl = case.slices(based)
            c0, t0, p0 = counters(plug), fr.verify_stats(), fr.slice_check_stats()
            assert fr.verify_slices_raw(frames, SIZES, ELEMS, sl) == (0, [D.VERIFY_SAME] * n), name
            c1, t1, p1 = counters(plug), fr.verify_stats(), fr.slice_check_stats()
            assert [b - a for a, b in zip(t0, t1)] == [b - a for a, b in zip(s0, s1)], name
            multi = case.multi_frames(chunk)
            d, dp = grown(c0, c1), [b - a for a, b in zip(p0, p1)]
            assert dp[:3] == [sum(1 for x in sl if x[2]), sum(SIZES), multi] and dp[3] == d["cmpp"], name
            assert d["cmp"] + d["cmpp"] == t1[3] - t0[3] and (d["cmpp"] > 0) == (multi > 0) and d["fp"] == d["fpp"] == d["find"] == d["diff"] == 0, name
            if name == "one":
                assert d["cmpp"] == 0
            # one planted byte inside a slice in the middle of a frame, on the live side and on the base side
            for base in ((False, True) if with_bases else (False,)):
                with Poke(world, case, *PLANT, base=base):
                    got = fr.verify_slices_raw(frames, SIZES, ELEMS, sl)
                    assert got == fr.verify_raw(frames, world["bufs"], given, ELEMS), name
                    assert got == (1, [PLANT[1] % chunk if c == hit else D.VERIFY_SAME for c in range(n)]), name
            # (a planted byte in a buffer whose frames the skip recognises as zero frames: live against base, not decoded)
            with Poke(world, case, 3, 9000):
                z0 = counters(plug)
                got = fr.verify_slices_raw(frames, SIZES, ELEMS, sl)
                assert got == fr.verify_raw(frames, world["bufs"], given, ELEMS) and got[0] == 1 and got[1][first[3]] == 9000, name
                if settings and with_bases and multi:
                    assert grown(z0, counters(plug))["cmpp_zero"] >= 1, name
            if name in ("w2048", "random"):
                # a wrong base: buffer 4 against itself
                wrong = [(i, o, s, p, (p if i == 4 else b)) for i, o, s, p, b in sl]
                got = fr.verify_slices_raw(frames, SIZES, ELEMS, wrong)
                assert got == fr.verify_raw(frames, world["bufs"], [world["bufs"][4] if i == 4 else g for i, g in enumerate(given)], ELEMS), name
                assert got[0] >= 1
                # a swapped element size
                swapped = (2, 1, 4, 8, 4, 2)
                got = fr.verify_slices_raw(frames, SIZES, swapped, sl)
                assert got == fr.verify_raw(frames, world["bufs"], given, swapped) and got[0] >= 1, name
                # a corrupt frame
                bad = [list(x) for x in frames]
                bad[5][1] = bad[5][1][:len(bad[5][1]) // 2]  # (cut short: it does not decode, with a checksum or without)
                r, fd = fr.verify_slices_raw(bad, SIZES, ELEMS, sl)
                rw, fw = fr.verify_raw(bad, world["bufs"], given, ELEMS)
                assert r == rw == D.ERROR and fd[first[5] + 1] == fw[first[5] + 1] == D.VERIFY_UNDECODED, name
            assert case.arena.snapshot() == case.before, name
    finally:
        fr.close()


@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
def test_one_slice_per_buffer_queues_the_contiguous_calls_launches(chkmock, world, monkeypatch, settings):
    if delegated():
        return
    plug, F = chkmock
    chunk = CHUNKS[0]
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        for based in (BASED, (False,) * len(SIZES)):
            given = [b if on else None for b, on in zip(world["bbufs"], based)]
            frames = fr.compress_device_batch_delta(world["bufs"], given, ELEMS)
            one = [(i, 0, n, p, given[i][0] if given[i] else None) for i, (p, n) in enumerate(world["bufs"])]
            # slices that follow each other in memory are the buffer they are cut from
            cutup = [(i, o, min(1000, n - o), p + o, (given[i][0] + o) if given[i] else None) for i, (p, n) in enumerate(world["bufs"])
                     for o in range(0, n, 1000)]
            c0 = counters(plug)
            fp = fr.fingerprint_raw(world["bufs"])
            c1 = counters(plug)
            want = fr.verify_raw(frames, world["bufs"], given, ELEMS)
            c2 = counters(plug)
            for sl in (one, cutup):
                a = counters(plug)
                assert fr.fingerprint_slices_raw(SIZES, sl) == fp
                b = counters(plug)
                assert fr.verify_slices_raw(frames, SIZES, ELEMS, sl) == want
                c = counters(plug)
                assert grown(a, b) == grown(c0, c1) and grown(b, c) == grown(c1, c2)
                assert c["fpp"] == c0["fpp"] and c["cmpp"] == c0["cmpp"]
        assert fr.slice_check_stats()[2:] == [0, 0]
    finally:
        fr.close()


@pytest.mark.parametrize("name", ("w2048", "random", "empties"))
def test_cycle_on_slices(chkmock, world, name):
    """compress slices -> verify slices -> restore into a fresh scattered layout -> check slices: all 0"""
    if delegated():
        return
    plug, F = chkmock
    chunk = CHUNKS[1]
    case = world["cases"][(name, chunk)]
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        assert fr.set_delta_skip(1) == 0
        sl = case.slices(BASED)
        frames = fr.compress_device_slices(SIZES, ELEMS, sl)
        assert fr.verify_slices_raw(frames, SIZES, ELEMS, sl)[0] == 0
        fps = fr.fingerprint_slices(SIZES, sl)
        out = SS.Arena(plug, sum(SIZES) + 48 * len(case.flat) + 4096, 15)
        order = np.random.default_rng(7).permutation(len(case.flat)).tolist()
        dst = [0] * len(case.flat)
        for rank, at in enumerate(order):  # (another order in memory than the sources')
            s = case.flat[at][2]
            dst[at] = out.put(bytes(s), (3 * rank + 1) % 16) if s else 0
        back = [(i, o, s, dst[at], case.bas[at] if s and BASED[i] else None) for at, (i, o, s) in enumerate(case.flat)]
        assert fr.restore_slices(frames, SIZES, ELEMS, back) == sum(len(f) for f in frames)
        flat = [v for fp in fps for v in fp]
        assert fr.check_slices_raw(SIZES, back, flat) == (0, [0] * len(flat))
        assert fr.verify_slices_raw(frames, SIZES, ELEMS, back)[0] == 0
        C.c_ubyte.from_address(next(d for d in dst if d)).value ^= 1
        assert fr.check_slices_raw(SIZES, back, flat)[0] == 1
        plug.lib.qzstd_mock_device_range(15, None, 0, 0)
    finally:
        fr.close()


def test_refusals_queue_nothing_and_count_nothing(chkmock, world):
    if delegated():
        return
    plug, F = chkmock
    chunk = CHUNKS[0]
    case = world["cases"][("w2048", chunk)]
    good = case.slices(BASED)
    host = C.create_string_buffer(4096)  # (not registered: host memory)
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        frames = fr.compress_device_slices(SIZES, ELEMS, good)
        fps = [v for fp in fr.fingerprint_slices(SIZES, good) for v in fp]
        state = lambda: (counters(plug), fr.fingerprint_stats(), fr.verify_stats(), fr.slice_check_stats())  # noqa: E731

        def refused(sizes, slices, what, elems=ELEMS, fingerprints=True, verify=True):
            s0 = state()
            if fingerprints:
                assert fr.fingerprint_slices_raw(sizes, slices)[0] == D.ERROR, what
                assert fr.check_slices_raw(sizes, slices, fps)[0] == D.ERROR, what
            if verify:
                assert fr.verify_slices_raw(frames, sizes, elems, slices)[0] == D.ERROR, what
            assert state() == s0, what

        def change(at, **kw):
            names = ("buf", "offset", "size", "src", "base")
            out = list(good)
            out[at] = tuple(kw.get(n, v) for n, v in zip(names, good[at]))
            return out

        mid = next(at for at, x in enumerate(good) if x[0] == 5 and x[1] > 0)  # a slice in the middle of the largest buffer
        refused(None, good, "null bufSizes")
        bs = (C.c_size_t * 6)(*SIZES)
        s0 = state()
        assert F.QZSTD_frontFingerprintDeviceSlices(fr.f, bs, 6, None, 3, None, (C.c_ulonglong * 64)(), None) == D.ERROR  # null slices with a count
        assert F.QZSTD_frontCheckDeviceSlices(fr.f, bs, 6, None, 3, None, (C.c_ulonglong * 64)(), len(fps), None) == D.ERROR
        assert state() == s0
        refused(SIZES, change(mid, buf=len(SIZES)), "buf >= nBufs")
        refused(SIZES, good[:mid] + [good[mid + 1], good[mid]] + good[mid + 2:], "out of order")
        refused(SIZES, list(reversed(good)), "buffers out of order")
        refused(SIZES, good[:mid] + good[mid + 1:], "a gap")
        refused(SIZES, good[:mid] + [good[mid]] + good[mid:], "an overlap")
        refused(SIZES, change(mid, offset=good[mid][1] - 1), "an overlap by one byte")
        refused(SIZES, change(len(good) - 1, size=good[-1][2] + 1), "an end past its buffer")
        refused(SIZES, good[:-1], "a buffer that ends short")
        refused(SIZES, good + [(5, SIZES[5] + 1, 0, 0, None)], "an empty slice past its buffer")
        refused(SIZES, change(mid, src=0), "null d_src")
        refused(SIZES, change(mid, src=C.addressof(host)), "a source in host memory")
        refused(SIZES, change(mid, src=case.arena.base + case.arena.size - 10), "a source whose last byte is not device memory")
        plug.lib.qzstd_mock_device_range(14, C.addressof(host), 4096, 1)  # another device
        refused(SIZES, change(mid, src=C.addressof(host)), "a source on another device")
        last = world["cases"][("empties", CHUNKS[1])].arena  # (slot 14 is this case's again)
        plug.lib.qzstd_mock_device_range(14, last.base, last.size, 0)
        # the verify call alone: bases count there, and element sizes
        refused(SIZES, change(mid, base=None), "based and unbased slices in one buffer", fingerprints=False)
        refused(SIZES, change(mid, base=C.addressof(host)), "a base in host memory", fingerprints=False)
        refused(SIZES, good, "QZSTD_ELEM_DIFF", elems=(2, 1, 4, 8, 2, 4 | D.ELEM_DIFF), fingerprints=False)
        refused(SIZES, good, "element size 3", elems=(2, 1, 3, 8, 2, 4), fingerprints=False)
        s0 = state()
        assert fr.verify_slices_raw(frames, SIZES, ELEMS, good, n_frames=len(fps) - 1)[0] == D.ERROR  # the nFrames rule
        assert fr.verify_slices_raw(frames[:-1] + [frames[-1][:-1]], SIZES, ELEMS, good)[0] == D.ERROR
        # the fingerprint calls alone
        assert fr.fingerprint_slices_raw(SIZES, good, null_fp=True)[0] == D.ERROR
        assert fr.check_slices_raw(SIZES, good, None, n_frames=len(fps))[0] == D.ERROR
        assert fr.check_slices_raw(SIZES, good, fps, n_frames=len(fps) - 1)[0] == D.ERROR
        assert fr.check_slices_raw(SIZES, good, fps[:-1])[0] == D.ERROR
        arr = fr.src_slice_array(good)
        assert F.QZSTD_frontFingerprintDeviceSlices(None, bs, 6, arr, len(good), None, (C.c_ulonglong * 64)(), None) == D.ERROR
        assert F.QZSTD_frontCheckDeviceSlices(None, bs, 6, arr, len(good), None, (C.c_ulonglong * 64)(*fps), len(fps), None) == D.ERROR
        assert F.QZSTD_frontVerifyDeviceSlices(None, None, 0, None, 0, bs, bytes(ELEMS), 6, arr, len(good), None, None) == D.ERROR
        assert state() == s0
        st = (C.c_ulonglong * 4)(9, 9, 9, 9)
        F.QZSTD_frontSliceCheckStats(None, st)
        assert list(st) == [0, 0, 0, 0]
        F.QZSTD_frontSliceCheckStats(fr.f, None)
        # no buffers, and only empty ones: 0, no GPU touched
        c0 = counters(plug)
        assert fr.fingerprint_slices_raw([], [])[0] == 0 and fr.fingerprint_slices_raw([0, 0], [(1, 0, 0, 0, None)])[0] == 0
        assert fr.check_slices_raw([0, 0], [(1, 0, 0, 0, None)], [])[0] == 0
        assert fr.verify_slices_raw([[], []], [0, 0], [2, 4], [(1, 0, 0, 0, None)])[0] == 0 and fr.verify_slices_raw([], [], [], [])[0] == 0
        assert counters(plug) == c0
        # and the good list is served
        assert fr.check_slices_raw(SIZES, good, fps)[0] == 0 and fr.verify_slices_raw(frames, SIZES, ELEMS, good)[0] == 0
    finally:
        fr.close()


def test_the_launchers_checks_in_the_mocks(chkmock):
    """the two mocks' own refusals, before anything is touched: a piece table that does not tile its row, and a base in the fingerprint's"""
    if delegated():
        return
    plug, F = chkmock
    L = D.bind_check_pieces_kernels(plug.lib)
    data = C.create_string_buffer(bytes(range(100)), 100)
    a = C.addressof(data)

    def table(cuts):
        pieces = (D.GroupPiece * len(cuts))()
        for p, (off, ln, so, base) in zip(pieces, cuts):
            p.src, p.base, p.off, p.len = (a + so if so is not None else 0), base, off, ln
        return pieces

    def fp(cuts, ln, np_=None):
        pieces, rows = table(cuts), (D.FpPiecesRow * 1)()
        rows[0].len, rows[0].tile0, rows[0].piece0, rows[0].nPieces = ln, 77, 0, len(cuts) if np_ is None else np_
        out = (C.c_uint64 * 4)(5, 5, 5, 5)
        rc = L.qzstd_hip_fingerprint_pieces(0, None, rows, 1, (D.FpPiecesRow * 1)(), pieces, len(cuts), (D.GroupPiece * len(cuts))(), out)
        return rc, rows[0].tile0, list(out)

    def cmp_(cuts, ln, k=2, flags=D.CMP_ZERO):
        pieces, rows = table(cuts), (D.UngroupCmpPiecesRow * 1)()
        rows[0].srcOff, rows[0].len, rows[0].elem, rows[0].flags, rows[0].tile0, rows[0].piece0, rows[0].nPieces = 0, ln, k, flags, 77, 0, len(cuts)
        out = (C.c_uint32 * 4)(5, 5, 5, 5)
        rc = L.qzstd_hip_ungroup_cmp_pieces(0, None, rows, 1, (D.UngroupCmpPiecesRow * 1)(), pieces, len(cuts), (D.GroupPiece * len(cuts))(), None, 0, out)
        return rc, rows[0].tile0, list(out)

    three = [(0, 1, 50, 0), (1, 60, 0, 0), (61, 39, 61, 0)]
    content = bytes(range(100))[50:51] + bytes(range(100))[0:60] + bytes(range(100))[61:100]
    assert fp(three, 100) == (0, 0, [D.fp_tile_ref(content), 5, 5, 5])
    assert cmp_(three, 100) == (0, 0, [0, 5, 5, 5])  # (a ZERO row against the bytes: byte 0 is 50)
    bad = {"a gap": [(0, 1, 50, 0), (2, 59, 0, 0), (61, 39, 61, 0)], "an overlap": [(0, 2, 50, 0), (1, 60, 0, 0), (61, 39, 61, 0)],
           "short": three[:2], "an empty piece": [(0, 1, 50, 0), (1, 0, 0, 0), (1, 60, 0, 0), (61, 39, 61, 0)],
           "a null source": [(0, 1, 50, 0), (1, 60, None, 0), (61, 39, 61, 0)]}
    for name, cuts in bad.items():
        assert fp(cuts, 100) == (-1, 77, [5, 5, 5, 5]), name
        assert cmp_(cuts, 100) == (-1, 77, [5, 5, 5, 5]), name
    assert fp(three, 100, np_=4) == (-1, 77, [5, 5, 5, 5])
    assert fp([(0, 1, 50, 0), (1, 60, 0, a), (61, 39, 61, 0)], 100) == (-1, 77, [5, 5, 5, 5])  # a base: refused, nothing queued
    assert cmp_([(0, 1, 50, 0), (1, 60, 0, a), (61, 39, 61, 0)], 100)[0] == 0                  # (no value of a base is refused there)
    assert cmp_(three, 100, k=3)[0] == -1 and cmp_(three, 100, flags=2)[0] == -1 and cmp_(three, 100, flags=0)[0] == -1  # (no stage)


def test_device_layer_without_the_two_entry_points(zstd, oracle):
    """the front-end linked against a mock WITHOUT the two new sources: a call with a frame of several pieces returns (size_t)-1 with no
    launch, no event wait and nothing counted; a call in which every frame lies in one piece, and the contiguous calls, are served (a
    process of its own)"""
    if delegated():
        return
    build_pair(zstd.path, OLD_MOCK_SO, OLD_FRONT_SO, check_pieces=False)
    res = T.run_child("""
chunk = 16400
n = 3 * chunk + 321
data = D.typed_corpus("bf16", n, 1)
base = D.typed_corpus("bf16", n, 2)
pool = T.Pool(plug, [data, data[:chunk], data[chunk:2 * chunk + 7], data[2 * chunk + 7:]], [0, 3, 9, 6], slot=0)
bas = T.Pool(plug, [base, base[:chunk], base[chunk:2 * chunk + 7], base[2 * chunk + 7:]], [5, 1, 0, 2], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
frames = fr.compress_device_batch_delta(pool.bufs[:1], bas.bufs[:1], [2])
fp = fr.fingerprint_raw(pool.bufs[:1])
ver = fr.verify_raw(frames, pool.bufs[:1], bas.bufs[:1], [2])
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_fingerprint_launches(), plug.lib.qzstd_mock_ungroup_cmp_launches(),
                 fr.fingerprint_stats(), fr.verify_stats(), fr.slice_check_stats())
before = state()
cut = [(0, 0, chunk, pool.bufs[1][0], bas.bufs[1][0]), (0, chunk, chunk + 7, pool.bufs[2][0], bas.bufs[2][0]),
       (0, 2 * chunk + 7, n - 2 * chunk - 7, pool.bufs[3][0], bas.bufs[3][0])]
r = [fr.fingerprint_slices_raw([n], cut)[0], fr.check_slices_raw([n], cut, fp[1])[0], fr.verify_slices_raw(frames, [n], [2], cut)[0]]
nothing = state() == before
whole = [(0, 0, n, pool.bufs[0][0], bas.bufs[0][0])]
one = fr.fingerprint_slices_raw([n], whole) == fp and fr.check_slices_raw([n], whole, fp[1])[0] == 0 and fr.verify_slices_raw(frames, [n], [2], whole) == ver
pool2 = T.Pool(plug, [data[:2 * chunk], data[2 * chunk:]], [7, 4], slot=2)
bas2 = T.Pool(plug, [base[:2 * chunk], base[2 * chunk:]], [2, 11], slot=3)
at = [(0, 0, 2 * chunk, pool2.bufs[0][0], bas2.bufs[0][0]), (0, 2 * chunk, n - 2 * chunk, pool2.bufs[1][0], bas2.bufs[1][0])]
at_frames = fr.fingerprint_slices_raw([n], at) == fp and fr.verify_slices_raw(frames, [n], [2], at) == ver
print(json.dumps({"refused": r == [D.ERROR] * 3, "nothing_queued": nothing, "one_slice": one, "cut_at_frames": at_frames,
                  "contiguous": fr.fingerprint_raw(pool.bufs[:1]) == fp and fr.verify_raw(frames, pool.bufs[:1], bas.bufs[:1], [2]) == ver,
                  "has_entry_points": hasattr(plug.lib, "qzstd_hip_fingerprint_pieces") or hasattr(plug.lib, "qzstd_hip_ungroup_cmp_pieces")}))
""", OLD_MOCK_SO, OLD_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "one_slice": True, "cut_at_frames": True, "contiguous": True,
                   "has_entry_points": False}, res
