"""The announcement batcher (host/qatseqprod.c: QZSTD_Batcher_T) over the mock HIP layer: announced block ranges of every state go into
a few device-wide launches on the batcher's own streams, instead of one launch per announcement.  Frames stay libzstd's frames from the
oracle's sequences; launches are counted by the mock (qzstd_mock_launches) and by the batcher (qzstd_test_hint_launches)."""
import ctypes as C
import threading
import time

import qz_bind as B
import qz_corpus as K
from test_host_mock import fail_stats, frames_of, mock, oracle_frames, restarted, stats_of  # noqa: F401 (mock: the fixture)

CHUNK = 131072


def _lib(mock):
    L = mock.lib
    L.QZSTD_hintSourceEx.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_uint]
    L.qzstd_test_hint_launches.restype = C.c_ulong
    L.qzstd_test_orphans.restype = C.c_ulong
    L.qzstd_mock_stall_ms.argtypes = [C.c_int]
    L.qzstd_mock_launches_on.argtypes = [C.c_int]
    return L


def _announce_and_compress(mock, zstd, L, st, buf, off, size, level, chunk=CHUNK, stable=1):
    assert L.QZSTD_hintSourceEx(st, C.byref(buf, off), size, chunk, level, stable) == 0
    return frames_of(zstd, mock.producer_addr, st, C.addressof(buf) + off, size, chunk, level)


def test_many_states_announcing_at_once_share_launches(mock, zstd, oracle):
    """eight threads, one state each, announce 1 MiB claims two ahead of what they compress (the batch front-end's shape) on one batch
    stream: claims that arrive while a launch is being queued collect in the open batch and go out together.  Every frame is the oracle's,
    every block comes from an announcement, and there are far fewer launches than claims"""
    L = _lib(mock)
    threads, claims, claim = 8, 6, 8 * CHUNK
    data = K.by_name("system", threads * claims * claim, seed=71)
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    want = oracle_frames(zstd, oracle, data, CHUNK, 1)
    got, stats, errors = {}, {}, []

    def worker(t):
        try:
            st = L.QZSTD_createSeqProdState()
            base = t * claims * claim
            for c in range(2):
                assert L.QZSTD_hintSourceEx(st, C.byref(buf, base + c * claim), claim, CHUNK, 1, 1) == 0
            for c in range(claims):
                if c + 2 < claims:
                    assert L.QZSTD_hintSourceEx(st, C.byref(buf, base + (c + 2) * claim), claim, CHUNK, 1, 1) == 0
                fr = frames_of(zstd, mock.producer_addr, st, C.addressof(buf) + base + c * claim, claim, CHUNK, 1)
                for k, f in enumerate(fr):
                    got[(base + c * claim) // CHUNK + k] = f
            stats[t] = (stats_of(mock, st), fail_stats(mock, st))
            L.QZSTD_freeSeqProdState(st)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    with restarted(mock, QZSTD_HIP_HINT_BATCHES="1"):
        l0, h0 = L.qzstd_mock_launches(), L.qzstd_test_hint_launches()
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        launches, hint_launches = L.qzstd_mock_launches() - l0, L.qzstd_test_hint_launches() - h0
    assert not errors, errors
    assert [got[i] for i in range(len(want))] == want
    for t in range(threads):
        (served, fs) = stats[t]
        assert served[0] == claims * 8 and served[1] == 0 and fs[0] == 0, (t, served, fs)
    assert launches == hint_launches  # (nothing else launched: no block took the per-block path)
    assert launches <= threads * claims // 2, "%d launches for %d claims" % (launches, threads * claims)


def _blocker(mock, L, data_len=4 * CHUNK):
    """a state whose announcement is launched while the mock device is stalled: its blocks never publish, so the stream it went to is
    not free again (count words) until the announcement is dropped and its wait times out"""
    blk = (C.c_char * data_len).from_buffer_copy(K.by_name("mix", data_len, seed=3))
    st = L.QZSTD_createSeqProdState()
    L.qzstd_mock_stall_ms(80)
    assert L.QZSTD_hintSourceEx(st, blk, data_len, CHUNK, 1, 1) == 0
    time.sleep(0.1)  # the stall is over; the blocker's launch stays unpublished
    return st, blk


def test_hint_dropped_while_its_part_waits_in_an_unissued_batch(mock, zstd, oracle):
    """the only batch stream is held by a launch that never publishes: a new announcement collects in the open batch.  Dropping it
    (QZSTD_dropHints) issues that batch behind the busy stream and waits for it; nothing strands, the areas are reused afterwards"""
    L = _lib(mock)
    data = K.by_name("system", 8 * CHUNK, seed=72)
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    want = oracle_frames(zstd, oracle, data, CHUNK, 1)
    with restarted(mock, QZSTD_HIP_HINT_BATCHES="1", QZSTD_HIP_TIMEOUT_MS="300"):
        sb, _keep = _blocker(mock, L)
        h0 = L.qzstd_test_hint_launches()
        st = L.QZSTD_createSeqProdState()
        assert L.QZSTD_hintSourceEx(st, buf, len(data), CHUNK, 1, 1) == 0
        assert L.qzstd_test_hint_launches() == h0  # collecting: the stream's last launch has not published
        L.QZSTD_dropHints(st)
        assert L.qzstd_test_hint_launches() == h0 + 1  # the drop issued it
        got = _announce_and_compress(mock, zstd, L, st, buf, 0, len(data), 1)  # (a callback issues a collecting batch itself, too)
        served, fs = stats_of(mock, st), fail_stats(mock, st)
        L.QZSTD_freeSeqProdState(st)
        L.QZSTD_freeSeqProdState(sb)  # the blocker's wait times out: its batch area is parked
    assert got == want
    assert served[0] == 8 and served[1] == 0 and fs[0] == 0, (served, fs)


def test_stalled_merged_launch_sends_every_part_to_the_per_block_path(mock, zstd, oracle):
    """two states' announcements collect in one batch behind a busy stream and go out as ONE launch that stalls: the first callback's
    wait times out, which fails every part of that batch — the other state does not wait again, its blocks take the per-block path.
    Frames are the oracle's; the batch's area is parked, not reused"""
    L = _lib(mock)
    a, b = K.by_name("system", 4 * CHUNK, seed=73), K.by_name("mix", 4 * CHUNK, seed=74)
    ba, bb = (C.c_char * len(a)).from_buffer_copy(a), (C.c_char * len(b)).from_buffer_copy(b)
    wa, wb = oracle_frames(zstd, oracle, a, CHUNK, 3), oracle_frames(zstd, oracle, b, CHUNK, 3)
    with restarted(mock, QZSTD_HIP_HINT_BATCHES="1", QZSTD_HIP_TIMEOUT_MS="60", QZSTD_HIP_SERVICE="0"):
        sb, _keep = _blocker(mock, L)
        o0, h0 = L.qzstd_test_orphans(), L.qzstd_test_hint_launches()
        s1, s2 = L.QZSTD_createSeqProdState(), L.QZSTD_createSeqProdState()
        assert L.QZSTD_hintSourceEx(s1, ba, len(a), CHUNK, 3, 1) == 0
        assert L.QZSTD_hintSourceEx(s2, bb, len(b), CHUNK, 3, 1) == 0
        assert L.qzstd_test_hint_launches() == h0
        L.qzstd_mock_stall_ms(400)
        try:
            seqs = (B.Sequence * B.sequence_bound(CHUNK))()
            # issues the merged batch (stalled: never publishes) and times out; the block goes to the per-block path (stalled too: the error
            # code, or its sequences once the stall is over)
            L.qatSequenceProducer(s1, seqs, len(seqs), ba, CHUNK, None, 0, 3, 1 << 17)
            assert stats_of(mock, s1)[0] == 0
            assert L.qzstd_test_hint_launches() == h0 + 1  # ONE launch for both announcements
        finally:
            L.qzstd_mock_stall_ms(0)
        got2 = frames_of(zstd, mock.producer_addr, s2, C.addressof(bb), len(b), CHUNK, 3)
        got1 = frames_of(zstd, mock.producer_addr, s1, C.addressof(ba), len(a), CHUNK, 3)
        st1, st2 = stats_of(mock, s1), stats_of(mock, s2)
        for s in (s1, s2, sb):
            L.QZSTD_freeSeqProdState(s)
        assert L.qzstd_test_orphans() >= o0 + 1
    assert got1 == wa and got2 == wb
    assert st1[0] == 0 and st2[0] == 0 and st2[1] == 4, (st1, st2)


def test_state_freed_with_parts_in_flight(mock, zstd, oracle):
    """states freed right after announcing (parts collecting or in flight) wait for their parts and let go of the areas: announcements
    of other states keep working on the same areas, frames are the oracle's"""
    L = _lib(mock)
    data = K.by_name("system", 16 * CHUNK, seed=75)
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    want = oracle_frames(zstd, oracle, data, CHUNK, 1)
    errors = []

    def churn(t):
        try:
            for _ in range(12):
                st = L.QZSTD_createSeqProdState()
                assert L.QZSTD_hintSourceEx(st, buf, 8 * CHUNK, CHUNK, 1, 1) == 0
                assert L.QZSTD_hintSourceEx(st, C.byref(buf, 8 * CHUNK), 8 * CHUNK, CHUNK, 1, 1) == 0
                L.QZSTD_freeSeqProdState(st)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    with restarted(mock, QZSTD_HIP_HINT_BATCHES="2"):
        ths = [threading.Thread(target=churn, args=(t,)) for t in range(6)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        st = L.QZSTD_createSeqProdState()
        got = _announce_and_compress(mock, zstd, L, st, buf, 0, len(data), 1)
        served = stats_of(mock, st)
        L.QZSTD_freeSeqProdState(st)
    assert not errors, errors
    assert got == want and served[0] == 16 and served[1] == 0, served


def test_mixed_levels_in_one_batch(mock, zstd, oracle):
    """a level-1 announcement collects in the open batch; a level-3 one arrives: one launch is one level, so the level-1 batch goes out
    as it is and the level-3 blocks open the next one.  Both states' frames are the oracle's, every block from an announcement"""
    L = _lib(mock)
    a, b = K.by_name("system", 6 * CHUNK, seed=76), K.by_name("mix", 5 * CHUNK + 999, seed=77)
    ba, bb = (C.c_char * len(a)).from_buffer_copy(a), (C.c_char * len(b)).from_buffer_copy(b)
    with restarted(mock, QZSTD_HIP_HINT_BATCHES="1", QZSTD_HIP_TIMEOUT_MS="300"):
        sb, _keep = _blocker(mock, L)
        h0 = L.qzstd_test_hint_launches()
        s1, s3 = L.QZSTD_createSeqProdState(), L.QZSTD_createSeqProdState()
        assert L.QZSTD_hintSourceEx(s1, ba, len(a), CHUNK, 1, 1) == 0
        assert L.qzstd_test_hint_launches() == h0
        assert L.QZSTD_hintSourceEx(s3, bb, len(b), CHUNK, 3, 1) == 0
        # the level-1 batch went out when level 3 came, and the level-3 one behind it (the mock's launch published at once: a free stream)
        assert L.qzstd_test_hint_launches() == h0 + 2
        got1 = frames_of(zstd, mock.producer_addr, s1, C.addressof(ba), len(a), CHUNK, 1)
        got3 = frames_of(zstd, mock.producer_addr, s3, C.addressof(bb), len(b), CHUNK, 3)
        assert L.qzstd_test_hint_launches() == h0 + 2
        st1, st3 = stats_of(mock, s1), stats_of(mock, s3)
        for s in (s1, s3, sb):
            L.QZSTD_freeSeqProdState(s)
    assert got1 == oracle_frames(zstd, oracle, a, CHUNK, 1) and got3 == oracle_frames(zstd, oracle, b, CHUNK, 3)
    assert st1[:2] == [6, 0] and st3[:2] == [6, 0], (st1, st3)


def test_split_over_two_devices_goes_to_each_devices_batcher(mock, zstd, oracle):
    """QZSTD_HIP_SPLIT over two mock GPUs: every announcement is cut in two ranges, each staged into its own GPU's batcher; four states
    at once, three claims announced ahead each.  Both GPUs launch, each in at most two thirds as many launches as ranges it got (3 – 5 of
    12 measured), frames are the oracle's, every block from an announcement"""
    L = _lib(mock)
    states, claim = 4, 8 * CHUNK
    data = K.by_name("system", states * 3 * claim, seed=78)
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    want = oracle_frames(zstd, oracle, data, CHUNK, 1)
    got, served, errors = {}, {}, []

    def worker(t):
        try:
            st = L.QZSTD_createSeqProdState()
            for c in range(3):  # (three claims announced ahead, as the front-end does)
                assert L.QZSTD_hintSourceEx(st, C.byref(buf, (t * 3 + c) * claim), claim, CHUNK, 1, 1) == 0
            for c in range(3):
                off = (t * 3 + c) * claim
                fr = frames_of(zstd, mock.producer_addr, st, C.addressof(buf) + off, claim, CHUNK, 1)
                for k, f in enumerate(fr):
                    got[off // CHUNK + k] = f
            served[t] = stats_of(mock, st)
            L.QZSTD_freeSeqProdState(st)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    with restarted(mock, QZSTD_MOCK_DEVICES="2", QZSTD_HIP_HINT_BATCHES="1"):
        before = [L.qzstd_mock_launches_on(d) for d in range(2)]
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(states)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        per_dev = [L.qzstd_mock_launches_on(d) - before[d] for d in range(2)]
    assert not errors, errors
    assert [got[i] for i in range(len(want))] == want
    assert all(s[:2] == [24, 0] for s in served.values()), served
    # every announcement is one range per device: states * 3 ranges went to each device's batcher, in clearly fewer launches
    assert all(0 < n <= 2 * states * 3 // 3 for n in per_dev), (per_dev, states * 3)
