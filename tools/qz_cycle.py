"""The checkpoint cycle as ONE function over either device layer (tests/test_device_cycle_mock.py: the mock; tests/test_gpu_device_cycle.py:
the real library and kernels): fingerprint the live buffers, QZSTD_frontCompressDeviceBatchDelta with the settings given, restore into fresh
buffers and in place over copies of the bases, restore slices, verify, check the fingerprints (include/qzstd_frontend_device.h) — at ANY
chunk size, with checksum, plane probe and delta skip in any combination, at any level.  Every comparison is byte-exact.

Buffers per chunk size C (buffers()): element sizes 1, 2, 4, 8 (text, bf16, fp32, ids64), sizes 0, 1, k + 1, C - 1, C, C + 1, 2 C + k + 1 each,
bases of five kinds spread over them (BASE_KIND): none, identical, one element of a middle frame differs, only the last byte differs, a
second draw.  Every buffer, base and destination lies at an odd offset of a 16-byte line, the three at different ones.

`mem` is the device memory: HostMem (host memory the mock treats as device memory) or TorchMem (a torch byte tensor).  It keeps a SHADOW of
the whole arena on the host — what the arena must hold — so that "exactly these bytes were written and nothing else" is one comparison of
the arena with the shadow: destinations, the 0xA5 guards between them, and the inputs every call must leave alone."""
import collections
import ctypes as C

import numpy as np

import qz_bind as B
import qz_corpus as K
import qz_device as D

GUARD = 64
FILL = 0xA5
TILE = 16384
KIND = {1: "text", 2: "bf16", 4: "fp32", 8: "ids64"}
# per element size, for the sizes 0, 1, k + 1, C - 1, C, C + 1, 2 C + k + 1: what the buffer's base is.  (A changed chunk that all but equals
# its base is a delta of zeros, the costliest content there is for the chain levels' match-finder — the oracle's and the mock's — so only
# two large buffers are of that kind: text "middle", with an equal chunk on either side of the changed one, and ids64 "last".)
BASE_KIND = {
    1: ("identical", "identical", "last", "none", "identical", "draw", "middle"),
    2: ("none", "last", "middle", "identical", "draw", "last", "none"),
    4: ("none", "last", "middle", "none", "draw", "identical", "draw"),
    8: ("identical", "none", "identical", "draw", "last", "middle", "identical"),
}
# (chunk sizes, levels, (checksum, probe, skip) settings): the matrix both test modules run
_ALL = [(c, p, s) for c in (False, True) for p in (False, True) for s in (False, True)]
MATRIX = [(chunk, 1, st) for chunk in (4080, 16400, 300001) for st in ((False, False, False), (True, True, True))]
MATRIX += [(chunk, 1, st) for chunk in (100003, 393216) for st in _ALL]
MATRIX += [(chunk, level, (True, True, True)) for chunk in (100003, 393216) for level in (6, 12)]


def case_id(case) -> str:
    chunk, level, (checksum, probe, skip) = case
    on = "+".join(n for n, v in (("checksum", checksum), ("probe", probe), ("skip", skip)) if v)
    return "%d-l%d-%s" % (chunk, level, on or "off")


def sizes_of(chunk: int, k: int) -> tuple:
    return (0, 1, k + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + k + 1)


Buf = collections.namedtuple("Buf", "k kind data base")  # base: bytes of the data's length, or None


_text = {}


def _draw(k: int, n: int, seed: int, most: int) -> bytes:
    """n bytes of the element size's corpus; text as a prefix of ONE draw of `most` bytes per seed (its vocabulary is costly to build)"""
    if k != 1:
        return D.typed_corpus(KIND[k], n, seed)
    if (seed, most) not in _text:
        if len(_text) >= 4:
            _text.pop(next(iter(_text)))
        _text[(seed, most)] = K.by_name("text", most, seed=seed)
    return _text[(seed, most)][:n]


def _base(kind: str, d: bytes, k: int, chunk: int, n_draw: bytes):
    if kind == "none":
        return None
    b = np.frombuffer(d, dtype=np.uint8).copy()
    n = len(b)
    if kind == "draw":
        return n_draw
    if kind == "last" and n:
        b[n - 1] ^= 0x40
    if kind == "middle" and n:  # one element of the middle frame (a frame shorter than an element: all of it)
        c = -(-n // chunk) // 2
        p = c * chunk + (min(chunk, n - c * chunk) // 2) // k * k
        b[p:min(p + k, n)] ^= 0x5A
    return b.tobytes()


_buffers = {}


def buffers(chunk: int) -> list:
    """the cycle's buffers for a chunk size, computed once per size and never changed"""
    if chunk not in _buffers:
        if len(_buffers) >= 2:
            _buffers.pop(next(iter(_buffers)))
        out = []
        for k in (1, 2, 4, 8):
            for n, kind in zip(sizes_of(chunk, k), BASE_KIND[k]):
                d = _draw(k, n, 3, 2 * chunk + 2)
                out.append(Buf(k, kind, d, _base(kind, d, k, chunk, _draw(k, n, 4, 2 * chunk + 2))))
        _buffers[chunk] = out
    return _buffers[chunk]


def chunks(d: bytes, chunk: int) -> list:
    return [d[o:o + chunk] for o in range(0, len(d), chunk)]


def xor(a: bytes, b: bytes) -> bytes:
    return (np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes()


def ungroup(b: bytes, k: int) -> bytes:
    """the byte-grouped layout undone in numpy (include/qzstd_bytegroup.h restated): k planes of len // k bytes, then the tail"""
    a = np.frombuffer(b, dtype=np.uint8)
    m = len(a) // k
    return np.concatenate([a[:m * k].reshape(k, m).T.reshape(-1), a[m * k:]]).tobytes()


class MemoOracle:
    """the oracle with its answers kept: the references ask for the same block's sequences once per setting (and the probe's twice), and
    the sequences of a block depend on the profile and the bytes alone"""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def __getattr__(self, name):
        return getattr(self.oracle, name)

    def find(self, prof, data, cap=None, parse_from=0):
        key = (bytes(prof), bytes(data), cap, parse_from)
        if key not in self.kept:
            n, sq = self.oracle.find(prof, data, cap=cap, parse_from=parse_from)
            if n != B.SEQ_ERROR:  # (kept without the unused capacity behind the answer)
                short = (B.Sequence * max(n, 1))()
                C.memmove(short, sq, n * C.sizeof(B.Sequence))
                sq = short
            self.kept[key] = (n, sq)
        return self.kept[key]


_reference = {}
_memo = {}


def reference(zstd, oracle, lib, chunk: int, level: int, checksum: bool, probe: bool, need) -> dict:
    """{(buffer, frame): (the frame the compress call must write for that chunk when it is not skipped, the reference's own counts for
    it)} for the frames in `need` — D.reference_frames_probe / D.reference_frames_grouped over the numpy XOR of chunk and base chunk, the
    level and the checksum setting passed on; every frame computed once per setting"""
    key = (chunk, level, checksum, probe)
    if key not in _reference:
        if len(_reference) >= 4:
            _reference.pop(next(iter(_reference)))
        _reference[key] = {}
    if (chunk, level) not in _memo:
        _memo.clear()
        _memo[(chunk, level)] = MemoOracle(oracle)
    have, orc, bufs = _reference[key], _memo[(chunk, level)], buffers(chunk)
    fn = D.reference_frames_probe if probe else D.reference_frames_grouped
    for i, c in sorted(set(need) - set(have)):
        b = bufs[i]
        piece = b.data[c * chunk:(c + 1) * chunk]
        if b.base is not None:
            piece = xor(piece, b.base[c * chunk:(c + 1) * chunk])
        counts = {}
        (f,) = fn(zstd, orc, piece, chunk, level, b.k, checksum=checksum, lib=lib, counts=counts)
        have[(i, c)] = (f, counts)
    return have


_zero_sums = {}


def zero_checksum(zstd, n: int) -> bytes:
    """the checksum field libzstd itself appends to a frame of n zero bytes"""
    if n not in _zero_sums:
        zc = zstd.cctx(1, checksumFlag=1)
        try:
            _zero_sums[n] = zstd.compress2(zc, bytes(n))[-4:]
        finally:
            zstd.free(zc)
    return _zero_sums[n]


class Mem:
    """an arena of `device` memory filled with 0xA5 and its shadow on the host.  alloc(bytes, align_offset) -> the address of a buffer
    `align_offset` bytes behind a 16-byte line, GUARD bytes behind its neighbour; read / write / poke(addr, bit) act on the device (write
    and poke on the shadow too); expect(addr, data) tells the shadow what a call is about to write; mismatch() compares the WHOLE arena
    with the shadow"""
    stream = None

    def reset(self, capacity: int):
        self.cap = capacity + GUARD + 16
        self.base = self._new(self.cap)
        self.shadow = np.full(self.cap, FILL, dtype=np.uint8)
        self.pos = 0

    def alloc(self, n: int, align_offset: int) -> int:
        addr = ((self.base + self.pos + GUARD + 15) & ~15) + align_offset
        self.pos = addr - self.base + n
        assert self.pos + GUARD <= self.cap, "the arena is too small"
        return addr

    def read(self, addr: int, n: int) -> bytes:
        return self._get(addr - self.base, n).tobytes()

    def write(self, addr: int, data: bytes):
        if len(data):
            a = np.frombuffer(data, dtype=np.uint8)
            self._put(addr - self.base, a)
            self.shadow[addr - self.base:addr - self.base + len(a)] = a

    def poke(self, addr: int, bit: int):
        self._xor(addr - self.base, bit)
        self.shadow[addr - self.base] ^= bit

    def expect(self, addr: int, data: bytes):
        self.shadow[addr - self.base:addr - self.base + len(data)] = np.frombuffer(data, dtype=np.uint8)

    def mismatch(self):
        """None, or where the arena is not what the shadow says"""
        got = self._get(0, self.cap)
        bad = np.flatnonzero(got != self.shadow)
        return None if not len(bad) else "arena byte %d (%d in all): 0x%02x, expected 0x%02x" % (bad[0], len(bad), got[bad[0]], self.shadow[bad[0]])


class HostMem(Mem):
    """host memory registered with the mock device layer as one device range"""

    def __init__(self, plug, slot: int = 0):
        self.plug, self.slot = plug, slot

    def _new(self, cap):
        self.arena = np.full(cap, FILL, dtype=np.uint8)
        self.plug.lib.qzstd_mock_device_range(self.slot, self.arena.ctypes.data, cap, 0)
        return self.arena.ctypes.data

    def _get(self, o, n):
        return self.arena[o:o + n].copy()

    def _put(self, o, a):
        self.arena[o:o + len(a)] = a

    def _xor(self, o, bit):
        self.arena[o] ^= bit


class TorchMem(Mem):
    """a torch byte tensor on the GPU; the library's calls are ordered behind torch's work by the current stream"""

    def __init__(self, device: str = "cuda:0"):
        self.device = device
        self.stream = D.torch.cuda.current_stream(D.torch.device(device)).cuda_stream

    def _new(self, cap):
        self.arena = D.torch.full((cap,), FILL, dtype=D.torch.uint8, device=self.device)
        return self.arena.data_ptr()

    def _get(self, o, n):
        return self.arena[o:o + n].cpu().numpy()

    def _put(self, o, a):
        self.arena[o:o + len(a)] = D.torch.from_numpy(a.copy()).to(self.device)

    def _xor(self, o, bit):
        self.arena[o] ^= bit


def slice_calls(sizes, elems, chunk: int) -> list:
    """two lists of slices (buffer, offset, size), each ascending and disjoint: [chunk - 3, 2 chunk + 4) — three frames, starting and ending
    inside an element — for a buffer of at least 2 chunk + 4 bytes; one byte at `chunk`; the last k + 1 bytes"""
    a, b = [], []
    for i, (n, k) in enumerate(zip(sizes, elems)):
        if n >= 2 * chunk + 4:
            a.append((i, chunk - 3, chunk + 7))
        elif n == chunk + 1:
            a.append((i, chunk, 1))
        elif n:
            a.append((i, max(n - k - 1, 0), min(k + 1, n)))
        if n > 2 * chunk:
            b.append((i, chunk, 1))
        if n > chunk:
            b.append((i, n - k - 1, k + 1))
    return [a, b]


def flip_plan(lens, elems_of_frame, frozen) -> dict:
    """{frame: offset inside its chunk} of the bits to flip: every kind of offset the frames allow at least once — a frame's byte 0, its last
    byte, bytes 16383 and 16384 of a frame longer than a tile, the first tail byte of a frame that does not hold whole elements, a byte of a
    frozen buffer's chunk — one flip per frame, every third of the remaining frames left alone"""
    kinds = collections.OrderedDict()
    for f, (n, k, z) in enumerate(zip(lens, elems_of_frame, frozen)):
        for name, ok, off in (("first", True, 0), ("last", n > 1, n - 1), ("b16383", n > TILE, TILE - 1), ("b16384", n > TILE, TILE),
                              ("tail", n % k != 0, n // k * k), ("frozen", z, n // 2)):
            if ok:
                kinds.setdefault(name, []).append((f, off))
    plan, used = {}, collections.Counter()
    for name in sorted(kinds, key=lambda m: len(kinds[m])):  # the rarest kind picks first
        for f, off in kinds[name]:
            if f not in plan:
                plan[f] = off
                used[name] += 1
                break
    assert set(used) == set(kinds), (used, list(kinds))
    for f in range(len(lens)):
        if f not in plan and f % 3 != 2:
            name = min((m for m in kinds if any(g == f for g, _ in kinds[m])), key=lambda m: used[m])
            plan[f] = next(off for g, off in kinds[name] if g == f)
            used[name] += 1
    return plan


def cycle(front_lib, zstd, oracle, mem, chunk: int, level: int, checksum: bool, probe: bool, skip: bool, threads: int = 3):
    bufs = buffers(chunk)
    nb = len(bufs)
    elems = [b.k for b in bufs]
    sizes = [len(b.data) for b in bufs]
    based = [b.base is not None for b in bufs]
    datas = [b.data for b in bufs]
    assert sum(sizes) < 8 << 20
    data_chunks = [chunks(b.data, chunk) for b in bufs]
    base_chunks = [chunks(b.base, chunk) if b.base is not None else None for b in bufs]
    equal = [[bc is not None and d == bc[c] for c, d in enumerate(dc)] for dc, bc in zip(data_chunks, base_chunks)]
    first = [0]
    for dc in data_chunks:
        first.append(first[-1] + len(dc))
    n_frames = first[-1]
    lens = [len(d) for dc in data_chunks for d in dc]
    n_equal = sum(sum(e) for e in equal)
    frame_elem = [k for k, dc in zip(elems, data_chunks) for _ in dc]
    # the block rule restated (include/qzstd_bytegroup.h): a block per plane from QZSTD_BYTEGROUP_CUT_MIN elements on, the plane cuts rounded
    # down to 16, every piece cut every 128 KiB — the references take their blocks from the library under test
    for n, k in sorted(set(zip(lens, frame_elem))):
        assert D.group_blocks(n, k, front_lib) == D.blocks_with_cuts(n, k, k > 1 and n // k >= 4096), (n, k)

    # ---- the cycle cannot pass vacuously: asserted on the reference's own counts and on the bytes, before the library is asked
    built = [(i, c) for i, es in enumerate(equal) for c, e in enumerate(es) if not (skip and e)]  # the frames that are not zero frames
    ref = reference(zstd, oracle, front_lib, chunk, level, checksum, probe, built)
    if probe and chunk >= 16400:
        assembled = sum(ref[ic][1]["assembled"] for ic in built)
        assert 0 < assembled < len(built), "the probe's reference assembles %d of %d frames" % (assembled, len(built))
    if probe and chunk == 4080:  # planes below QZSTD_BYTEGROUP_CUT_MIN: nothing is raw-predicted, probe on IS probe off
        off = reference(zstd, oracle, front_lib, chunk, level, checksum, False, built)
        assert all(ref[ic][1]["raw"] == 0 and ref[ic][0] == off[ic][0] for ic in built)
    if skip:
        full = [e for i, es in enumerate(equal) for c, e in enumerate(es) if based[i] and len(data_chunks[i][c]) == chunk]
        tail = [e for i, es in enumerate(equal) for c, e in enumerate(es) if based[i] and len(data_chunks[i][c]) < chunk and c > 0]
        assert any(full) and any(tail) and not all(e for i, es in enumerate(equal) if based[i] for e in es)
        if chunk > 131072:
            assert len(D.frame_blocks(D.zero_frame(chunk))) > 1  # an equal full chunk: a zero frame of several RLE blocks

    slices = slice_calls(sizes, elems, chunk)
    assert any(n == chunk + 7 for _, _, n in slices[0]) and any(n == 1 for _, _, n in slices[1])
    mem.reset(5 * sum(sizes) + 4 * sum(n for sl in slices for _, _, n in sl) + (5 * nb + 4 * sum(len(sl) for sl in slices)) * (GUARD + 48))
    soff = [(1, 3, 15, 5, 9)[i % 5] for i in range(nb)]

    def place(sz, shift, fill=None):
        out = []
        for i, n in enumerate(sz):
            p = mem.alloc(n, (soff[i % nb] + shift) % 16)
            if fill is not None and fill[i] is not None:
                mem.write(p, fill[i])
            out.append((p, n))
        return out

    src = place(sizes, 0, datas)
    bas = place(sizes, 6, [b.base if b.base is not None else bytes(len(b.data)) for b in bufs])
    given = [b if on else None for b, on in zip(bas, based)]
    assert all((s[0] - b[0]) % 16 for s, b in zip(src, bas))
    st = mem.stream
    fr = D.DeviceFront(threads, level, chunk, lib=front_lib)
    try:
        assert fr.set_checksum(checksum) == 0 and fr.set_plane_probe(probe) == 0 and fr.set_delta_skip(skip) == 0
        # ---- 1. fingerprints of the live buffers
        kept = fr.fingerprint(src, st)
        assert kept == [[D.fingerprint_ref(d) for d in dc] for dc in data_chunks]
        # ---- 2. compress: every frame is the reference's, frame by frame
        frames = fr.compress_device_batch_delta(src, given, elems, st)
        assert [len(per) for per in frames] == [len(dc) for dc in data_chunks]
        compared = 0
        for i, per in enumerate(frames):
            for c, f in enumerate(per):
                n = len(data_chunks[i][c])
                if skip and equal[i][c]:
                    want = D.zero_frame(n, checksum) + (zero_checksum(zstd, n) if checksum else b"")
                else:
                    want = ref[(i, c)][0]
                assert f == want, "buffer %d (%d bytes, elem %d, base %s) frame %d: not the reference's frame" % (
                    i, sizes[i], elems[i], bufs[i].kind, c)
                compared += 1
                # an independent reader: libzstd (which verifies a checksum), numpy, the base chunk
                content = ungroup(zstd.decompress(f, chunk), elems[i])
                assert (xor(content, base_chunks[i][c]) if based[i] else content) == data_chunks[i][c], (i, c)
        assert compared == n_frames == sum(len(per) for per in frames)
        if skip:
            assert fr.delta_skip_stats()[:2] == [sum(len(dc) for dc, on in zip(data_chunks, based) if on), n_equal]
        if probe and chunk >= 16400:
            assert fr.plane_probe_stats()[2] > 0
        assert mem.mismatch() is None  # the inputs were only read
        # ---- 3. restore into fresh guarded buffers, 4. and in place over copies of the bases
        out = place(sizes, 10)
        for (p, _), d in zip(out, datas):
            mem.expect(p, d)
        assert fr.restore_batch_delta(frames, out, given, elems, st) == n_frames
        assert mem.mismatch() is None
        inp = place(sizes, 4, [b.base for b in bufs])
        for (p, _), d in zip(inp, datas):
            mem.expect(p, d)
        assert fr.restore_batch_delta(frames, inp, [b if on else None for b, on in zip(inp, based)], elems, st) == n_frames
        assert mem.mismatch() is None
        # ---- 5. slices: onto the bases' matching slices, and in place over copies of them
        for sl in slices:
            need = {(i, c) for i, o, n in sl for c in range(o // chunk, (o + n - 1) // chunk + 1)}
            for in_place in (False, True):
                dst = place([n for _, _, n in sl], 10, [bufs[i].base[o:o + n] if in_place and based[i] else None for i, o, n in sl])
                give = [(i, o, n, p, None if not based[i] else (p if in_place else bas[i][0] + o)) for (i, o, n), (p, _) in zip(sl, dst)]
                for (i, o, n), (p, _) in zip(sl, dst):
                    mem.expect(p, datas[i][o:o + n])
                assert fr.restore_slices(frames, sizes, elems, give, st) == len(need)
                assert mem.mismatch() is None, (sl, in_place)
        # ---- 6. verify, untouched and after bit flips
        r, diff = fr.verify_raw(frames, src, given, elems, st)
        assert (r, diff) == (0, [D.VERIFY_SAME] * n_frames)
        frozen = [bufs[i].kind == "identical" for i, dc in enumerate(data_chunks) for _ in dc]
        plan = flip_plan(lens, frame_elem, frozen)
        where = {first[i] + c: (i, c) for i, dc in enumerate(data_chunks) for c in range(len(dc))}
        for f, o in plan.items():
            i, c = where[f]
            mem.poke(src[i][0] + c * chunk + o, 1 << (f % 8))
        want = []  # firstDiff as the header defines it, on the host: decode, ungroup, XOR the base chunk, compare with the live chunk
        for i, per in enumerate(frames):
            live = mem.read(*src[i])
            for c, f in enumerate(per):
                u = ungroup(zstd.decompress(f, chunk), elems[i])
                u = np.frombuffer(xor(u, base_chunks[i][c]) if based[i] else u, dtype=np.uint8)
                bad = np.flatnonzero(u != np.frombuffer(live[c * chunk:(c + 1) * chunk], dtype=np.uint8))
                want.append(int(bad[0]) if len(bad) else D.VERIFY_SAME)
        assert want == [plan.get(f, D.VERIFY_SAME) for f in range(n_frames)] and 0 < len(plan) < n_frames
        r, diff = fr.verify_raw(frames, src, given, elems, st)
        assert r == len(plan) and diff == want
        # ---- 7. fingerprints: the flipped buffers, the restored ones, a restore against swapped bases
        touched = [where[f] for f in sorted(plan)]
        assert fr.check(src, kept, st) == touched
        for f, o in plan.items():
            i, c = where[f]
            mem.poke(src[i][0] + c * chunk + o, 1 << (f % 8))
        assert fr.check(src, kept, st) == [] and fr.check(out, kept, st) == [] and fr.check(inp, kept, st) == []
        swapped = place(sizes, 12)
        for (p, _), b in zip(swapped, bufs):  # (d ^ base) ^ d: the base's bytes come back
            mem.expect(p, b.data if b.base is None else b.base)
        assert fr.restore_batch_delta(frames, swapped, [s if on else None for s, on in zip(src, based)], elems, st) == n_frames
        assert mem.mismatch() is None
        changed = [(i, c) for i, es in enumerate(equal) if based[i] for c, e in enumerate(es) if not e]
        assert changed and fr.check(swapped, kept, st) == changed
        assert fr.verify_raw(frames, src, given, elems, st)[0] == 0
        assert mem.mismatch() is None  # compress, verify and the fingerprint calls left every input byte as it was
    finally:
        fr.close()
    return n_frames
