"""GPU: the windowed ungrouping scatter (qzstd_hip_ungroup_window, include/qzstd_hip_device.h) alone, through the C ABI, against numpy: every
row of one launch must write u[winOff : winOff + winLen] ^ base of its staged frame (u[]: the frame's ungrouped content) to its destination —
windows at every phase of an element, across tile boundaries, inside and into the tail, whole frames, empty ones; destination and base at
alignments chosen independently; rows with a base of their own, without one and in place; several windows of ONE frame in a launch, also with
destinations packed back to back so that 16-byte words have two owners.  Exactly the rows' bytes may change (0xA5 everywhere else), the
stage's padding (0xEE) must never show, a disjoint base never changes.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 64
ELEMS = (1, 2, 4, 8)
ALIGNS = (0, 1, 7, 8, 15)
FILL, PAD = 0xA5, 0xEE
TILE = 16384


def lens(k):
    return [k - 1, k + 1, 17, 16 * k + 1, 4097, TILE - 1, TILE, TILE + k + 1, 131072 + k + 1, (1 << 20) + 3]


def payload(rng, n):
    """random bytes without the two marker values: a 0xEE or a 0xA5 in the wrong place is then visible as such"""
    a = rng.integers(0, 254, n, dtype=np.uint8)
    a[a >= FILL] += 1
    a[a >= PAD] += 1
    return a


def numpy_group(a, k):
    n = len(a) // k
    return np.concatenate([a[:n * k].reshape(n, k).T.reshape(-1), a[n * k:]])


def windows(n, k):
    """-> (fixed [(winOff, winLen)], flexible [(start phase, winLen)]) of a frame of n bytes, element size k; only what fits the frame"""
    fixed = [(0, n), (0, 1), (n - 1, 1), (1, n - 2), (TILE - 5, 10), (TILE - 5, TILE + 10), (min(5, n), 0)]
    body = n // k * k
    if n > body:
        fixed += [(body, n - body), (body + (n - body) // 2, 1)]          # inside the tail
        fixed += [(max(body - 3 * k + 1, 0), min(3 * k - 1, body) + 1)]   # elements, ending inside the tail
        fixed += [(max(body - TILE - 3, 0), min(TILE + 3, body) + n - body)]  # ... from the tile before, through the whole tail
    fixed = sorted({(o, w) for o, w in fixed if o >= 0 and w >= 0 and o + w <= n})
    flex = [(p, w) for p in range(1, k) for w in (1, k, 16, 17, 33) if p + w <= n]
    return fixed, flex


def rounds_of(n, k):
    """the frame's windows dealt into rounds: in a round they are disjoint and ascending, as one launch wants the windows of one frame.  A
    flexible window starts at the first byte of its phase behind the round's last window (so the phases land anywhere in the frame, in
    any tile), or opens a round of its own"""
    fixed, flex = windows(n, k)
    rounds = []
    for o, w in fixed:
        for r in rounds:
            if r[-1][0] + r[-1][1] <= o:
                r.append((o, w))
                break
        else:
            rounds.append([(o, w)])
    for p, w in flex:
        for r in rounds:
            end = r[-1][0] + r[-1][1]
            o = end + (p - end) % k
            if o + w <= n:
                r.append((o, w))
                break
        else:
            rounds.append([(p, w)])
    return rounds


def align_pairs(n):
    """(destination alignment, base alignment): all 25 pairs of ALIGNS, for the longest frames five that differ and one that agrees"""
    if n < (1 << 20):
        return [(a, b) for a in ALIGNS for b in ALIGNS]
    return [(ALIGNS[i], ALIGNS[(i + 2) % 5]) for i in range(5)] + [(7, 7)]


def kinds(i):
    return "none" if i % 3 == 1 else ("self" if i % 4 == 2 else "base")


class Stage:
    """frames (u[]: marker-free content, element size, length) grouped at 16-aligned offsets of one device buffer, 0xEE between len and
    pad16(len), in the gaps and behind the end"""

    def __init__(self, frames, seed):
        rng = np.random.default_rng(seed)
        self.frames, parts, so = [], [], 0  # (srcOff, len, elem, u)
        for i, (n, k) in enumerate(frames):
            gap = 32 if i % 5 == 0 else 0
            parts.append(np.full(gap, PAD, dtype=np.uint8))
            so += gap
            u = payload(rng, n)
            self.frames.append((so, n, k, u))
            parts.append(numpy_group(u, k))
            pad = (-n) % 16 if n else 16  # (an empty frame keeps an offset of its own: equal offsets mean ONE frame)
            parts.append(np.full(pad, PAD, dtype=np.uint8))
            so += n + pad
        self.host = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        self.size = len(self.host)
        self.t = torch.full((self.size + 48,), PAD, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.t.data_ptr() + (-self.t.data_ptr()) % 16
        o = self.ptr - self.t.data_ptr()
        self.t[o:o + self.size] = torch.from_numpy(self.host).to("cuda:0")


def launch(plug, L, stage, specs, seed, packed=False, order=None, stage_skew=0, stage_bytes=None, null=None, null_dst=False, tweak=None):
    """specs: [(frame index, winOff, winLen, destination alignment, base alignment, kind)] in STAGE order; order: the rows' places in the
    destination (a permutation; default: stage order); packed: every destination right behind the one before it.  Builds the bases so that
    every destination ends up marker-free (rows without one: the stage's own content), runs ONE launch and compares: the destination with its
    guards, the bases.  -> the return value"""
    rng = np.random.default_rng(seed)
    order = list(range(len(specs))) if order is None else order
    place, pos, bpos = {}, 5 if packed else 0, GUARD
    for i in order:
        f, wo, wl, a, b, kind = specs[i]
        if not packed:
            pos = ((pos + 15) & ~15) + a + (32 if i % 7 == 0 else 0)
        bpos = ((bpos + 15) & ~15) + b
        place[i] = (pos, bpos)
        pos += wl
        bpos += wl if kind == "base" else 0
    size = pos + 16
    bas = rng.integers(0, 256, bpos + GUARD, dtype=np.uint8)
    init = np.full(GUARD + size + GUARD, FILL, dtype=np.uint8)
    want = np.full(GUARD + size + GUARD, FILL, dtype=np.uint8)
    for i, (f, wo, wl, a, b, kind) in enumerate(specs):
        p, bp = place[i]
        u = stage.frames[f][3][wo:wo + wl]
        if kind == "none":
            want[GUARD + p:GUARD + p + wl] = u
            continue
        final = payload(rng, wl)
        want[GUARD + p:GUARD + p + wl] = final
        if kind == "self":
            init[GUARD + p:GUARD + p + wl] = u ^ final  # what the destination held before: the previous checkpoint's bytes
        else:
            bas[bp:bp + wl] = u ^ final
    dst = torch.from_numpy(init).to("cuda:0")
    base_t = torch.from_numpy(bas).to("cuda:0")
    assert dst.data_ptr() % 16 == 0 and base_t.data_ptr() % 16 == 0
    rows = (D.UngroupWinRow * max(len(specs), 1))()
    for i, (r, (f, wo, wl, a, b, kind)) in enumerate(zip(rows, specs)):
        so, n, k, _ = stage.frames[f]
        r.dst = 0 if null_dst else dst.data_ptr() + GUARD + place[i][0]
        r.base = 0 if kind == "none" else (r.dst if kind == "self" else base_t.data_ptr() + place[i][1])
        r.srcOff, r.len, r.elem, r.winOff, r.winLen, r.tile0, r.reserved = so, n, k, wo, wl, 0xDEAD, 0
    if tweak:
        tweak(rows)
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_ungroup_window(0, None, None if null == "rows" else rows, len(specs), None if null == "d_rows" else d_rows,
                                        None if null == "stage" else stage.ptr + stage_skew, stage.size if stage_bytes is None else stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    got = dst.cpu().numpy()
    if rc != 0 or not specs or all(s[2] == 0 for s in specs):
        assert np.array_equal(got, init), "a launch that queues nothing changed the destination"
        return rc
    bad = np.flatnonzero(got != want)
    if len(bad):
        at = int(bad[0]) - GUARD
        row = max((i for i in place if place[i][0] <= at), key=lambda i: place[i][0], default=None)
        raise AssertionError("destination differs from numpy at byte %d, %d bytes in all (got 0x%02x, want 0x%02x); row %s at %s, frame (srcOff, len, elem) = %s"
                             % (at, len(bad), got[bad[0]], want[bad[0]], specs[row] if row is not None else None, place.get(row),
                                stage.frames[specs[row][0]][:3] if row is not None else None))
    assert not (got == PAD).any()  # no byte of the stage's padding anywhere
    assert np.array_equal(base_t.cpu().numpy(), bas)  # a disjoint base is only read
    # tile0 is the running sum of the rows' workgroups
    t0 = 0
    for r, (f, wo, wl, *_rest) in zip(rows, specs):
        assert r.tile0 == t0
        so, n, k, _ = stage.frames[f]
        tiles = max(-(-(n // k) // (TILE // k)), 1)
        t0 += 0 if not wl else min((wo + wl - 1) // TILE, tiles - 1) - min(wo // TILE, tiles - 1) + 1
    return rc


@pytest.fixture(scope="module")
def api(gpu_plugin):
    return D.bind_window_kernel(D.bind_xor_kernels(gpu_plugin.lib))


@pytest.fixture(scope="module")
def big_stage(api):
    """every frame length for every element size, an instance per alignment pair, long and short interleaved"""
    inst = [(n, k, a, b) for k in ELEMS for n in lens(k) for a, b in align_pairs(n)]
    rng = np.random.default_rng(16)
    inst = [inst[i] for i in rng.permutation(len(inst))]
    return Stage([(n, k) for n, k, _, _ in inst], seed=1), inst


def test_window_kernel_every_frame_length_window_element_size_and_both_alignments(gpu_plugin, api, big_stage):
    stage, inst = big_stage
    per = [rounds_of(n, k) for n, k, _, _ in inst]
    # what the windows must cover, for every element size: the whole frame, mid-element starts of every phase, tile crossings, the tail
    for k in ELEMS:
        n = 131072 + k + 1
        flat = [w for r in rounds_of(n, k) for w in r]
        assert (0, n) in flat and (TILE - 5, TILE + 10) in flat and (n - 1, 1) in flat and (min(5, n), 0) in flat
        assert {o % k for o, w in flat if w in (1, k, 16, 17, 33)} >= set(range(1, k))
        assert k == 1 or (any(o >= n // k * k and w for o, w in flat) and any(0 < o < n // k * k < o + w for o, w in flat))
    row = 0
    for rnd in range(max(len(p) for p in per)):
        specs = []
        for f, ((n, k, a, b), rs) in enumerate(zip(inst, per)):
            for wo, wl in rs[rnd] if rnd < len(rs) else ():
                specs.append((f, wo, wl, a, b, kinds(row)))
                row += 1
        assert launch(gpu_plugin, api, stage, specs, seed=100 + rnd) == 0, gpu_plugin.err()
    assert row > 10000


@pytest.mark.parametrize("reverse", (False, True))
def test_adjacent_windows_of_one_frame_packed_back_to_back_share_their_words(gpu_plugin, api, reverse):
    """the windows of a frame tile it without a gap, their destinations follow each other at boundaries that are no multiple of 16: every
    shared word has two owners, in two workgroups.  In stage order, and with the destinations in reverse order"""
    frames = [(n, k) for k in ELEMS for n in (100003, TILE + k + 1, 4097, 33)]
    stage = Stage(frames, seed=2)
    rng = np.random.default_rng(3)
    specs = []
    for f, (n, k) in enumerate(frames):
        cuts = sorted({0, n} | set(int(c) for c in rng.integers(1, n, 9)) | {min(n, TILE - 3), min(n, TILE + 5)})
        for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            specs.append((f, lo, hi - lo, 0, ALIGNS[(f + i) % 5], kinds(len(specs))))
    order = list(range(len(specs)))
    assert sum(1 for s in specs if s[2] % 16) > len(specs) // 2
    assert launch(gpu_plugin, api, stage, specs, seed=4, packed=True, order=order[::-1] if reverse else order) == 0, gpu_plugin.err()


def test_whole_frame_windows_are_the_ungroup_xor_kernel(gpu_plugin, api):
    """rows whose window is the whole frame: byte for byte what qzstd_hip_ungroup_xor leaves on the same stage, bases and destinations"""
    L = api
    frames = [(n, k) for k in ELEMS for n in (0, 1, 15, 16, 17, 4097, TILE, TILE + k + 1, 70001, 131072 + k + 1)]
    stage = Stage(frames, seed=5)
    rng = np.random.default_rng(6)
    total = sum(((n + 15) & ~15) + 32 for n, _ in frames)
    bas = torch.from_numpy(rng.integers(0, 256, total + GUARD, dtype=np.uint8)).to("cuda:0")
    outs = []
    for which in ("window", "xor"):
        dst = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        rows = ((D.UngroupWinRow if which == "window" else D.UngroupXorRow) * len(frames))()
        pos = 0
        for i, (r, (so, n, k, _)) in enumerate(zip(rows, stage.frames)):
            pos = ((pos + 15) & ~15) + ALIGNS[i % 5]
            r.dst, r.srcOff, r.len, r.elem = dst.data_ptr() + GUARD + pos, so, n, k
            r.base = 0 if i % 3 == 1 else bas.data_ptr() + pos + ALIGNS[(i + 2) % 5]
            if which == "window":
                r.winOff, r.winLen = 0, n
            pos += n
        d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
        assert d_rows, gpu_plugin.err()
        try:
            torch.cuda.synchronize()
            fn = L.qzstd_hip_ungroup_window if which == "window" else L.qzstd_hip_ungroup_xor
            assert fn(0, None, rows, len(frames), d_rows, stage.ptr, stage.size) == 0, gpu_plugin.err()
            gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
        finally:
            L.qzstd_hip_free(0, d_rows)
        outs.append(dst.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    assert (outs[0] != FILL).sum() > sum(n for n, _ in frames) * 0.9  # (something was written)


def test_window_launcher_refusals_leave_the_destination_untouched(gpu_plugin, api):
    frames = [(100, 2), (48, 8), (4000, 4)]
    stage = Stage(frames, seed=7)
    assert [f[0] for f in stage.frames] == [32, 144, 192] and stage.size == 4192
    good = [(0, 3, 50, 3, 7, "base"), (0, 60, 40, 0, 1, "none"), (1, 0, 0, 0, 0, "none"), (2, 1001, 2999, 15, 8, "self")]

    def setter(i, **kw):
        def tweak(rows):
            for name, v in kw.items():
                setattr(rows[i], name, v)
        return tweak

    cases = {
        "misaligned srcOff": setter(0, srcOff=40),
        "elem 0": setter(0, elem=0), "elem 3": setter(3, elem=3), "elem 16": setter(1, elem=16),
        "reserved": setter(1, reserved=1),
        "window past its frame": setter(1, winLen=41),
        "winOff past its frame": setter(2, winOff=49),
        "winOff + winLen wraps": setter(3, winOff=0xFFFFFFFF, winLen=2),
        "frame ends past stageBytes": setter(3, len=4001 + 16, winOff=0),
        "len above 0xFFFFFFE0": setter(3, len=0xFFFFFFE1),
        "same frame, another len": setter(1, len=99, winLen=10),
        "same frame, another elem": setter(1, elem=4),
        "windows of a frame overlap": setter(1, winOff=52),
        "windows of a frame out of order": setter(1, winOff=0, winLen=2),
        "frames overlap": setter(3, srcOff=stage.frames[0][0] + 96, len=16, winOff=0, winLen=16),
        "frames out of order": setter(3, srcOff=0, len=16, winOff=0, winLen=16),
    }
    for name, tweak in cases.items():
        assert launch(gpu_plugin, api, stage, good, seed=8, tweak=tweak) < 0, name
    for null in ("rows", "d_rows", "stage"):
        assert launch(gpu_plugin, api, stage, good, seed=8, null=null) < 0, null
    assert launch(gpu_plugin, api, stage, good, seed=8, null_dst=True) < 0
    assert launch(gpu_plugin, api, stage, good, seed=8, stage_skew=8) < 0
    assert launch(gpu_plugin, api, stage, good, seed=8, stage_bytes=stage.frames[2][0] + 3999) < 0
    assert launch(gpu_plugin, api, stage, good, seed=8, stage_bytes=1 << 37, tweak=setter(3, srcOff=1 << 36, len=16, winOff=0, winLen=16)) < 0
    # (more than 2^31 - 1 workgroups cannot be reached below the other limits: a frame has at most 2^18 tiles and a stage fewer than 2^4 such frames)
    # the two launches that queue nothing and return 0
    assert launch(gpu_plugin, api, stage, [], seed=8) == 0
    assert launch(gpu_plugin, api, stage, [(0, 3, 0, 3, 7, "base"), (0, 60, 0, 0, 1, "none"), (1, 0, 0, 0, 0, "self")], seed=8) == 0
    # no value of base is refused: one that equals the destination, one at an odd address
    assert launch(gpu_plugin, api, stage, good, seed=9) == 0, gpu_plugin.err()
