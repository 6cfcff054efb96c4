"""Device-resident input against today's way, one JSON line.

On N GiB of qz_corpus.system_corpus in a GPU tensor, at levels 1 / 6 / 12 with 128 KiB frames and 16 worker threads:
  host   t.cpu() + QZSTD_frontCompress (the tensor copied to host memory, then the producer path)
  device QZSTD_frontCompressDevice (match-finder + compaction on the tensor's GPU, one dense D2H copy per part)
GB/s of input (best of --reps; the window holds the library calls and, for the host way, t.cpu() — nothing else: the destination is
sized once, one untimed pass of each way comes first, frames are read out of the destination after the window), D2H bytes per input
byte, frames that took the raw-bytes fallback, compressed sizes, whether both ways give the same frames.

  python tools/device_bench.py --gib 1 --reps 3 [--levels 1,6,12]

--batch: a LIST of tensors, N GiB in total from the same corpus, in three mixes — (a) tensors of 128 KiB, (b) sizes log-uniform between
4 KiB and 64 MiB from a fixed seed, each tensor its own allocation, (c) one tensor — and three ways, library calls timed, every run listed:
  batch  one QZSTD_frontCompressDeviceBatch call (skipped, "n/a", on a library without it: the other two ways measure an older build)
  loop   one QZSTD_frontCompressDevice call per tensor
  cat    torch.cat + one QZSTD_frontCompressDevice call, the cat inside the window (mixes a and b)

  python tools/device_bench.py --batch --gib 1 --reps 3 [--levels 1,6,12] [--ways batch,loop,cat] [--mixes a_128k,b_loguniform,c_one]

--checksum: content checksums (QZSTD_frontSetChecksum).  The legs above on one tensor — host (t.cpu() + QZSTD_frontCompress: the baseline,
libzstd hashes), device (QZSTD_frontCompressDevice: the GPU hashes) — and batch (one QZSTD_frontCompressDeviceBatch call over the tensor's
128 KiB pieces, each an allocation of its own), every leg with the setting off and on in the same run on the same front, every run listed;
plus who hashed the frames and whether the device frames equal the host path's with the setting on.

  python tools/device_bench.py --checksum --gib 1 --reps 3 [--levels 1,6,12] [--legs host,device,batch] [--no-compare]

--group: byte grouping (QZSTD_frontSetByteGroup) on typed data — an N GiB bf16 tensor and an N GiB fp32 one of N(0, 0.02) weights (drawn on the
GPU from a fixed seed).  Four legs, every run listed, grouping off and on alternating in one run:
  off    QZSTD_frontCompressDevice, the setting 1
  on     QZSTD_frontCompressDevice, the setting the element size (grouped on the GPU while staging, a block per plane)
  torch  what a caller can do without the feature: a torch byte transposition of every frame on the GPU, then QZSTD_frontCompressDevice
         with the setting 1 (grouped content, blocks every 128 KiB); the transposition is inside the window
  host   t.cpu() + numpy grouping of every frame + QZSTD_frontCompress
plus compressed sizes, the share of grouped frames by how they were built (QZSTD_frontByteGroupStats) and bytes device->host per input byte.
--kernels: one untimed `on` pass per element size 2, 4, 8 (the same bytes seen as bf16, fp32, int64) and one `off` pass of an unaligned
view (gathered) at level 1 and nothing else: the run to put under rocprofv3.

  python tools/device_bench.py --group --gib 1 --reps 3 [--levels 1,6,12] [--legs off,on,torch,host] [--kernels]

--restore: the way back (QZSTD_frontRestoreDeviceBatchTyped) on the same typed data — N GiB of bf16 and of fp32 N(0, 0.02) weights, level-1
frames of 128 KiB, grouped (the element size) and ungrouped (1) — into one N GiB tensor and into tensors of 128 KiB, each an allocation of
its own.  Two legs, alternating in one run, every run listed, GB/s of restored content:
  lib       one QZSTD_frontRestoreDeviceBatchTyped call (the front's workers decode, one H2D copy and one ungroup launch per part)
  baseline  what a caller does today, written here: ZSTD_decompressDCtx on --threads Python threads (ctypes: the GIL is released inside
            the calls) into pinned memory, QZSTD_byteUngroup on the same threads for grouped frames, then one copy_ per tensor
The window holds the calls, the copies and the closing synchronize; the frames, the destinations and the pinned buffer exist before it.
--kernels: one untimed restore per element size 1, 2, 4, 8 (the same bytes) into one tensor and nothing else: the run to put under rocprofv3.

  python tools/device_bench.py --restore --gib 1 --reps 3 [--kernels]

--delta: delta frames against a base (QZSTD_frontCompressDeviceBatchDelta / QZSTD_frontRestoreDeviceBatchDelta) — N GiB of bf16 and of fp32
N(0, 0.02) weights (the base) and the same after an update drawn from N(0, 1e-5) (the new checkpoint), both on the GPU.  Two legs each way,
alternating in one run, every run listed, GB/s of input / of restored content:
  delta  one QZSTD_frontCompressDeviceBatchDelta call; back: one QZSTD_frontRestoreDeviceBatchDelta call in place over the base
  torch  what a caller does today: torch.bitwise_xor into a temporary (allocated inside the window, as a caller must) +
         QZSTD_frontCompressDeviceBatchTyped; back: QZSTD_frontRestoreDeviceBatchTyped into a temporary + bitwise_xor_ into the base
plus compressed / input for delta + grouped and for grouped alone, and bytes device->host per input byte.
--kernels: through the C ABI, nothing timed: qzstd_hip_group_xor and qzstd_hip_group, then qzstd_hip_ungroup_xor and qzstd_hip_ungroup, over
the same N GiB of 128 KiB rows for each element size 1, 2, 4, 8: the run to put under rocprofv3.

  python tools/device_bench.py --delta --gib 1 --reps 3 [--levels 1,6,12] [--kernels]

--slices: a resharded load (QZSTD_frontRestoreDeviceSlices) — N GiB of bf16 and of fp32 N(0, 0.02) weights as 2-D tensors with rows of 16 KiB,
level-1 grouped frames of 128 KiB, written with and without a base.  Two legs, alternating in one run, every run listed, seconds per load,
frames decoded, bytes host->device and torch's peak extra device memory:
  A  one QZSTD_frontRestoreDeviceSlices call: a 1/8 row shard (one slice) and a 1/8 column shard (2 KiB of every row: a slice per row)
  B  what a caller does today: QZSTD_frontRestoreDeviceBatchDelta of the whole tensor into a temporary, then narrow().copy_()
--kernels: through the C ABI, nothing timed: qzstd_hip_ungroup_xor, then qzstd_hip_ungroup_window over the same N GiB stage as whole-frame
windows and as the column shard's 2 KiB windows, for each element size 1, 2, 4, 8: the run to put under rocprofv3.

  python tools/device_bench.py --slices --gib 1 --reps 3 [--kernels]

--skip: delta skip (QZSTD_frontSetDeltaSkip) — N GiB of bf16 N(0, 0.02) weights as 64 tensors against their bases; a share p of 0, 0.5, 0.9
and 1 of the tensors is identical to its base and the rest has taken the delta leg's N(0, 1e-5) update.  Levels 1 and 6, the setting off and
on alternating in one run, every run listed: the delta compress call, the delta restore in place over a copy of the bases and into fresh
tensors (off: the setting-off call's frames, the setting off; on: the setting-on call's frames, the setting on); GB/s of input, compressed
bytes, bytes device->host and host->device per input byte.
--kernels: through the C ABI, nothing timed: qzstd_hip_diff over N GiB of 128 KiB rows (equal, different, and b at another alignment than
a), then qzstd_hip_group_xor over the same rows: the run to put under rocprofv3.

  python tools/device_bench.py --skip --gib 1 --reps 3 [--levels 1,6] [--kernels]

--verify: the check before the previous checkpoint is dropped (QZSTD_frontVerifyDeviceBatch) — N GiB of bf16 and of fp32 N(0, 0.02) weights
after an N(0, 1e-5) update against a base, written as level-1 grouped delta frames of 128 KiB; one tensor of N GiB and N x 8192 tensors of
128 KiB; delta skip off, and on with every other chunk unchanged (p = 0.5).  Two legs, alternating in one run, every run listed, ms per
check, bytes host->device and torch's peak extra device memory:
  verify         one QZSTD_frontVerifyDeviceBatch call against the live tensors
  restore_equal  what a caller does today: QZSTD_frontRestoreDeviceBatchDelta into fresh tensors + torch.equal per tensor
--kernels: through the C ABI, nothing timed: qzstd_hip_ungroup_xor, then qzstd_hip_ungroup_cmp, ONE launch each over the same N GiB stage of
128 KiB frames with a base, for each element size 1, 2, 4, 8: the run to put under rocprofv3.

  python tools/device_bench.py --verify --gib 1 --reps 3 [--kernels]

--probe: the plane probe (QZSTD_frontSetPlaneProbe) on --group's typed data — an N GiB bf16 tensor and an N GiB fp32 one of N(0, 0.02) weights,
byte grouping on (the element size), levels 1 / 6 / 12.  Two legs, the setting off and on alternating in one run, every run listed: GB/s of
input of QZSTD_frontCompressDevice, compressed sizes, bytes device->host per input byte, and of the setting-on frames the share the library
assembled and the share that fell back (QZSTD_frontPlaneProbeStats [2] and [3]), blocks probed and written raw.
--kernels: through the C ABI, timed with events around ONE launch each, every run listed as ms per GiB: qzstd_hip_group (element size 2) over
N GiB of 128 KiB rows, and qzstd_hip_plane_cost over N GiB of 128 KiB rows of a noise plane (random bytes), of an exponent plane (the high
bytes of bf16 N(0, 0.02) weights: a handful of values) and over the grouped stage's own 64 KiB planes as the front-end launches it.

  python tools/device_bench.py --probe --gib 1 --reps 3 [--levels 1,6,12] [--kernels]

--code: the plane code (QZSTD_frontSetPlaneCode) on --probe's data and settings, the legs probe on / code on alternating in one run: GB/s,
compressed bytes, D2H per input byte, the share of frames assembled without libzstd; --kernels: qzstd_hip_huf_code beside
qzstd_hip_plane_cost, ms per GiB, in the same run.

  python tools/device_bench.py --code --gib 1 --reps 3 [--levels 1,6,12] [--kernels]

--fingerprint: the load-time check (QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch) — N GiB of bf16 N(0, 0.02) weights as one
tensor and as N x 8192 tensors of 128 KiB.  Three legs, alternating in one run, every run listed, ms per call (the call and the closing
synchronize):
  fingerprint  one QZSTD_frontFingerprintDeviceBatch call
  host_hash    what a caller can do today: t.cpu() per tensor and XXH64 (python-xxhash) of every 128 KiB chunk on --threads threads
  verify       QZSTD_frontVerifyDeviceBatch of the same tensors' level-1 grouped frames: the only other end-to-end check, which needs the live tensors
then, in the same run, the kernels through the C ABI with events around ONE launch each over N GiB of 128 KiB rows, the three alternating:
qzstd_hip_fingerprint, qzstd_hip_diff (two sides) and qzstd_hip_xxh64, ms per GiB.  --kernels: those kernel legs alone (also the run to put
under rocprofv3).

  python tools/device_bench.py --fingerprint --gib 1 --reps 3 [--kernels]

--srcslices: a tensor that is not contiguous, written (QZSTD_frontCompressDeviceSlices) — the left half of an [N x 65536, 16384]-byte matrix of
bf16 N(0, 0.02) weights: N x 65536 slices of 8 KiB, frames of 128 KiB, levels 1 and 6, without and with a base (the same view of a second
matrix, an N(0, 1e-5) update away).  Three legs, alternating in one run, every run listed, GB/s of input, compressed bytes (equal across the
legs: asserted) and torch's peak extra device memory:
  slices      one QZSTD_frontCompressDeviceSlices call on the view's rows
  contiguous  what a caller does today: view.contiguous() (the base's too) inside the window + the Typed / Delta call
  typed       the Typed / Delta call on a tensor that is contiguous already: what the pieces cost
then, in the same run, the kernel through the C ABI with events around ONE launcher call each (tables uploaded inside, from pinned memory)
over an N GiB stage of 128 KiB rows, alternating: qzstd_hip_group_xor, and qzstd_hip_group_pieces with pieces of a whole frame, 8 KiB, 2 KiB and
64 bytes, for k = 1, 2, 4, 8, ms per GiB; and the upload of each piece table alone.  --kernels: the kernel legs alone.

  python tools/device_bench.py --srcslices --gib 1 --reps 3 [--levels 1,6] [--kernels]
--slicecheck: the same view, checked without a contiguous copy — QZSTD_frontFingerprintDeviceSlices, QZSTD_frontCheckDeviceSlices and
QZSTD_frontVerifyDeviceSlices against view.contiguous() + the contiguous call and against that call on a contiguous tensor, level 1, with and
without a base for the verify call; then (or alone, --kernels) the two kernels from pieces beside qzstd_hip_fingerprint / qzstd_hip_ungroup_cmp
  python tools/device_bench.py --slicecheck --gib 1 --reps 3 [--kernels]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qz_device as D  # noqa: E402  (torch first)
import qz_bind as B  # noqa: E402
import qz_corpus as K  # noqa: E402

torch = D.torch


def batch_mixes(size: int):
    """-> {mix: [tensor sizes]}, each summing to `size`"""
    import numpy as np
    rng = np.random.default_rng(2024)
    b, left = [], size
    while left > 0:
        n = min(left, int(np.exp(rng.uniform(np.log(4096), np.log(64 << 20)))))
        b.append(n)
        left -= n
    return {"a_128k": [131072] * (size // 131072), "b_loguniform": b, "c_one": [size]}


def batch_main(a):
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    size = int(a.gib * (1 << 30))
    data = K.by_name("system", size)
    has_batch = hasattr(lib, "QZSTD_frontCompressDeviceBatch")
    ways = [w for w in a.ways.split(",") if w != "batch" or has_batch]
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "timed": "library calls (+ torch.cat for `cat`), every run of %d" % a.reps,
           "batch_call_present": has_batch, "mixes": {}}
    for mix, sizes in batch_mixes(size).items():
        if mix not in a.mixes.split(","):
            continue
        tensors, o = [], 0
        for n in sizes:  # each tensor an allocation of its own
            tensors.append(torch.frombuffer(bytearray(data[o:o + n]), dtype=torch.uint8).to("cuda:0"))
            o += n
        torch.cuda.synchronize()
        res = out["mixes"][mix] = {"tensors": len(sizes), "levels": {}}
        for level in [int(x) for x in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            try:
                stream = torch.cuda.current_stream().cuda_stream
                pairs = [(t.data_ptr(), t.numel()) for t in tensors]
                n_frames = sum((n + a.chunk - 1) // a.chunk for n in sizes)
                fr.reserve_frames(max(n_frames, (size + a.chunk - 1) // a.chunk))

                def batch_pass():
                    return fr.call_device_batch(bufs, nb, nf, stream)[0] == nf

                def loop_pass():
                    return all(fr.call_device(p, n, stream)[0] == (n + a.chunk - 1) // a.chunk for p, n in pairs)

                def cat_pass():
                    whole = torch.cat(tensors)
                    return fr.call_device(whole.data_ptr(), size, stream)[0] == (size + a.chunk - 1) // a.chunk

                passes = {"batch": batch_pass, "loop": loop_pass, "cat": cat_pass}
                if has_batch:
                    bufs, nb, nf = fr.batch(pairs)
                use = [w for w in ways if not (w == "cat" and len(sizes) == 1)]
                runs = {w: [] for w in use}
                for w in use:  # untimed: the device slots, the pinned arenas, first touch of the destination
                    assert passes[w](), w
                for _ in range(a.reps):
                    for w in use:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        ok = passes[w]()
                        dt = time.perf_counter() - t0
                        assert ok, "%s pass failed" % w
                        runs[w].append(round(size / dt / 1e9, 3))
                res["levels"][str(level)] = {w + "_gbps": runs[w] for w in use}
            finally:
                fr.close()
        del tensors
        torch.cuda.empty_cache()
    print(json.dumps(out))


def checksum_main(a):
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    size = int(a.gib * (1 << 30))
    n = (size + a.chunk - 1) // a.chunk
    data = K.by_name("system", size)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    del data
    pieces = [t[o:o + 131072].clone() for o in range(0, size, 131072)]
    torch.cuda.synchronize()
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "levels": {},
           "timed": "library calls (+ t.cpu() for the host leg), GB/s of input, every run of %d, checksum off and on alternating" % a.reps}
    for level in [int(x) for x in a.levels.split(",")]:
        fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
        try:
            fr.reserve(size)
            stream = torch.cuda.current_stream().cuda_stream
            bufs, nb, nf = fr.batch([(p.data_ptr(), p.numel()) for p in pieces])
            fr.reserve_frames(max(n, nf))

            def host_pass():
                h = t.cpu()
                return fr.call_host(h.data_ptr(), size)[0] == n

            def device_pass():
                return fr.call_device(t.data_ptr(), size, stream)[0] == n

            def batch_pass():
                return fr.call_device_batch(bufs, nb, nf, stream)[0] == nf

            legs = [x for x in (("host", host_pass), ("device", device_pass), ("batch", batch_pass)) if x[0] in a.legs.split(",")]
            runs = {"%s_%s_gbps" % (name, ("off", "on")[on]): [] for name, _ in legs for on in (0, 1)}
            for on in (0, 1):  # untimed: first touch of the destination, the device slots, the pinned arenas, the hash buffers
                assert fr.set_checksum(on) == 0
                for name, f in legs:
                    assert f(), name
            c0, d2h = fr.checksum_stats(), {}
            for _ in range(a.reps):
                for on in (0, 1):
                    assert fr.set_checksum(on) == 0
                    for name, f in legs:
                        torch.cuda.synchronize()
                        s0 = fr.stats()
                        t0 = time.perf_counter()
                        ok = f()
                        dt = time.perf_counter() - t0
                        assert ok, "%s pass failed" % name
                        runs["%s_%s_gbps" % (name, ("off", "on")[on])].append(round(size / dt / 1e9, 3))
                        d2h["%s_%s" % (name, ("off", "on")[on])] = round((fr.stats()[2] - s0[2]) / size, 5)
            c1 = fr.checksum_stats()
            res = out["levels"][str(level)] = dict(runs)
            res["d2h_bytes_per_input_byte"] = d2h
            res["frames_hashed_by_gpu_per_rep"] = (c1[0] - c0[0]) // a.reps
            res["frames_hashed_by_libzstd_per_rep"] = (c1[1] - c0[1]) // a.reps
            if not a.no_compare:
                fr.set_checksum(1)
                h = t.cpu()
                r, sizes = fr.call_host(h.data_ptr(), size)
                frames_h = fr.frames(n, sizes)
                r, sizes = fr.call_device(t.data_ptr(), size, stream)
                frames_d = fr.frames(n, sizes)
                res["frames_identical_to_host_path"] = frames_h == frames_d
                res["frames_flagged"] = all(f[4] & 4 for f in frames_d)
                res["compressed_on"] = sum(len(x) for x in frames_d)
        finally:
            fr.close()
    print(json.dumps(out))


def group_main(a):
    import numpy as np
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    size = int(a.gib * (1 << 30)) & ~(a.chunk - 1)
    n = size // a.chunk
    torch.manual_seed(0)
    if a.kernels:
        t = (torch.randn(size // 2 + 8, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8)
        fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
        try:
            fr.reserve(size)
            stream = torch.cuda.current_stream().cuda_stream
            for k in (2, 4, 8):
                assert fr.set_byte_group(k) == 0 and fr.call_device(t.data_ptr(), size, stream)[0] == n
            assert fr.set_byte_group(1) == 0 and fr.call_device(t.data_ptr() + 1, size, stream)[0] == n  # (unaligned: every part gathered)
        finally:
            fr.close()
        print(json.dumps({"bytes": size, "passes": "group k=2, k=4, k=8, then gather; level 1; %d parts each" % (size >> 26)}))
        return
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "data": {},
           "timed": "library calls (+ the torch transposition / t.cpu() and numpy grouping), GB/s of input, every run of %d, legs alternating" % a.reps}
    for kind, dt, k in (("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 4)):
        t = (torch.randn(size // k, device="cuda:0") * 0.02).to(dt)
        torch.cuda.synchronize()
        res = out["data"][kind] = {"elem": k, "levels": {}}
        for level in [int(x) for x in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            try:
                fr.reserve(size)
                stream = torch.cuda.current_stream().cuda_stream

                def off_pass():
                    fr.set_byte_group(1)
                    return fr.call_device(t.data_ptr(), size, stream)

                def on_pass():
                    fr.set_byte_group(k)
                    return fr.call_device(t.data_ptr(), size, stream)

                def torch_pass():
                    fr.set_byte_group(1)
                    g = t.view(torch.uint8).view(n, a.chunk // k, k).transpose(1, 2).contiguous()
                    return fr.call_device(g.data_ptr(), size, stream)

                def host_pass():
                    fr.set_byte_group(1)
                    h = t.cpu().view(torch.uint8).numpy().reshape(n, a.chunk // k, k)
                    g = np.ascontiguousarray(h.transpose(0, 2, 1))
                    return fr.call_host(g.ctypes.data, size)

                legs = [x for x in (("off", off_pass), ("on", on_pass), ("torch", torch_pass), ("host", host_pass)) if x[0] in a.legs.split(",")]
                cell = {name + "_gbps": [] for name, _ in legs}
                for name, f in legs:  # untimed: first touch of the destination, the device slots, the pinned arenas
                    r, sizes = f()
                    assert r == n, name
                    cell["compressed_" + name] = sum(sizes[c] for c in range(n))
                g0 = fr.byte_group_stats()
                for _ in range(a.reps):
                    for name, f in legs:
                        torch.cuda.synchronize()
                        s0 = fr.stats()
                        t0 = time.perf_counter()
                        r, _ = f()
                        dt_s = time.perf_counter() - t0
                        assert r == n, "%s pass failed" % name
                        cell[name + "_gbps"].append(round(size / dt_s / 1e9, 3))
                        cell["d2h_bytes_per_input_byte_" + name] = round((fr.stats()[2] - s0[2]) / size, 4)
                g1 = fr.byte_group_stats()
                cell["grouped_frames_share"] = dict(zip(("sequences_and_literals", "rebuilt", "copied_back"),
                                                        [round((x - y) / max(sum(g1) - sum(g0), 1), 4) for x, y in zip(g1, g0)]))
                res["levels"][str(level)] = cell
            finally:
                fr.close()
        del t
        torch.cuda.empty_cache()
    print(json.dumps(out))


def restore_main(a):
    from concurrent.futures import ThreadPoolExecutor
    import ctypes as C
    z = B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    size = int(a.gib * (1 << 30)) & ~(a.chunk - 1)
    n = size // a.chunk
    torch.manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    if a.kernels:
        t = (torch.randn(size // 2, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8)
        back = torch.empty(size, dtype=torch.uint8, device="cuda:0")
        fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
        try:
            fr.reserve(size)
            for k in (1, 2, 4, 8):
                assert fr.set_byte_group(k) == 0
                r, sizes = fr.call_device(t.data_ptr(), size, stream)
                assert r == n
                back.zero_()
                assert fr.call_restore((fr._dst, fr.stride, sizes), n, fr.out_batch([(back.data_ptr(), size)]), 1, None, stream) == n
                assert torch.equal(back, t)
        finally:
            fr.close()
        print(json.dumps({"bytes": size, "passes": "restore k=1, k=2, k=4, k=8 into one tensor; %d parts each" % max(size >> 26, 1)}))
        return
    L = z.lib
    L.ZSTD_createDCtx.restype = C.c_void_p
    L.ZSTD_freeDCtx.argtypes = [C.c_void_p]
    L.ZSTD_decompressDCtx.restype = C.c_size_t
    L.ZSTD_decompressDCtx.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    ungroup = D.bind_bytegroup(lib).QZSTD_byteUngroup
    pool = ThreadPoolExecutor(a.threads)
    dctx = [L.ZSTD_createDCtx() for _ in range(a.threads)]
    scratch = [C.create_string_buffer(a.chunk) for _ in range(a.threads)]
    pinned = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "level": 1, "data": {},
           "timed": "the calls, the copies and the closing synchronize; GB/s of restored content, every run of %d, legs alternating" % a.reps,
           "baseline": "ZSTD_decompressDCtx (+ QZSTD_byteUngroup) on %d Python threads through ctypes into pinned memory, one copy_ per tensor" % a.threads}
    for kind, dt, k in (("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 4)):
        t = (torch.randn(size // k, device="cuda:0") * 0.02).to(dt).view(torch.uint8)
        one = torch.empty(size, dtype=torch.uint8, device="cuda:0")
        many = [torch.empty(a.chunk, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        shapes = {"one_tensor": [one], "tensors_of_128k": many}
        res = out["data"][kind] = {"elem": k}
        fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
        try:
            fr.reserve(size)
            for label, e in (("grouped", k), ("ungrouped", 1)):
                assert fr.set_byte_group(e) == 0
                r, sizes = fr.call_device(t.data_ptr(), size, stream)
                assert r == n
                frames_at = C.addressof(fr._dst)
                cell = res[label] = {"compressed": sum(sizes[c] for c in range(n))}
                fsize = [sizes[c] for c in range(n)]
                for shape, tensors in shapes.items():
                    bufs = fr.out_batch([(x.data_ptr(), x.numel()) for x in tensors])
                    packed = (fr._dst, fr.stride, sizes)

                    def lib_pass():
                        assert fr.call_restore(packed, n, bufs, len(tensors), None, stream) == n

                    def decode(w):
                        zd, tmp = dctx[w], scratch[w]
                        for c in range(w * n // a.threads, (w + 1) * n // a.threads):
                            to = pinned.data_ptr() + c * a.chunk
                            if e == 1:
                                assert L.ZSTD_decompressDCtx(zd, to, a.chunk, frames_at + c * fr.stride, fsize[c]) == a.chunk
                            else:
                                assert L.ZSTD_decompressDCtx(zd, tmp, a.chunk, frames_at + c * fr.stride, fsize[c]) == a.chunk
                                ungroup(to, tmp, a.chunk, e)

                    def baseline_pass():
                        list(pool.map(decode, range(a.threads)))
                        if len(tensors) == 1:
                            tensors[0].copy_(pinned, non_blocking=True)
                        else:
                            for c, x in enumerate(tensors):
                                x.copy_(pinned[c * a.chunk:(c + 1) * a.chunk], non_blocking=True)

                    runs = cell[shape] = {"lib_gbps": [], "baseline_gbps": []}
                    for name, f in (("lib", lib_pass), ("baseline", baseline_pass)):  # untimed, and checked
                        for x in tensors:
                            x.zero_()
                        f()
                        torch.cuda.synchronize()
                        assert torch.equal(tensors[0] if len(tensors) == 1 else torch.cat(tensors), t), (kind, label, shape, name)
                    for _ in range(a.reps):
                        for name, f in (("lib", lib_pass), ("baseline", baseline_pass)):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            f()
                            torch.cuda.synchronize()
                            runs[name + "_gbps"].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
        finally:
            fr.close()
        del t, one, many, shapes
        torch.cuda.empty_cache()
    for zd in dctx:
        L.ZSTD_freeDCtx(zd)
    print(json.dumps(out))


def delta_kernels(a, size):
    """the four staging kernels over the same rows, per element size: qzstd_hip_group_xor / qzstd_hip_group into a stage, then
    qzstd_hip_ungroup_xor / qzstd_hip_ungroup out of it"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_xor_kernels(plug.lib)
    for fn in (L.qzstd_hip_group, L.qzstd_hip_ungroup):
        fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    n = size // a.chunk
    src = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0")
    stage = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.GroupXorRow))
    assert d_rows and stage.data_ptr() % 16 == 0
    want = torch.bitwise_xor(src, base)
    try:
        for k in (1, 2, 4, 8):
            gx, g, ux, u = (D.GroupXorRow * n)(), (D.GroupRow * n)(), (D.UngroupXorRow * n)(), (D.UngroupRow * n)()
            for c in range(n):
                o = c * a.chunk
                gx[c].src, gx[c].base, gx[c].dstOff, gx[c].len, gx[c].pad, gx[c].elem = src.data_ptr() + o, base.data_ptr() + o, o, a.chunk, 0, k
                g[c].src, g[c].dstOff, g[c].len, g[c].pad, g[c].elem = want.data_ptr() + o, o, a.chunk, 0, k
                ux[c].dst, ux[c].base, ux[c].srcOff, ux[c].len, ux[c].elem = dst.data_ptr() + o, base.data_ptr() + o, o, a.chunk, k
                u[c].dst, u[c].srcOff, u[c].len, u[c].elem = dst.data_ptr() + o, o, a.chunk, k
            torch.cuda.synchronize()
            for fn, rows in ((L.qzstd_hip_group, g), (L.qzstd_hip_group_xor, gx)):  # both leave group(src ^ base) in the stage
                assert fn(0, None, rows, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
                plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert L.qzstd_hip_ungroup(0, None, u, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert torch.equal(dst, want), k
            assert L.qzstd_hip_ungroup_xor(0, None, ux, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert torch.equal(dst, src), k
    finally:
        L.qzstd_hip_free(0, d_rows)
    print(json.dumps({"bytes": size, "passes": "per element size 1, 2, 4, 8: group, group_xor, ungroup, ungroup_xor over %d rows of %d bytes" % (n, a.chunk)}))


def delta_main(a):
    size = int(a.gib * (1 << 30)) & ~(a.chunk - 1)
    if a.kernels:
        return delta_kernels(a, size)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "step": 1e-5, "data": {},
           "timed": "the calls, the torch passes and the closing synchronize; GB/s of input (compress) and of restored content (restore), every "
                    "run of %d, legs alternating" % a.reps,
           "torch_leg": "bitwise_xor into a fresh temporary + QZSTD_frontCompressDeviceBatchTyped; QZSTD_frontRestoreDeviceBatchTyped into a fresh "
                        "temporary + bitwise_xor_ into the base"}
    for kind, dt, k in (("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 4)):
        base_f = (torch.randn(size // k, device="cuda:0") * 0.02).to(dt)
        new = (base_f.float() + torch.randn(size // k, device="cuda:0") * 1e-5).to(dt).view(torch.uint8)
        base = base_f.view(torch.uint8)
        work = torch.empty_like(base)  # the restore legs' "previous checkpoint": refilled from `base` before every run
        res = out["data"][kind] = {"elem": k, "levels": {}}
        for level in [int(x) for x in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            cell = res["levels"][str(level)] = {}
            try:
                fr.reserve(size)
                n = size // a.chunk
                bufs_new, _, _ = fr.batch([(new.data_ptr(), size)])
                bufs_base, _, _ = fr.batch([(base.data_ptr(), size)])
                es = bytes([k]) + b"\0"
                _, sizes = fr._frame_buffers(n)

                def grouped_alone():
                    return fr.lib.QZSTD_frontCompressDeviceBatchTyped(fr.f, bufs_new, es, 1, stream, fr._dst, len(fr._dst), sizes, None)

                def delta_compress():
                    return fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, bufs_new, bufs_base, es, 1, stream, fr._dst, len(fr._dst), sizes, None)

                def torch_compress():
                    tmp = torch.bitwise_xor(new, base)
                    b, _, _ = fr.batch([(tmp.data_ptr(), size)])
                    return fr.lib.QZSTD_frontCompressDeviceBatchTyped(fr.f, b, es, 1, stream, fr._dst, len(fr._dst), sizes, None)

                assert grouped_alone() == n
                cell["compressed_grouped"] = sum(sizes[c] for c in range(n))
                assert torch_compress() == n
                cell["compressed_torch"] = sum(sizes[c] for c in range(n))
                s0 = fr.stats()
                assert delta_compress() == n
                s1 = fr.stats()
                cell["compressed_delta"] = sum(sizes[c] for c in range(n))
                cell["d2h_bytes_per_input_byte_delta"] = round((s1[2] - s0[2]) / size, 4)
                cell["ratio_grouped"] = round(cell["compressed_grouped"] / size, 4)
                cell["ratio_delta"] = round(cell["compressed_delta"] / size, 4)
                cell["delta_frames_by_build"] = fr.delta_stats()[:3]
                runs = {"delta_gbps": [], "torch_gbps": [], "restore_delta_gbps": [], "restore_torch_gbps": []}
                for _ in range(a.reps):
                    for name, f in (("delta", delta_compress), ("torch", torch_compress)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert f() == n
                        torch.cuda.synchronize()
                        runs[name + "_gbps"].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
                # the way back, from the delta frames (the last compress left the torch leg's, which are the same bytes)
                assert delta_compress() == n
                packed = (fr._dst, fr.stride, sizes)
                out_work = fr.out_batch([(work.data_ptr(), size)])
                base_work, _, _ = fr.batch([(work.data_ptr(), size)])

                def delta_restore():
                    return fr.lib.QZSTD_frontRestoreDeviceBatchDelta(fr.f, packed[0], packed[1], packed[2], n, out_work, base_work, es, 1, stream)

                def torch_restore():
                    tmp = torch.empty_like(work)
                    r = fr.call_restore(packed, n, fr.out_batch([(tmp.data_ptr(), size)]), 1, [k], stream)
                    work.bitwise_xor_(tmp)
                    return r

                for name, f in (("delta", delta_restore), ("torch", torch_restore)):  # untimed, and checked
                    work.copy_(base)
                    assert f() == n
                    torch.cuda.synchronize()
                    assert torch.equal(work, new), (kind, level, name)
                for _ in range(a.reps):
                    for name, f in (("delta", delta_restore), ("torch", torch_restore)):
                        work.copy_(base)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert f() == n
                        torch.cuda.synchronize()
                        runs["restore_" + name + "_gbps"].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
                cell.update(runs)
            finally:
                fr.close()
        del base_f, new, base, work
        torch.cuda.empty_cache()
    print(json.dumps(out))


def slices_kernels(a, size):
    """through the C ABI, nothing timed, per element size 1, 2, 4, 8 over the same stage of N GiB of 128 KiB frames: qzstd_hip_ungroup_xor, then
    qzstd_hip_ungroup_window with whole-frame windows (both with a base: the same bytes written), then qzstd_hip_ungroup_window with a column
    shard's windows — 2 KiB of every 16 KiB of each frame, 1/8 of the bytes"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_window_kernel(D.bind_xor_kernels(plug.lib))
    n, row, piece = size // a.chunk, 16384, 2048
    per = a.chunk // row
    stage = torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    dst2 = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * per * C.sizeof(D.UngroupWinRow))
    assert d_rows and stage.data_ptr() % 16 == 0
    try:
        for k in (1, 2, 4, 8):
            ux, w, col = (D.UngroupXorRow * n)(), (D.UngroupWinRow * n)(), (D.UngroupWinRow * (n * per))()
            for c in range(n):
                o = c * a.chunk
                ux[c].dst, ux[c].base, ux[c].srcOff, ux[c].len, ux[c].elem = dst.data_ptr() + o, base.data_ptr() + o, o, a.chunk, k
                w[c].dst, w[c].base, w[c].srcOff, w[c].len, w[c].elem, w[c].winOff, w[c].winLen = dst2.data_ptr() + o, base.data_ptr() + o, o, a.chunk, k, 0, a.chunk
                for j in range(per):
                    r = col[c * per + j]
                    r.dst, r.base, r.srcOff, r.len, r.elem = dst2.data_ptr() + (c * per + j) * piece, base.data_ptr() + (c * per + j) * piece, o, a.chunk, k
                    r.winOff, r.winLen = j * row + 3 * piece, piece
            torch.cuda.synchronize()
            assert L.qzstd_hip_ungroup_xor(0, None, ux, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert L.qzstd_hip_ungroup_window(0, None, w, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert torch.equal(dst, dst2), k
            assert L.qzstd_hip_ungroup_window(0, None, col, n * per, d_rows, stage.data_ptr(), size) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            want = torch.bitwise_xor(dst, base).view(n * per, row)[:, 3 * piece:4 * piece].reshape(-1)  # (the ungrouped frames, the shard's columns)
            assert torch.equal(torch.bitwise_xor(dst2[:n * per * piece], base[:n * per * piece]), want), k
    finally:
        L.qzstd_hip_free(0, d_rows)
    print(json.dumps({"bytes": size, "passes": "per element size 1, 2, 4, 8: ungroup_xor over %d rows of %d bytes, ungroup_window over the same as whole-frame "
                                               "windows, ungroup_window over %d windows of %d bytes (%d bytes written)" % (n, a.chunk, n * per, piece, n * per * piece)}))


def slices_main(a):
    """--slices: a resharded load.  N GiB of bf16 and of fp32 weights as 2-D tensors with rows of 16 KiB, level-1 grouped frames, written with
    and without a base; leg A: QZSTD_frontRestoreDeviceSlices of a 1/8 row shard and of a 1/8 column shard (2 KiB of every row); leg B: what a
    caller does today — QZSTD_frontRestoreDeviceBatchDelta of the whole tensor into a temporary, then narrow().copy_()"""
    size = int(a.gib * (1 << 30)) & ~(8 * a.chunk - 1)
    if a.kernels:
        return slices_kernels(a, size)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    rowb = 16384
    R = size // rowb
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "level": 1, "rows": R, "row_bytes": rowb, "data": {},
           "timed": "the calls, the copies and the closing synchronize; seconds per load, every run of %d, legs alternating" % a.reps,
           "legs": "A: QZSTD_frontRestoreDeviceSlices; B: QZSTD_frontRestoreDeviceBatchDelta of the whole tensor into a temporary allocated inside "
                   "the window, then narrow().copy_()",
           "peak_extra_device_bytes": "torch's peak allocation above the level before the call (the temporary); the library's two device stages "
                                      "(one part each) are the same in both legs and not included"}
    n = size // a.chunk
    for kind, dt, k in (("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 4)):
        Cc = rowb // k
        base_f = (torch.randn(size // k, device="cuda:0") * 0.02).to(dt)
        new = (base_f.float() + torch.randn(size // k, device="cuda:0") * 1e-5).to(dt).view(R, Cc)
        base = base_f.view(R, Cc)
        res = out["data"][kind] = {"elem": k, "cells": {}}
        fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
        try:
            for based in (False, True):
                fr.reserve(size)
                _, sizes = fr._frame_buffers(n)
                assert fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, fr.batch([(new.data_ptr(), size)])[0], fr.batch([(base.data_ptr(), size)])[0] if based else None,
                                                                  bytes([k]) + b"\0", 1, stream, fr._dst, len(fr._dst), sizes, None) == n
                packed = (fr._dst, fr.stride, sizes)  # the frames where the compress call left them
                for shard, dim in (("row", 0), ("column", 1)):
                    start, length = (R // 8 * 3, R // 8) if dim == 0 else (Cc // 8 * 3, Cc // 8)
                    want = new.narrow(dim, start, length).contiguous()
                    dst = torch.empty_like(want)
                    bshard = base.narrow(dim, start, length).contiguous() if based else None
                    sl = D.shard_slices(0, (R, Cc), k, dim, start, length, dst.data_ptr(), None if bshard is None else bshard.data_ptr())
                    arr = fr.slice_array(sl)
                    whole_base, _, _ = fr.batch([(base.data_ptr(), size)])

                    def leg_a():
                        return fr.call_restore_slices(packed, n, [size], [k], arr, len(sl), stream)

                    def leg_b():
                        tmp = torch.empty_like(new)
                        r = fr.lib.QZSTD_frontRestoreDeviceBatchDelta(fr.f, packed[0], packed[1], packed[2], n, fr.out_batch([(tmp.data_ptr(), size)]),
                                                                      whole_base if based else None, bytes([k]) + b"\0", 1, stream)
                        dst.copy_(tmp.narrow(dim, start, length))
                        return r

                    cell = res["cells"]["%s_%s" % (shard, "base" if based else "nobase")] = {"slices": len(sl), "bytes_written": want.numel() * k}
                    for name, f in (("A", leg_a), ("B", leg_b)):  # untimed, and checked
                        dst.zero_()
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        m0, r0 = torch.cuda.memory_allocated(), fr.restore_stats()
                        got = f()
                        torch.cuda.synchronize()
                        r1, peak = fr.restore_stats(), torch.cuda.max_memory_allocated() - m0  # (before the comparison below allocates)
                        assert got == r1[0] - r0[0] and got != D.ERROR and torch.equal(dst, want), (kind, shard, based, name)
                        cell[name] = {"frames_decoded": got, "h2d_bytes": r1[2] - r0[2], "peak_extra_device_bytes": peak, "seconds": []}
                    for _ in range(a.reps):
                        for name, f in (("A", leg_a), ("B", leg_b)):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            f()
                            torch.cuda.synchronize()
                            cell[name]["seconds"].append(round(time.perf_counter() - t0, 4))
                    del want, dst, bshard
                del packed
        finally:
            fr.close()
        del base_f, new, base
        torch.cuda.empty_cache()
    print(json.dumps(out))


def skip_kernels(a, size):
    """through the C ABI, nothing timed: qzstd_hip_diff over N GiB of 128 KiB rows (equal rows, rows that differ, and a and b at different
    alignments mod 16), and qzstd_hip_group_xor over the same rows for element size 2: the run to put under rocprofv3"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_diff_kernel(D.bind_xor_kernels(plug.lib))
    n = size // a.chunk
    src = torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda:0")
    same = src.clone()
    other = torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda:0")
    stage = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    flags = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.GroupXorRow))
    assert d_rows and stage.data_ptr() % 16 == 0
    try:
        for name, b, skew, want in (("equal", same, 0, 0), ("different", other, 0, 1), ("equal, b 7 bytes off", same, 7, 0)):
            rows = (D.DiffRow * n)()
            if skew:
                b = torch.empty_like(same)
                b[skew:] = same[:-skew]
            for c in range(n):
                rows[c].a, rows[c].b, rows[c].len = src.data_ptr() + c * a.chunk, b.data_ptr() + skew + c * a.chunk, a.chunk
            torch.cuda.synchronize()
            assert L.qzstd_hip_diff(0, None, rows, n, d_rows, flags.data_ptr()) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert bool((flags == want).all()), name
        gx = (D.GroupXorRow * n)()
        for c in range(n):
            o = c * a.chunk
            gx[c].src, gx[c].base, gx[c].dstOff, gx[c].len, gx[c].pad, gx[c].elem = src.data_ptr() + o, other.data_ptr() + o, o, a.chunk, 0, 2
        assert L.qzstd_hip_group_xor(0, None, gx, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    print(json.dumps({"bytes": size, "passes": "qzstd_hip_diff over %d rows of %d bytes: equal, different, equal with b 7 bytes off; then qzstd_hip_group_xor "
                                               "(element size 2) over the same rows" % (n, a.chunk)}))


def skip_main(a):
    """--skip: delta skip (QZSTD_frontSetDeltaSkip) on a checkpoint of which a share did not change"""
    import ctypes as C
    size = int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1)
    if a.kernels:
        return skip_kernels(a, size)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    nt, per = 64, size // 64
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "tensors": nt, "tensor_bytes": per, "step": 1e-5, "dtype": "bf16", "cells": {},
           "timed": "the calls and the closing synchronize; GB/s of input (compress) and of restored content (restore), every run of %d, the setting "
                    "off and on alternating; restore: off = the setting-off call's frames restored with the setting off, on = the setting-on call's "
                    "frames restored with the setting on; in place over a copy of the bases (refilled outside the window) and into fresh tensors" % a.reps,
           "d2h": "QZSTD_frontDeviceStats [2] per input byte; the on leg's flags (4 bytes per compared frame) are listed apart as flag_bytes"}
    bases = [(torch.randn(per // 2, device="cuda:0") * 0.02).to(torch.bfloat16) for _ in range(nt)]
    stepped = [(b.float() + torch.randn(per // 2, device="cuda:0") * 1e-5).to(torch.bfloat16) for b in bases]
    work = [torch.empty_like(b) for b in bases]
    fresh = [torch.empty_like(b) for b in bases]
    n = size // a.chunk
    for share in (0.0, 0.5, 0.9, 1.0):
        frozen = [int((i + 1) * share) > int(i * share) for i in range(nt)]  # evenly spread
        new = [b if fz else s for b, s, fz in zip(bases, stepped, frozen)]
        assert all(fz or not torch.equal(x, b) for x, b, fz in zip(new, bases, frozen))
        for level in [int(x) for x in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            cell = out["cells"]["p=%g,level=%d" % (share, level)] = {"frozen_tensors": sum(frozen)}
            try:
                fr.reserve(size)
                es = bytes([2] * nt) + b"\0"
                bufs_new, _, _ = fr.batch([(x.data_ptr(), per) for x in new])
                bufs_base, _, _ = fr.batch([(x.data_ptr(), per) for x in bases])
                bufs_work, _, _ = fr.batch([(x.data_ptr(), per) for x in work])
                out_work = fr.out_batch([(x.data_ptr(), per) for x in work])
                out_fresh = fr.out_batch([(x.data_ptr(), per) for x in fresh])
                _, sizes = fr._frame_buffers(n)
                kept = {}

                def compress(on):
                    assert fr.set_delta_skip(on) == 0
                    return fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, bufs_new, bufs_base, es, nt, stream, fr._dst, len(fr._dst), sizes, None)

                def restore(on, in_place):
                    buf, sz = kept[on]
                    assert fr.set_delta_skip(on) == 0
                    return fr.lib.QZSTD_frontRestoreDeviceBatchDelta(fr.f, buf, fr.stride, sz, n, out_work if in_place else out_fresh,
                                                                     bufs_work if in_place else bufs_base, es, nt, stream)

                for on in (0, 1):  # untimed: the slots, and what each setting leaves
                    s0, k0 = fr.stats(), fr.delta_skip_stats()
                    assert compress(on) == n
                    s1, k1 = fr.stats(), fr.delta_skip_stats()
                    tag = "on" if on else "off"
                    cell["compressed_" + tag] = sum(sizes[c] for c in range(n))
                    cell["d2h_bytes_per_input_byte_" + tag] = round((s1[2] - s0[2]) / size, 5)
                    if on:
                        cell["flag_bytes"] = 4 * (k1[0] - k0[0])
                        cell["frames_compared_equal"] = [k1[0] - k0[0], k1[1] - k0[1]]
                    buf = C.create_string_buffer(n * fr.stride)
                    C.memmove(buf, fr._dst, n * fr.stride)
                    kept[on] = (buf, (C.c_size_t * n)(*sizes[:n]))
                runs = {"compress_off_gbps": [], "compress_on_gbps": [], "restore_in_place_off_gbps": [], "restore_in_place_on_gbps": [],
                        "restore_fresh_off_gbps": [], "restore_fresh_on_gbps": []}
                for _ in range(a.reps):
                    for on in (0, 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert compress(on) == n
                        torch.cuda.synchronize()
                        runs["compress_%s_gbps" % ("on" if on else "off")].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
                for in_place in (True, False):
                    where = "in_place" if in_place else "fresh"
                    for on in (0, 1):  # untimed, and checked
                        for w, b in zip(work, bases):
                            w.copy_(b)
                        r0 = fr.restore_stats()
                        assert restore(on, in_place) == n
                        torch.cuda.synchronize()
                        cell["h2d_bytes_per_input_byte_%s_%s" % (where, "on" if on else "off")] = round((fr.restore_stats()[2] - r0[2]) / size, 5)
                        assert all(torch.equal(g, x) for g, x in zip(work if in_place else fresh, new)), (share, level, where, on)
                    for _ in range(a.reps):
                        for on in (0, 1):
                            for w, b in zip(work, bases):
                                w.copy_(b)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            assert restore(on, in_place) == n
                            torch.cuda.synchronize()
                            runs["restore_%s_%s_gbps" % (where, "on" if on else "off")].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
                cell.update(runs)
            finally:
                fr.close()
    print(json.dumps(out))


def verify_kernels(a, size):
    """through the C ABI, nothing timed: for k = 1, 2, 4, 8 ONE qzstd_hip_ungroup_xor launch over an N GiB stage of 128 KiB frames (base XORed in,
    a destination written) and ONE qzstd_hip_ungroup_cmp launch over the same stage and base against that destination as the live bytes —
    every tile word must say "same"; then one launch with a bit changed.  The run to put under rocprofv3"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_cmp_kernel(D.bind_xor_kernels(plug.lib))
    n = size // a.chunk
    stage = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    tiles = torch.empty(size >> 14, dtype=torch.int32, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.UngroupCmpRow))
    assert d_rows and stage.data_ptr() % 16 == 0
    try:
        for k in (1, 2, 4, 8):
            ux = (D.UngroupXorRow * n)()
            cr = (D.UngroupCmpRow * n)()
            for c in range(n):
                o = c * a.chunk
                ux[c].dst, ux[c].base, ux[c].srcOff, ux[c].len, ux[c].elem = dst.data_ptr() + o, base.data_ptr() + o, o, a.chunk, k
                cr[c].ref, cr[c].base, cr[c].srcOff, cr[c].len, cr[c].elem, cr[c].flags = dst.data_ptr() + o, base.data_ptr() + o, o, a.chunk, k, 0
            torch.cuda.synchronize()
            assert L.qzstd_hip_ungroup_xor(0, None, ux, n, d_rows, stage.data_ptr(), size) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            tiles.fill_(7)
            torch.cuda.synchronize()
            assert L.qzstd_hip_ungroup_cmp(0, None, cr, n, d_rows, stage.data_ptr(), size, tiles.data_ptr()) == 0, plug.err()
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
            assert bool((tiles == -1).all()), k
        dst[5 * a.chunk + 16385] ^= 1  # (k = 8 still staged)
        torch.cuda.synchronize()
        assert L.qzstd_hip_ungroup_cmp(0, None, cr, n, d_rows, stage.data_ptr(), size, tiles.data_ptr()) == 0, plug.err()
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
        hit = torch.nonzero(tiles != -1).flatten().tolist()
        assert hit == [5 * (a.chunk >> 14) + 1] and int(tiles[hit[0]]) == 16385
    finally:
        L.qzstd_hip_free(0, d_rows)
    print(json.dumps({"bytes": size, "passes": "for k = 1, 2, 4, 8: qzstd_hip_ungroup_xor, then qzstd_hip_ungroup_cmp, each ONE launch over %d frames of %d "
                                               "bytes with a base; a last qzstd_hip_ungroup_cmp launch (k = 8) with one bit changed" % (n, a.chunk)}))


def verify_main(a):
    """--verify: QZSTD_frontVerifyDeviceBatch against what a caller does without it — QZSTD_frontRestoreDeviceBatchDelta into fresh tensors and
    torch.equal per tensor — on a checkpoint just written as level-1 grouped delta frames"""
    import ctypes as C
    size = int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1)
    if a.kernels:
        return verify_kernels(a, size)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    n = size // a.chunk
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "level": 1, "step": 1e-5, "reps": a.reps, "cells": {},
           "timed": "ms per check, every run, the two legs alternating in one run: verify = QZSTD_frontVerifyDeviceBatch (firstDiff given) and the "
                    "closing synchronize; restore_equal = torch.empty_like per tensor, the array of their addresses, QZSTD_frontRestoreDeviceBatchDelta into them, torch.equal per "
                    "tensor (its answer read on the host), the tensors dropped",
           "h2d": "verify: computed from the frames — the call copies pad16(len) bytes per frame that is not a recognised canonical zero frame (the "
                  "library keeps no counter of it), plus 32 bytes per row up and 4 bytes per 16 KiB back; restore_equal: QZSTD_frontRestoreStats [2]",
           "peak": "torch.cuda.max_memory_allocated() - memory_allocated() before the leg: torch's allocator only; the library's two restore slots "
                   "(pinned + device stage of a part each) are the same in both legs and are not in it"}
    for dt, tdt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        k = 2 if dt == "bf16" else 4
        base = (torch.randn(size // k, device="cuda:0") * 0.02).to(tdt)
        stepped = (base.float() + torch.randn(size // k, device="cuda:0") * 1e-5).to(tdt)
        for layout, nt in (("one_tensor", 1), ("8192_tensors", size // a.chunk)):
            per = size // nt
            for share in (0.0, 0.5):
                # p = 0.5: every other 128 KiB chunk did not change
                new = stepped.clone()
                if share:
                    v, bv = new.view(n, -1), base.view(n, -1)
                    v[::2] = bv[::2]
                tensors = [new[i * (per // k):(i + 1) * (per // k)] for i in range(nt)]
                bases = [base[i * (per // k):(i + 1) * (per // k)] for i in range(nt)]
                fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
                cell = out["cells"]["%s,%s,skip=%s" % (dt, layout, "on,p=0.5" if share else "off")] = {}
                try:
                    fr.reserve(size)
                    assert fr.set_delta_skip(1 if share else 0) == 0
                    es = bytes([k] * nt) + b"\0"
                    bufs_new, _, _ = fr.batch([(x.data_ptr(), per) for x in tensors])
                    bufs_base, _, _ = fr.batch([(x.data_ptr(), per) for x in bases])
                    _, sizes = fr._frame_buffers(n)
                    assert fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, bufs_new, bufs_base, es, nt, stream, fr._dst, len(fr._dst), sizes, None) == n
                    frames = C.create_string_buffer(n * fr.stride)
                    C.memmove(frames, fr._dst, n * fr.stride)
                    zero = D.zero_frame(a.chunk)
                    n_zero = sum(1 for c in range(n) if sizes[c] == len(zero) and C.string_at(C.addressof(frames) + c * fr.stride, len(zero)) == zero) if share else 0
                    cell["compressed"] = sum(sizes[c] for c in range(n))
                    cell["zero_frames"] = n_zero
                    first = (C.c_size_t * n)()

                    def verify():
                        return fr.lib.QZSTD_frontVerifyDeviceBatch(fr.f, frames, fr.stride, sizes, n, bufs_new, bufs_base, es, nt, stream, first)

                    def restore_equal():
                        fresh = [torch.empty_like(t) for t in tensors]
                        outs = fr.out_batch([(x.data_ptr(), per) for x in fresh])
                        assert fr.lib.QZSTD_frontRestoreDeviceBatchDelta(fr.f, frames, fr.stride, sizes, n, outs, bufs_base, es, nt, stream) == n
                        return 0 if all(torch.equal(f, t) for f, t in zip(fresh, tensors)) else 1

                    runs = {"verify_ms": [], "restore_equal_ms": [], "verify_peak_bytes": [], "restore_equal_peak_bytes": []}
                    for name, leg in (("verify", verify), ("restore_equal", restore_equal)):  # untimed: the slots
                        r0 = fr.restore_stats()
                        assert leg() == 0
                        torch.cuda.synchronize()
                        cell[name + "_h2d_bytes"] = (n - n_zero) * a.chunk if name == "verify" else fr.restore_stats()[2] - r0[2]
                    for _ in range(a.reps):
                        for name, leg in (("verify", verify), ("restore_equal", restore_equal)):
                            torch.cuda.synchronize()
                            torch.cuda.reset_peak_memory_stats()
                            m0 = torch.cuda.memory_allocated()
                            t0 = time.perf_counter()
                            assert leg() == 0
                            torch.cuda.synchronize()
                            runs[name + "_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
                            runs[name + "_peak_bytes"].append(torch.cuda.max_memory_allocated() - m0)
                    cell.update(runs)
                    # the answer is worth something: one bit of the live data, found at its place
                    new.view(torch.uint8)[3 * a.chunk + 16385] ^= 1
                    torch.cuda.synchronize()
                    assert verify() == 1 and first[3] == 16385 and restore_equal() == 1
                    cell["verify_stats"] = fr.verify_stats()
                finally:
                    fr.close()
                del tensors, bases, new
        del base, stepped
    print(json.dumps(out))


def probe_kernels(a, size):
    """--probe --kernels: qzstd_hip_plane_cost beside qzstd_hip_group over the same N GiB, ms per GiB from events around one launch each"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_plane_kernel(D.bind_xor_kernels(plug.lib))
    L.qzstd_hip_group.restype = C.c_int
    L.qzstd_hip_group.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    n = size // a.chunk
    torch.manual_seed(0)
    w = (torch.randn(size // 2, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8)
    noise = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0")
    expo = w.view(-1, 2)[:, 1].repeat(2).contiguous()  # the high bytes, twice: N GiB of exponent plane
    stage = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    cost = torch.empty(2 * n, dtype=torch.int32, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, 2 * n * C.sizeof(D.GroupRow))
    assert d_rows and stage.data_ptr() % 16 == 0
    gib = size / float(1 << 30)
    out = {"bytes": size, "rows": n, "row_bytes": a.chunk, "timed": "events around one launch (rows uploaded inside), ms per GiB, every run of %d after one untimed" % a.reps}

    def timed(call):
        runs = []
        for i in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert call() == 0, plug.err()
            e1.record()
            torch.cuda.synchronize()
            if i:
                runs.append(round(e0.elapsed_time(e1) / gib, 3))
        return runs

    try:
        gr = (D.GroupRow * n)()
        for c in range(n):
            gr[c].src, gr[c].dstOff, gr[c].len, gr[c].pad, gr[c].elem = w.data_ptr() + c * a.chunk, c * a.chunk, a.chunk, 0, 2
        out["group_k2_ms_per_gib"] = timed(lambda: L.qzstd_hip_group(0, None, gr, n, d_rows, stage.data_ptr(), size))
        rows = (D.PlaneRow * n)(*[D.PlaneRow(c * a.chunk, a.chunk, 0) for c in range(n)])
        out["plane_cost_noise_ms_per_gib"] = timed(lambda: L.qzstd_hip_plane_cost(0, None, noise.data_ptr(), rows, n, d_rows, cost.data_ptr()))
        out["noise_cost_per_row"] = [int(cost[:n].min()), int(cost[:n].max())]
        out["plane_cost_exponent_ms_per_gib"] = timed(lambda: L.qzstd_hip_plane_cost(0, None, expo.data_ptr(), rows, n, d_rows, cost.data_ptr()))
        out["exponent_cost_per_row"] = [int(cost[:n].min()), int(cost[:n].max())]
        half = a.chunk // 2
        planes = (D.PlaneRow * (2 * n))(*[D.PlaneRow(c * half, half, 0) for c in range(2 * n)])
        out["plane_cost_grouped_stage_ms_per_gib"] = timed(lambda: L.qzstd_hip_plane_cost(0, None, stage.data_ptr(), planes, 2 * n, d_rows, cost.data_ptr()))
    finally:
        L.qzstd_hip_free(0, d_rows)
    print(json.dumps(out))


def probe_main(a):
    """--probe: the grouped device call with the plane probe off and on"""
    size = int(a.gib * (1 << 30)) & ~(a.chunk - 1)
    if a.kernels:
        return probe_kernels(a, size)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    n = size // a.chunk
    torch.manual_seed(0)
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "data": {},
           "timed": "QZSTD_frontCompressDevice with byte grouping on, GB/s of input, every run of %d, the plane probe off and on alternating" % a.reps}
    for kind, dt, k in (("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 4)):
        t = (torch.randn(size // k, device="cuda:0") * 0.02).to(dt)
        torch.cuda.synchronize()
        res = out["data"][kind] = {"elem": k, "levels": {}}
        for level in [int(x) for x in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            try:
                fr.reserve(size)
                stream = torch.cuda.current_stream().cuda_stream
                assert fr.set_byte_group(k) == 0
                cell = {"off_gbps": [], "on_gbps": []}
                for on in (0, 1):  # untimed: first touch of the destination, the device slots, the pinned arenas
                    tag = "on" if on else "off"
                    assert fr.set_plane_probe(on) == 0
                    s0, p0 = fr.stats(), fr.plane_probe_stats()
                    r, sizes = fr.call_device(t.data_ptr(), size, stream)
                    assert r == n, tag
                    s1, p1 = fr.stats(), fr.plane_probe_stats()
                    cell["compressed_" + tag] = sum(sizes[c] for c in range(n))
                    cell["d2h_bytes_per_input_byte_" + tag] = round((s1[2] - s0[2]) / size, 5)
                    cell["frames_from_the_arena_" + tag] = round((s1[0] - s0[0]) / n, 4)
                    if on:
                        cell["blocks_probed_raw"] = [p1[0] - p0[0], p1[1] - p0[1]]
                        cell["frames_assembled_share"] = round((p1[2] - p0[2]) / n, 4)
                        cell["frames_fell_back_share"] = round((p1[3] - p0[3]) / n, 4)
                for _ in range(a.reps):
                    for on in (0, 1):
                        assert fr.set_plane_probe(on) == 0
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r, _ = fr.call_device(t.data_ptr(), size, stream)
                        dt_s = time.perf_counter() - t0
                        assert r == n
                        cell["on_gbps" if on else "off_gbps"].append(round(size / dt_s / 1e9, 3))
                res["levels"][str(level)] = cell
            finally:
                fr.close()
        del t
        torch.cuda.empty_cache()
    print(json.dumps(out))


def code_kernels(a, size):
    """--code --kernels: qzstd_hip_huf_code (its four launches) beside qzstd_hip_plane_cost over the same N GiB of exponent plane and of noise,
    rows of --chunk bytes, ms per GiB from events around the call, the two alternating"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_huf_kernel(D.bind_plane_kernel(plug.lib))
    n = size // a.chunk
    torch.manual_seed(0)
    w = (torch.randn(size // 2, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8)
    expo = w.view(-1, 2)[:, 1].repeat(2).contiguous()  # the high bytes, twice: N GiB of exponent plane
    del w
    noise = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0")
    rows = (D.PlaneRow * n)(*[D.PlaneRow(c * a.chunk, a.chunk, 0) for c in range(n)])
    need = L.qzstd_hip_huf_code_bytes(rows, n)
    words = torch.empty(3 * n + 1, dtype=torch.int32, device="cuda:0")
    dense = torch.empty(need + 16, dtype=torch.uint8, device="cuda:0")
    scratch = torch.empty(D.huf_scratch_bytes(n, need) + 16, dtype=torch.uint8, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.PlaneRow))
    assert d_rows and dense.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0
    gib = size / float(1 << 30)
    out = {"bytes": size, "rows": n, "row_bytes": a.chunk,
           "timed": "events around one call (rows uploaded inside), ms per GiB, every run of %d after one untimed, the kernels alternating" % a.reps}
    calls = {}
    for name, t in (("exponent", expo), ("noise", noise)):
        calls["plane_cost_%s_ms_per_gib" % name] = lambda t=t: L.qzstd_hip_plane_cost(0, None, t.data_ptr(), rows, n, d_rows, words.data_ptr())
        calls["huf_code_%s_ms_per_gib" % name] = lambda t=t: L.qzstd_hip_huf_code(
            0, None, t.data_ptr(), rows, n, d_rows, words.data_ptr(), words.data_ptr() + 4 * n, words.data_ptr() + 8 * n, dense.data_ptr(), need,
            scratch.data_ptr(), D.huf_scratch_bytes(n, need))
    try:
        for key in calls:
            out[key] = []
        for i in range(a.reps + 1):
            for key, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                assert call() == 0, plug.err()
                e1.record()
                torch.cuda.synchronize()
                if i:
                    out[key].append(round(e0.elapsed_time(e1) / gib, 3))
                if key.startswith("huf_code"):
                    out[key.replace("_ms_per_gib", "_dense_bytes_per_input_byte")] = round(int(words[3 * n]) / size, 5)
    finally:
        L.qzstd_hip_free(0, d_rows)
    print(json.dumps(out))


def code_main(a):
    """--code: the grouped device call with the plane probe on and with the plane code on"""
    size = int(a.gib * (1 << 30)) & ~(a.chunk - 1)
    if a.kernels:
        return code_kernels(a, size)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    n = size // a.chunk
    torch.manual_seed(0)
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "data": {},
           "timed": "QZSTD_frontCompressDevice with byte grouping on, GB/s of input, every run of %d, the plane probe on and the plane code on alternating" % a.reps}

    def setting(fr, code):
        assert fr.set_plane_code(code) == 0 and fr.set_plane_probe(not code) == 0

    for kind, dt, k in (("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 4)):
        t = (torch.randn(size // k, device="cuda:0") * 0.02).to(dt)
        torch.cuda.synchronize()
        res = out["data"][kind] = {"elem": k, "levels": {}}
        for level in [int(x) for x in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            try:
                fr.reserve(size)
                stream = torch.cuda.current_stream().cuda_stream
                assert fr.set_byte_group(k) == 0
                cell = {"probe_gbps": [], "code_gbps": []}
                for code in (0, 1):  # untimed: first touch of the destination, the device slots, the pinned arenas
                    tag = "code" if code else "probe"
                    setting(fr, code)
                    s0, c0 = fr.stats(), fr.plane_code_stats()
                    r, sizes = fr.call_device(t.data_ptr(), size, stream)
                    assert r == n, tag
                    s1, c1 = fr.stats(), fr.plane_code_stats()
                    cell["compressed_" + tag] = sum(sizes[c] for c in range(n))
                    cell["d2h_bytes_per_input_byte_" + tag] = round((s1[2] - s0[2]) / size, 5)
                    if code:
                        cell["rows_coded_blocks_taken"] = [c1[0] - c0[0], c1[1] - c0[1]]
                        cell["frames_without_libzstd_share"] = round((c1[2] - c0[2]) / n, 4)
                        cell["frames_fell_back_share"] = round((c1[3] - c0[3]) / n, 4)
                for _ in range(a.reps):
                    for code in (0, 1):
                        setting(fr, code)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r, _ = fr.call_device(t.data_ptr(), size, stream)
                        dt_s = time.perf_counter() - t0
                        assert r == n
                        cell["code_gbps" if code else "probe_gbps"].append(round(size / dt_s / 1e9, 3))
                res["levels"][str(level)] = cell
            finally:
                fr.close()
        del t
        torch.cuda.empty_cache()
    print(json.dumps(out))


def fingerprint_kernels(a, size, out):
    """qzstd_hip_fingerprint beside qzstd_hip_diff and qzstd_hip_xxh64 IN ONE RUN: ONE launch each over the same N GiB as rows of 128 KiB, ms per
    GiB from events around the launch (rows uploaded inside), the three alternating, every run listed after one untimed round"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_fingerprint_kernel(D.bind_diff_kernel(plug.lib))
    L.qzstd_hip_xxh64.restype = C.c_int
    L.qzstd_hip_xxh64.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    n = size // a.chunk
    torch.manual_seed(0)
    src = (torch.randn(size // 2, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8)
    same = src.clone()
    tiles = torch.empty(size >> 14, dtype=torch.int64, device="cuda:0")
    flags = torch.empty(n, dtype=torch.int32, device="cuda:0")
    hashes = torch.empty(n, dtype=torch.int64, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.DiffRow))
    assert d_rows and src.data_ptr() % 16 == 0
    gib = size / float(1 << 30)
    fp_rows, diff_rows, hash_rows = (D.FpRow * n)(), (D.DiffRow * n)(), (D.HashRow * n)()
    for c in range(n):
        o = c * a.chunk
        fp_rows[c].src, fp_rows[c].len = src.data_ptr() + o, a.chunk
        diff_rows[c].a, diff_rows[c].b, diff_rows[c].len = src.data_ptr() + o, same.data_ptr() + o, a.chunk
        hash_rows[c].srcOff, hash_rows[c].len = o, a.chunk
    legs = (("fingerprint", lambda: L.qzstd_hip_fingerprint(0, None, fp_rows, n, d_rows, tiles.data_ptr())),
            ("diff", lambda: L.qzstd_hip_diff(0, None, diff_rows, n, d_rows, flags.data_ptr())),
            ("xxh64", lambda: L.qzstd_hip_xxh64(0, None, src.data_ptr(), hash_rows, n, d_rows, hashes.data_ptr())))
    # the same three over the FIRST 64 MiB only (512 rows): a part of the compress calls, the launch size the checksum kernel's 4.7 ms per GiB
    # was measured at (profiles/device_checksum_kernels.txt: 16 such launches a GiB)
    m = min(n, (64 << 20) // a.chunk)
    part = (("fingerprint", lambda: L.qzstd_hip_fingerprint(0, None, fp_rows, m, d_rows, tiles.data_ptr())),
            ("diff", lambda: L.qzstd_hip_diff(0, None, diff_rows, m, d_rows, flags.data_ptr())),
            ("xxh64", lambda: L.qzstd_hip_xxh64(0, None, src.data_ptr(), hash_rows, m, d_rows, hashes.data_ptr())))
    runs = {name: [] for name, _ in legs}
    part_runs = {name: [] for name, _ in part}
    try:
        for which, into, scale in ((legs, runs, gib), (part, part_runs, 1.0)):
            for i in range(a.reps + 1):
                for name, call in which:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    assert call() == 0, plug.err()
                    e1.record()
                    torch.cuda.synchronize()
                    if i:
                        into[name].append(round(e0.elapsed_time(e1) / scale, 3))
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert not bool(flags.any())
    # the digests are worth something: the first and the last row against the plain-C function
    host = src[:a.chunk].cpu().numpy().tobytes(), src[size - a.chunk:].cpu().numpy().tobytes()
    per = a.chunk >> 14
    lib = B.Front().lib
    for row, data in ((0, host[0]), (n - 1, host[1])):
        got = D.fp_fold_ref([v & 0xFFFFFFFFFFFFFFFF for v in tiles[row * per:(row + 1) * per].tolist()], a.chunk)
        assert got == D.fingerprint_of(data, lib=lib), row
    out["kernels"] = {"rows": n, "row_bytes": a.chunk, "fingerprint_ms_per_gib": runs["fingerprint"], "diff_ms_per_gib": runs["diff"],
                      "xxh64_ms_per_gib": runs["xxh64"],
                      "part_rows": m, "part_fingerprint_ms_per_launch": part_runs["fingerprint"], "part_diff_ms_per_launch": part_runs["diff"],
                      "part_xxh64_ms_per_launch": part_runs["xxh64"],
                      "part": "the same three launches over the first %d rows only (%d MiB: one part of a compress call), ms per LAUNCH" % (m, m * a.chunk >> 20),
                      "timed": "events around ONE launch each (rows uploaded inside) over the same %d rows of %d bytes, ms per GiB of rows, the three "
                               "alternating in one run, every run of %d after one untimed round; diff reads two sides (2 bytes per content byte)" % (n, a.chunk, a.reps)}


def fingerprint_main(a):
    """--fingerprint: QZSTD_frontFingerprintDeviceBatch against what a caller can do today — t.cpu() and a host hash of the chunks on --threads
    threads — and beside QZSTD_frontVerifyDeviceBatch, the only existing end-to-end check, on N GiB of bf16 as one tensor and as tensors of
    128 KiB; then the kernel beside qzstd_hip_diff and qzstd_hip_xxh64 in the same run.  --kernels: the kernel legs alone"""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    import xxhash
    size = int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1)
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "reps": a.reps, "dtype": "bf16"}
    if a.kernels:
        fingerprint_kernels(a, size, out)
        return print(json.dumps(out))
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    n = size // a.chunk
    out["timed"] = ("ms per call, every run, the legs alternating in one run; the window holds the call and the closing synchronize: fingerprint = "
                    "QZSTD_frontFingerprintDeviceBatch; host_hash = t.cpu() per tensor and xxhash.xxh64 of every %d-byte chunk on %d threads (the "
                    "module releases the GIL); verify = QZSTD_frontVerifyDeviceBatch of level-1 grouped frames of the same tensors against "
                    "them (it needs the LIVE tensors: no load-time check)" % (a.chunk, a.threads))
    out["cells"] = {}
    whole = (torch.randn(size // 2, device="cuda:0") * 0.02).to(torch.bfloat16)
    pool = ThreadPoolExecutor(a.threads)
    for layout, nt in (("one_tensor", 1), ("%d_tensors" % n, n)):
        per = size // nt
        tensors = [whole[i * (per // 2):(i + 1) * (per // 2)] for i in range(nt)]
        fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
        cell = out["cells"][layout] = {}
        try:
            fr.reserve(size)
            bufs, _, frames_n = fr.batch([(x.data_ptr(), per) for x in tensors])
            assert frames_n == n
            fp = (C.c_ulonglong * n)()
            es = bytes([2] * nt) + b"\0"
            _, sizes = fr._frame_buffers(n)
            assert fr.lib.QZSTD_frontCompressDeviceBatchTyped(fr.f, bufs, es, nt, stream, fr._dst, len(fr._dst), sizes, None) == n
            frames = C.create_string_buffer(n * fr.stride)
            C.memmove(frames, fr._dst, n * fr.stride)

            def fingerprint():
                return fr.lib.QZSTD_frontFingerprintDeviceBatch(fr.f, bufs, nt, stream, fp, None)

            def host_hash():
                def one(t):
                    h = t.cpu().view(torch.uint8).numpy()
                    return [xxhash.xxh64(h[o:o + a.chunk]).intdigest() for o in range(0, len(h), a.chunk)]
                if nt == 1:  # one tensor: one copy, its chunks hashed on the threads
                    h = tensors[0].cpu().view(torch.uint8).numpy()
                    return len(list(pool.map(lambda o: xxhash.xxh64(h[o:o + a.chunk]).intdigest(), range(0, size, a.chunk))))
                return sum(len(x) for x in pool.map(one, tensors))

            def verify():
                r = fr.lib.QZSTD_frontVerifyDeviceBatch(fr.f, frames, fr.stride, sizes, n, bufs, None, es, nt, stream, None)
                return n if r == 0 else r

            legs = (("fingerprint", fingerprint), ("host_hash", host_hash), ("verify", verify))
            runs = {name + "_ms": [] for name, _ in legs}
            for name, leg in legs:  # untimed: the slots, the pinned scratch
                assert leg() == n, name
                torch.cuda.synchronize()
            for _ in range(a.reps):
                for name, leg in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert leg() == n, name
                    torch.cuda.synchronize()
                    runs[name + "_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            cell.update(runs)
            # the answer is worth something: the plain-C function over the first and the last chunk, and one bit found at its place
            host = whole.view(torch.uint8)
            assert fp[0] == D.fingerprint_of(host[:a.chunk].cpu().numpy().tobytes(), lib=lib)
            assert fp[n - 1] == D.fingerprint_of(host[size - a.chunk:].cpu().numpy().tobytes(), lib=lib)
            flags = C.create_string_buffer(n)
            host[3 * a.chunk + 16385] ^= 1
            torch.cuda.synchronize()
            assert fr.lib.QZSTD_frontCheckDeviceBatch(fr.f, bufs, nt, stream, fp, n, flags) == 1 and flags.raw == bytes(3) + b"\x01" + bytes(n - 4)
            host[3 * a.chunk + 16385] ^= 1
            torch.cuda.synchronize()
            cell["d2h_bytes"] = 8 * (size >> 14)
            cell["h2d_bytes"] = 16 * n
            cell["fingerprint_stats"] = fr.fingerprint_stats()
        finally:
            fr.close()
        del tensors
    pool.shutdown()
    del whole
    torch.cuda.empty_cache()
    fingerprint_kernels(a, size, out)
    print(json.dumps(out))


def ediff_kernels(a, size, out):
    """qzstd_hip_group_ediff beside qzstd_hip_group and qzstd_hip_esum beside qzstd_hip_ungroup IN ONE RUN: ONE launch each over the same N GiB
    as rows of 128 KiB, k = 4 and 8, ms per GiB from events around the launch (rows uploaded inside), alternating, every run listed after one
    untimed round.  Traffic: the two gathers move 2 bytes per content byte; the summing launch reads the destination twice and writes it once"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_ediff_kernels(plug.lib)
    L.qzstd_hip_group.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    L.qzstd_hip_ungroup.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    n = size // a.chunk
    gib = size / float(1 << 30)
    torch.manual_seed(0)
    src = torch.cumsum(torch.randint(5, 41, (size // 8,), device="cuda:0", dtype=torch.int64), 0).view(torch.uint8)
    stage = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    tiles = size >> 14
    scratch = torch.empty(D.esum_scratch_bytes(tiles), dtype=torch.uint8, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.GroupEdiffRow))
    assert d_rows and src.data_ptr() % 16 == 0 and stage.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0
    cells = {}
    try:
        for k in (4, 8):
            g_rows, e_rows, u_rows, s_rows = (D.GroupRow * n)(), (D.GroupEdiffRow * n)(), (D.UngroupRow * n)(), (D.EsumRow * n)()
            for c in range(n):
                o = c * a.chunk
                for r in (g_rows[c], e_rows[c]):
                    r.src, r.dstOff, r.len, r.pad, r.elem = src.data_ptr() + o, o, a.chunk, 16 if c + 1 == n else 0, k
                e_rows[c].flags = D.EDIFF_DIFF
                u_rows[c].dst, u_rows[c].srcOff, u_rows[c].len, u_rows[c].elem = dst.data_ptr() + o, o, a.chunk, k
                s_rows[c].dst, s_rows[c].len, s_rows[c].elem = dst.data_ptr() + o, a.chunk, k
            legs = (("group", lambda: L.qzstd_hip_group(0, None, g_rows, n, d_rows, stage.data_ptr(), size + 16)),
                    ("group_ediff", lambda: L.qzstd_hip_group_ediff(0, None, e_rows, n, d_rows, stage.data_ptr(), size + 16)),
                    ("ungroup", lambda: L.qzstd_hip_ungroup(0, None, u_rows, n, d_rows, stage.data_ptr(), size + 16)),
                    ("esum", lambda: L.qzstd_hip_esum(0, None, s_rows, n, d_rows, scratch.data_ptr(), scratch.numel())))
            runs = {name: [] for name, _ in legs}
            for i in range(a.reps + 1):
                for name, call in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    assert call() == 0, plug.err()
                    e1.record()
                    torch.cuda.synchronize()
                    if i:
                        runs[name].append(round(e0.elapsed_time(e1) / gib, 3))
            # the last round's order was group_ediff -> ungroup -> esum: the destination holds the source again
            assert torch.equal(dst.view(torch.int64)[:1 << 16], src.view(torch.int64)[:1 << 16]) and torch.equal(dst[-(1 << 16):], src[-(1 << 16):]), k
            cells["k%d" % k] = {name + "_ms_per_gib": v for name, v in runs.items()}
    finally:
        L.qzstd_hip_free(0, d_rows)
    out["kernels"] = {"rows": n, "row_bytes": a.chunk, "cells": cells,
                      "timed": "events around ONE launcher call each (rows uploaded inside; esum is three kernels) over the same %d rows of %d bytes, ms per "
                               "GiB of rows, alternating in one run, every run of %d after one untimed round" % (n, a.chunk, a.reps)}


def ediff_main(a):
    """--ediff: N GiB of int64 timestamps and of int32 offsets as ONE tensor each, 128 KiB frames: the Typed calls with QZSTD_ELEM_DIFF off and on,
    and what a caller does today — a torch.diff-style pre-pass into a temporary, then the Typed call; the Typed restore, then cumsum — the legs
    alternating in one run; then the two kernels beside qzstd_hip_group and qzstd_hip_ungroup.  --kernels: the kernel legs alone"""
    size = int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1)
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "reps": a.reps}
    if a.kernels:
        ediff_kernels(a, size, out)
        return print(json.dumps(out))
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    stream = torch.cuda.current_stream().cuda_stream
    n = size // a.chunk
    out["timed"] = ("GB/s of input, every run, the legs alternating in one run; the window holds the library call, the torch passes of the leg and the "
                    "closing synchronize.  off / on: QZSTD_frontCompressDeviceBatchTyped and QZSTD_frontRestoreDeviceBatchTyped without and with "
                    "QZSTD_ELEM_DIFF; torch: d[0] = x[0], d[1:] = x[1:] - x[:-1] into a fresh temporary (over the whole tensor, no zigzag), the Typed "
                    "call on it, and on the way back the Typed restore followed by cumsum into the destination")
    out["cells"] = {}
    torch.manual_seed(1)
    inputs = (("timestamps_int64", torch.int64, 8,
               lambda m: 1_700_000_000_000_000 + torch.cumsum(torch.empty(m, device="cuda:0").exponential_(1e-3).to(torch.int64) + 1, 0)),
              ("offsets_int32", torch.int32, 4, lambda m: torch.cumsum(torch.randint(5, 41, (m,), device="cuda:0", dtype=torch.int64), 0).to(torch.int32)))
    for name, dtype, k, make in inputs:
        x = make(size // k)
        back = torch.empty_like(x)
        for level in [int(v) for v in a.levels.split(",")]:
            fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
            cell = out["cells"]["%s_level%d" % (name, level)] = {}
            try:
                fr.reserve(size)

                import ctypes as C
                _, sizes = fr._frame_buffers(n)
                outb = fr.out_batch([(back.data_ptr(), size)])
                kept = {}

                def compress(t, flag):
                    bufs, _, frames_n = fr.batch([(t.data_ptr(), size)])
                    assert frames_n == n
                    return fr.lib.QZSTD_frontCompressDeviceBatchTyped(fr.f, bufs, bytes([k | flag, 0]), 1, stream, fr._dst, len(fr._dst), sizes, None)

                def pre(t):
                    d = torch.empty_like(t)
                    d[0] = t[0]
                    torch.sub(t[1:], t[:-1], out=d[1:])
                    return d

                def c_off():
                    return compress(x, 0)

                def c_on():
                    return compress(x, D.ELEM_DIFF)

                def c_torch():
                    return compress(pre(x), 0)

                for leg, f in (("off", c_off), ("on", c_on), ("torch", c_torch)):  # untimed: the slots, the pinned scratch; the frames are kept
                    assert f() == n, leg
                    torch.cuda.synchronize()
                    buf = C.create_string_buffer(n * fr.stride)
                    C.memmove(buf, fr._dst, n * fr.stride)
                    kept[leg] = (buf, (C.c_size_t * n)(*sizes[:n]))
                    cell["compressed_" + leg] = sum(sizes[:n])

                def restore(leg, to, flag):
                    buf, sz = kept[leg]
                    return fr.lib.QZSTD_frontRestoreDeviceBatchTyped(fr.f, buf, fr.stride, sz, n, to, bytes([k | flag, 0]), 1, stream)

                def r_off():
                    return restore("off", outb, 0)

                def r_on():
                    return restore("on", outb, D.ELEM_DIFF)

                def r_torch():
                    tmp = torch.empty_like(x)
                    r = restore("torch", fr.out_batch([(tmp.data_ptr(), size)]), 0)
                    torch.cumsum(tmp, 0, dtype=dtype, out=back)
                    return r

                runs = {}
                for leg, f in (("restore_off", r_off), ("restore_on", r_on), ("restore_torch", r_torch)):
                    back.zero_()
                    assert f() == n, leg
                    torch.cuda.synchronize()
                    assert torch.equal(back, x), leg
                legs = (("compress_off", c_off), ("compress_on", c_on), ("compress_torch", c_torch), ("restore_off", r_off), ("restore_on", r_on),
                        ("restore_torch", r_torch))
                for _ in range(a.reps):
                    for leg, f in legs:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert f() == n, leg
                        torch.cuda.synchronize()
                        runs.setdefault(leg + "_gbps", []).append(round(size / (time.perf_counter() - t0) / 1e9, 2))
                cell.update(runs)
                cell["elem_diff_stats"] = fr.elem_diff_stats()
            finally:
                fr.close()
        del x, back
        torch.cuda.empty_cache()
    ediff_kernels(a, size, out)
    print(json.dumps(out))


def advise_kernels(a, size, out):
    """qzstd_hip_ediff_cost beside qzstd_hip_fingerprint and qzstd_hip_plane_cost IN ONE RUN: ONE launch each over the same N GiB as rows of
    128 KiB, ms per GiB from events around the launch (rows uploaded inside), alternating, every run listed after one untimed round; the
    cost kernel for k = 1, 2, 4, 8, on noise and on a zero-plane-heavy input (an int64 column of steps 5 .. 40: differenced, seven of its
    eight planes are zero).  The other two do not depend on k.  Traffic: all three read 1 byte per content byte; the cost kernel does two LDS
    histogram updates per byte where the plane-cost kernel does one"""
    import ctypes as C
    plug = B.Plugin()
    L = D.bind_ediff_cost_kernel(D.bind_fingerprint_kernel(D.bind_plane_kernel(plug.lib)))
    n = size // a.chunk
    gib = size / float(1 << 30)
    torch.manual_seed(0)
    inputs = (("noise", torch.randint(0, 256, (size,), device="cuda:0", dtype=torch.uint8)),
              ("zero_planes", torch.cumsum(torch.randint(5, 41, (size // 8,), device="cuda:0", dtype=torch.int64), 0).view(torch.uint8)))
    tiles = torch.empty(2 * (size >> 14), dtype=torch.int32, device="cuda:0")
    fp_tiles = torch.empty(size >> 14, dtype=torch.int64, device="cuda:0")
    cost = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, n * C.sizeof(D.EdiffCostRow))
    assert d_rows
    cells = {}
    lib = D.bind(B.Front().lib)
    try:
        for name, src in inputs:
            assert src.data_ptr() % 16 == 0
            fp_rows, pl_rows = (D.FpRow * n)(), (D.PlaneRow * n)()
            ec_rows = {k: (D.EdiffCostRow * n)() for k in (1, 2, 4, 8)}
            for c in range(n):
                o = c * a.chunk
                fp_rows[c].src, fp_rows[c].len = src.data_ptr() + o, a.chunk
                pl_rows[c].srcOff, pl_rows[c].len = o, a.chunk
                for k, rows in ec_rows.items():
                    rows[c].src, rows[c].len, rows[c].elem = src.data_ptr() + o, a.chunk, k
            legs = [("ediff_cost_k%d" % k, (lambda rows: lambda: L.qzstd_hip_ediff_cost(0, None, rows, n, d_rows, tiles.data_ptr()))(rows))
                    for k, rows in ec_rows.items()]
            legs += [("fingerprint", lambda: L.qzstd_hip_fingerprint(0, None, fp_rows, n, d_rows, fp_tiles.data_ptr())),
                     ("plane_cost", lambda: L.qzstd_hip_plane_cost(0, None, src.data_ptr(), pl_rows, n, d_rows, cost.data_ptr()))]
            runs = {leg: [] for leg, _ in legs}
            for i in range(a.reps + 1):
                for leg, call in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    assert call() == 0, plug.err()
                    e1.record()
                    torch.cuda.synchronize()
                    if i:
                        runs[leg].append(round(e0.elapsed_time(e1) / gib, 3))
            # the words are worth something: the last launch (k = 8) over the first and the last row against the plain-C function
            per = a.chunk >> 14
            for row in (0, n - 1):
                w = tiles[2 * row * per:2 * (row + 1) * per].cpu().numpy().astype("uint32").reshape(-1, 2).sum(axis=0)
                assert (int(w[0]), int(w[1])) == D.ediff_cost_of(src[row * a.chunk:(row + 1) * a.chunk].cpu().numpy().tobytes(), 8, lib=lib), (name, row)
            cells[name] = {leg + "_ms_per_gib": v for leg, v in runs.items()}
    finally:
        L.qzstd_hip_free(0, d_rows)
    out["kernels"] = {"rows": n, "row_bytes": a.chunk, "cells": cells,
                      "timed": "events around ONE launcher call each (rows uploaded inside) over the same %d rows of %d bytes, ms per GiB of rows, "
                               "alternating in one run, every run of %d after one untimed round" % (n, a.chunk, a.reps)}


def advise_main(a):
    """--advise: QZSTD_frontAdviseDeviceBatch against what a caller does today to decide on QZSTD_ELEM_DIFF — the Typed compress call twice,
    flag off and on, and the sizes compared — on N GiB of int32 offsets as one tensor and as tensors of 128 KiB, level 1, the legs alternating
    in one run; then the kernel beside qzstd_hip_fingerprint and qzstd_hip_plane_cost.  --kernels: the kernel legs alone"""
    import ctypes as C
    size = int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1)
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "reps": a.reps, "dtype": "int32 offsets, steps 5 .. 40", "level": 1}
    if a.kernels:
        advise_kernels(a, size, out)
        return print(json.dumps(out))
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    n = size // a.chunk
    out["timed"] = ("ms per decision, every run, the legs alternating in one run; the window holds the calls and the closing synchronize: advise = ONE "
                    "QZSTD_frontAdviseDeviceBatch; twice = QZSTD_frontCompressDeviceBatchTyped at level 1 without and then with QZSTD_ELEM_DIFF "
                    "on every tensor, and the per-tensor sizes compared on the host")
    out["cells"] = {}
    whole = torch.cumsum(torch.randint(5, 41, (size // 4,), device="cuda:0", dtype=torch.int64), 0).to(torch.int32)
    for layout, nt in (("one_tensor", 1), ("%d_tensors" % n, n)):
        per = size // nt
        tensors = [whole[i * (per // 4):(i + 1) * (per // 4)] for i in range(nt)]
        fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
        cell = out["cells"][layout] = {}
        try:
            fr.reserve(size)
            bufs, _, frames_n = fr.batch([(x.data_ptr(), per) for x in tensors])
            assert frames_n == n
            _, sizes = fr._frame_buffers(n)
            first = (C.c_size_t * (nt + 1))()
            es = bytes([4] * nt) + b"\0"
            es_on = bytes([4 | D.ELEM_DIFF] * nt) + b"\0"
            adv = C.create_string_buffer(nt)
            est = (C.c_ulonglong * (2 * nt))()

            def advise():
                return fr.lib.QZSTD_frontAdviseDeviceBatch(fr.f, bufs, es, nt, stream, adv, est)

            def twice():
                per_tensor = []
                for e in (es, es_on):
                    assert fr.lib.QZSTD_frontCompressDeviceBatchTyped(fr.f, bufs, e, nt, stream, fr._dst, len(fr._dst), sizes, first) == n
                    s = sizes[:n]
                    per_tensor.append([sum(s[first[i]:first[i + 1]]) for i in range(nt)])
                return sum(1 for off, on in zip(*per_tensor) if on < off)

            legs = (("advise", advise), ("twice", twice))
            runs = {name + "_ms": [] for name, _ in legs}
            for name, leg in legs:  # untimed: the slots, the pinned scratch
                cell[name + "_flagged"] = leg()
                torch.cuda.synchronize()
            for _ in range(a.reps):
                for name, leg in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert leg() == cell[name + "_flagged"], name
                    torch.cuda.synchronize()
                    runs[name + "_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            cell.update(runs)
            # the estimate is worth something: the plain-C function over the first chunk-sized tensor, and both layouts sum to the same words
            cell["est_sum"] = [sum(est[0::2]), sum(est[1::2])]
            if nt > 1:
                host = tensors[0].view(torch.uint8).cpu().numpy().tobytes()
                assert (est[0], est[1]) == D.ediff_cost(host, 4, a.chunk, lib=fr.lib)
                assert per != a.chunk or cell["est_sum"] == out["cells"]["one_tensor"]["est_sum"]
            cell["d2h_bytes"] = 8 * (size >> 14)
            cell["h2d_bytes"] = 24 * n
            cell["advise_stats"] = fr.advise_stats()
        finally:
            fr.close()
        del tensors
    del whole
    torch.cuda.empty_cache()
    advise_kernels(a, size, out)
    print(json.dumps(out))


def srcslices_kernels(a, size, out):
    """qzstd_hip_group_pieces beside qzstd_hip_group_xor IN ONE RUN: ONE launch each over the same N GiB as rows of 128 KiB, without a base, ms
    per GiB from events around the launcher call (rows and pieces uploaded inside, from pinned memory), alternating, every run listed after
    one untimed round; pieces of a whole frame, 8 KiB, 2 KiB and 64 bytes — cut out of the same contiguous source, so the bytes read are the
    same and only the table differs — for k = 1, 2, 4, 8; the stage of every pieces launch is compared with the group_xor launch's"""
    import ctypes as C
    import numpy as np
    plug = B.Plugin()
    L = D.bind_pieces_kernel(D.bind_xor_kernels(plug.lib))
    n = size // a.chunk
    gib = size / float(1 << 30)
    torch.manual_seed(0)
    src = torch.randint(0, 256, (size,), device="cuda:0", dtype=torch.uint8)
    stage = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    stage2 = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    assert src.data_ptr() % 16 == 0 and stage.data_ptr() % 16 == 0 and stage2.data_ptr() % 16 == 0
    piece_t = np.dtype([("src", "<u8"), ("base", "<u8"), ("off", "<u4"), ("len", "<u4")])
    row_t = np.dtype([("dstOff", "<u8"), ("len", "<u4"), ("pad", "<u4"), ("elem", "<u4"), ("piece0", "<u4"), ("nPieces", "<u4"), ("reserved", "<u4")])
    widths = (("frame", a.chunk), ("8k", 8192), ("2k", 2048), ("64", 64))
    most = size // 64
    pin_p = torch.empty(most * piece_t.itemsize, dtype=torch.uint8).pin_memory()
    pin_r = torch.empty(n * row_t.itemsize, dtype=torch.uint8).pin_memory()
    d_pieces = L.qzstd_hip_malloc(0, most * piece_t.itemsize)
    d_rows = L.qzstd_hip_malloc(0, n * max(row_t.itemsize, C.sizeof(D.GroupXorRow)))
    assert d_pieces and d_rows
    cells = {}
    try:
        for k in (1, 2, 4, 8):
            xrows = (D.GroupXorRow * n)()
            for c in range(n):
                x = xrows[c]
                x.src, x.base, x.dstOff, x.len, x.pad, x.elem = src.data_ptr() + c * a.chunk, 0, c * a.chunk, a.chunk, 16 if c + 1 == n else 0, k
            rows = pin_r.numpy().view(row_t)
            cell = cells["k%d" % k] = {}

            def timed(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                assert call() == 0, plug.err()
                e1.record()
                torch.cuda.synchronize()
                return round(e0.elapsed_time(e1) / gib, 3)

            runs = {"group_xor": []}
            for i in range(a.reps + 1):
                t = timed(lambda: L.qzstd_hip_group_xor(0, None, xrows, n, d_rows, stage.data_ptr(), size + 16))
                if i:
                    runs["group_xor"].append(t)
            for name, w in widths:
                per = a.chunk // w
                np_ = n * per
                pieces = pin_p.numpy()[:np_ * piece_t.itemsize].view(piece_t)
                pieces["src"] = np.uint64(src.data_ptr()) + np.arange(np_, dtype=np.uint64) * np.uint64(w)
                pieces["base"] = 0
                pieces["off"] = (np.arange(np_, dtype=np.uint64) % np.uint64(per)) * np.uint64(w)
                pieces["len"] = w
                rows["dstOff"] = np.arange(n, dtype=np.uint64) * np.uint64(a.chunk)
                rows["len"], rows["pad"], rows["elem"], rows["nPieces"], rows["reserved"] = a.chunk, 0, k, per, 0
                rows["pad"][n - 1] = 16
                rows["piece0"] = np.arange(n, dtype=np.uint64) * np.uint64(per)
                key = "pieces_" + name
                runs[key], runs[key + "_table_upload"] = [], []
                dev_copy = torch.empty(np_ * piece_t.itemsize, dtype=torch.uint8, device="cuda:0")
                for i in range(a.reps + 1):
                    t = timed(lambda: L.qzstd_hip_group_pieces(0, None, rows.ctypes.data, n, d_rows, pieces.ctypes.data, np_, d_pieces, stage2.data_ptr(),
                                                               size + 16))
                    u = timed(lambda: (dev_copy.copy_(pin_p[:np_ * piece_t.itemsize], non_blocking=True), 0)[1])
                    if i:
                        runs[key].append(t)
                        runs[key + "_table_upload"].append(u)
                assert torch.equal(stage, stage2), (k, name)
                stage2.zero_()
                del dev_copy
            cell.update({leg + "_ms_per_gib": v for leg, v in runs.items()})
    finally:
        L.qzstd_hip_free(0, d_rows)
        L.qzstd_hip_free(0, d_pieces)
    out["kernels"] = {"rows": n, "row_bytes": a.chunk, "cells": cells, "piece_table_bytes": {name: size // w * 24 for name, w in widths},
                      "timed": "events around ONE launcher call each (rows and pieces uploaded inside, from pinned memory) over the same %d rows of %d "
                               "bytes of random bytes, no base, ms per GiB of rows, every run of %d after one untimed round; *_table_upload: the same "
                               "events around a copy of the piece table alone" % (n, a.chunk, a.reps)}


def srcslices_main(a):
    """--srcslices: QZSTD_frontCompressDeviceSlices on a column view against view.contiguous() + the Typed / Delta call and against that call on a
    contiguous tensor; then the kernel beside qzstd_hip_group_xor.  --kernels: the kernel legs alone"""
    import ctypes as C
    rows_n = (int(a.gib * 65536) + 15) & ~15
    rowb, width = 16384, 8192
    size = rows_n * width
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "reps": a.reps, "dtype": "bf16 N(0, 0.02)", "matrix_bytes": [rows_n, rowb],
           "slices": rows_n, "slice_bytes": width}
    if a.kernels:
        srcslices_kernels(a, int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1), out)
        return print(json.dumps(out))
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    n = size // a.chunk
    out["timed"] = ("GB/s of input, every run, the legs alternating in one run; the window holds the calls (the slice and buffer arrays exist before "
                    "it), for `contiguous` the .contiguous() copies, and the closing synchronize")
    out["peak_extra_device_bytes"] = ("torch's peak allocation above the level before the call (the .contiguous() temporaries); the library's own "
                                      "stages are the same in all legs and not included")
    mat = (torch.randn(rows_n * rowb // 2, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8).view(rows_n, rowb)
    bmat = ((mat.view(torch.bfloat16).float() + torch.randn(rows_n, rowb // 2, device="cuda:0") * 1e-5).to(torch.bfloat16)).view(torch.uint8).view(rows_n, rowb)
    mat, bmat = bmat, mat  # (the new checkpoint is the update; the base is what it came from)
    view, bview = mat[:, :width], bmat[:, :width]
    flat, bflat = view.contiguous(), bview.contiguous()
    out["cells"] = {}
    for level in [int(x) for x in a.levels.split(",")]:
        fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
        try:
            fr.reserve(size)
            _, sizes = fr._frame_buffers(n)
            first = (C.c_size_t * 2)()
            es = bytes([2]) + b"\0"
            bs = (C.c_size_t * 1)(size)
            for based in (False, True):
                sl = [(0, r * width, width, view.data_ptr() + r * rowb, bview.data_ptr() + r * rowb if based else None) for r in range(rows_n)]
                arr = fr.src_slice_array(sl)
                fbufs, fbase = fr.batch([(flat.data_ptr(), size)])[0], fr.batch([(bflat.data_ptr(), size)])[0]

                def leg_slices():
                    return fr.call_compress_slices(bs, 1, es, arr, rows_n, sizes, first, stream)

                def delta(t, b):
                    return fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, fr.batch([(t.data_ptr(), size)])[0],
                                                                      fr.batch([(b.data_ptr(), size)])[0] if based else None, es, 1, stream,
                                                                      fr._dst, len(fr._dst), sizes, first)

                def leg_contiguous():
                    return delta(view.contiguous(), bview.contiguous() if based else None)

                def leg_typed():
                    return fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, fbufs, fbase if based else None, es, 1, stream, fr._dst, len(fr._dst), sizes, first)

                legs = (("slices", leg_slices), ("contiguous", leg_contiguous), ("typed", leg_typed))
                cell = out["cells"]["level%d_%s" % (level, "base" if based else "nobase")] = {}
                frames = {}
                for name, leg in legs:  # untimed, and checked
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    m0, s0, p0 = torch.cuda.memory_allocated(), fr.stats(), fr.src_slice_stats()
                    assert leg() == n, name
                    torch.cuda.synchronize()
                    peak, s1 = torch.cuda.max_memory_allocated() - m0, fr.stats()
                    frames[name] = fr.frames(n, sizes)
                    cell[name] = {"compressed_bytes": sum(len(x) for x in frames[name]), "peak_extra_device_bytes": peak,
                                  "d2h_bytes_per_input_byte": round((s1[2] - s0[2]) / size, 4), "gbps": []}
                    if name == "slices":
                        cell[name]["src_slice_stats"] = [y - x for x, y in zip(p0, fr.src_slice_stats())]
                assert frames["slices"] == frames["contiguous"] == frames["typed"], (level, based)
                del frames
                for _ in range(a.reps):
                    for name, leg in legs:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert leg() == n, name
                        torch.cuda.synchronize()
                        cell[name]["gbps"].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
        finally:
            fr.close()
    del mat, bmat, view, bview, flat, bflat
    torch.cuda.empty_cache()
    srcslices_kernels(a, int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1), out)
    print(json.dumps(out))


def slicecheck_kernels(a, size, out):
    """qzstd_hip_fingerprint_pieces beside qzstd_hip_fingerprint and qzstd_hip_ungroup_cmp_pieces beside qzstd_hip_ungroup_cmp IN ONE RUN: ONE
    launch each over the same N GiB as rows of 128 KiB, ms per GiB from events around the launcher call (rows and pieces uploaded inside, from
    pinned memory), alternating, every run listed after one untimed round; pieces of a whole frame, 8 KiB, 2 KiB and 64 bytes — cut out of the
    same contiguous source, so the bytes read are the same and only the table differs; the comparison for k = 2 and 4 without a base, its
    stage the grouped source (every word says SAME); the tile words of every pieces launch are compared with the contiguous launch's"""
    import ctypes as C
    import numpy as np
    plug = B.Plugin()
    L = D.bind_check_pieces_kernels(D.bind_cmp_kernel(D.bind_fingerprint_kernel(D.bind_xor_kernels(plug.lib))))
    n = size // a.chunk
    gib = size / float(1 << 30)
    torch.manual_seed(0)
    src = torch.randint(0, 256, (size,), device="cuda:0", dtype=torch.uint8)
    stage = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
    assert src.data_ptr() % 16 == 0 and stage.data_ptr() % 16 == 0
    piece_t = np.dtype([("src", "<u8"), ("base", "<u8"), ("off", "<u4"), ("len", "<u4")])
    fprow_t = np.dtype([("len", "<u4"), ("tile0", "<u4"), ("piece0", "<u4"), ("nPieces", "<u4")])
    cmprow_t = np.dtype([("srcOff", "<u8"), ("len", "<u4"), ("elem", "<u4"), ("flags", "<u4"), ("tile0", "<u4"), ("piece0", "<u4"), ("nPieces", "<u4")])
    widths = (("frame", a.chunk), ("8k", 8192), ("2k", 2048), ("64", 64))
    most = size // 64
    tiles_n = n * (a.chunk // 16384)
    pin_p = torch.empty(most * piece_t.itemsize, dtype=torch.uint8).pin_memory()
    pin_r = torch.empty(n * cmprow_t.itemsize, dtype=torch.uint8).pin_memory()
    d_pieces = L.qzstd_hip_malloc(0, most * piece_t.itemsize)
    d_rows = L.qzstd_hip_malloc(0, n * max(cmprow_t.itemsize, C.sizeof(D.GroupXorRow), C.sizeof(D.UngroupCmpRow)))
    assert d_pieces and d_rows and a.chunk % 16384 == 0
    fp_a, fp_b = torch.zeros(tiles_n, dtype=torch.int64, device="cuda:0"), torch.zeros(tiles_n, dtype=torch.int64, device="cuda:0")
    cw_a, cw_b = torch.zeros(tiles_n, dtype=torch.int32, device="cuda:0"), torch.zeros(tiles_n, dtype=torch.int32, device="cuda:0")

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert call() == 0, plug.err()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / gib, 3)

    def table(w):
        per = a.chunk // w
        np_ = n * per
        pieces = pin_p.numpy()[:np_ * piece_t.itemsize].view(piece_t)
        pieces["src"] = np.uint64(src.data_ptr()) + np.arange(np_, dtype=np.uint64) * np.uint64(w)
        pieces["base"] = 0
        pieces["off"] = (np.arange(np_, dtype=np.uint64) % np.uint64(per)) * np.uint64(w)
        pieces["len"] = w
        return pieces, np_, per

    cells = {}
    try:
        # the fingerprint pair
        crows = (D.FpRow * n)()
        for c in range(n):
            crows[c].src, crows[c].len, crows[c].tile0 = src.data_ptr() + c * a.chunk, a.chunk, 0
        runs = {"fingerprint": []}
        rows = pin_r.numpy()[:n * fprow_t.itemsize].view(fprow_t)
        for name, w in widths:
            pieces, np_, per = table(w)
            rows["len"], rows["tile0"], rows["nPieces"] = a.chunk, 0, per
            rows["piece0"] = np.arange(n, dtype=np.uint64) * np.uint64(per)
            key = "pieces_" + name
            runs[key] = []
            for i in range(a.reps + 1):
                t0 = timed(lambda: L.qzstd_hip_fingerprint(0, None, crows, n, d_rows, fp_a.data_ptr()))
                t1 = timed(lambda: L.qzstd_hip_fingerprint_pieces(0, None, rows.ctypes.data, n, d_rows, pieces.ctypes.data, np_, d_pieces, fp_b.data_ptr()))
                if i:
                    runs["fingerprint"].append(t0)
                    runs[key].append(t1)
            assert torch.equal(fp_a, fp_b), name
            fp_b.zero_()
        cells["fingerprint"] = {leg + "_ms_per_gib": v for leg, v in runs.items()}
        # the comparison pair
        for k in (2, 4):
            xrows = (D.GroupXorRow * n)()
            for c in range(n):
                x = xrows[c]
                x.src, x.base, x.dstOff, x.len, x.pad, x.elem = src.data_ptr() + c * a.chunk, 0, c * a.chunk, a.chunk, 16 if c + 1 == n else 0, k
            assert L.qzstd_hip_group_xor(0, None, xrows, n, d_rows, stage.data_ptr(), size + 16) == 0, plug.err()
            torch.cuda.synchronize()
            vrows = (D.UngroupCmpRow * n)()
            for c in range(n):
                v = vrows[c]
                v.ref, v.base, v.srcOff, v.len, v.elem, v.flags, v.tile0 = src.data_ptr() + c * a.chunk, 0, c * a.chunk, a.chunk, k, 0, 0
            runs = {"ungroup_cmp": []}
            rows = pin_r.numpy().view(cmprow_t)
            for name, w in widths:
                pieces, np_, per = table(w)
                rows["srcOff"] = np.arange(n, dtype=np.uint64) * np.uint64(a.chunk)
                rows["len"], rows["elem"], rows["flags"], rows["tile0"], rows["nPieces"] = a.chunk, k, 0, 0, per
                rows["piece0"] = np.arange(n, dtype=np.uint64) * np.uint64(per)
                key = "pieces_" + name
                runs[key] = []
                for i in range(a.reps + 1):
                    t0 = timed(lambda: L.qzstd_hip_ungroup_cmp(0, None, vrows, n, d_rows, stage.data_ptr(), size, cw_a.data_ptr()))
                    t1 = timed(lambda: L.qzstd_hip_ungroup_cmp_pieces(0, None, rows.ctypes.data, n, d_rows, pieces.ctypes.data, np_, d_pieces,
                                                                      stage.data_ptr(), size, cw_b.data_ptr()))
                    if i:
                        runs["ungroup_cmp"].append(t0)
                        runs[key].append(t1)
                assert torch.equal(cw_a, cw_b) and bool((cw_a == -1).all()), (k, name)
                cw_b.zero_()
            cells["ungroup_cmp_k%d" % k] = {leg + "_ms_per_gib": v for leg, v in runs.items()}
    finally:
        L.qzstd_hip_free(0, d_rows)
        L.qzstd_hip_free(0, d_pieces)
    out["kernels"] = {"rows": n, "row_bytes": a.chunk, "cells": cells, "piece_table_bytes": {name: size // w * 24 for name, w in widths},
                      "timed": "events around ONE launcher call each (rows and pieces uploaded inside, from pinned memory) over the same %d rows of %d "
                               "bytes of random bytes, no base, ms per GiB of rows; the contiguous kernel and the kernel from pieces alternate, every "
                               "run of %d after one untimed round" % (n, a.chunk, a.reps)}


def slicecheck_main(a):
    """--slicecheck: QZSTD_frontFingerprintDeviceSlices, QZSTD_frontCheckDeviceSlices and QZSTD_frontVerifyDeviceSlices on a column view (the
    --srcslices setting) against view.contiguous() + the contiguous call and against that call on a tensor that is contiguous already; then the
    two kernels beside their contiguous neighbours.  --kernels: the kernel legs alone"""
    import ctypes as C
    rows_n = (int(a.gib * 65536) + 15) & ~15
    rowb, width = 16384, 8192
    size = rows_n * width
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "reps": a.reps, "dtype": "bf16 N(0, 0.02)", "matrix_bytes": [rows_n, rowb],
           "slices": rows_n, "slice_bytes": width}
    if a.kernels:
        slicecheck_kernels(a, int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1), out)
        return print(json.dumps(out))
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    torch.manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    n = size // a.chunk
    out["timed"] = ("GB/s of tensor bytes, every run, the legs alternating in one run; the window holds the call (the slice and buffer arrays exist "
                    "before it), for `contiguous` the .contiguous() copies, and the closing synchronize")
    out["peak_extra_device_bytes"] = ("torch's peak allocation above the level before the call (the .contiguous() temporaries); the library's own "
                                      "scratch is the same in all legs and not included")
    mat = (torch.randn(rows_n * rowb // 2, device="cuda:0") * 0.02).to(torch.bfloat16).view(torch.uint8).view(rows_n, rowb)
    bmat = ((mat.view(torch.bfloat16).float() + torch.randn(rows_n, rowb // 2, device="cuda:0") * 1e-5).to(torch.bfloat16)).view(torch.uint8).view(rows_n, rowb)
    mat, bmat = bmat, mat  # (the new checkpoint is the update; the base is what it came from)
    view, bview = mat[:, :width], bmat[:, :width]
    flat, bflat = view.contiguous(), bview.contiguous()
    out["cells"] = {}
    fr = D.DeviceFront(a.threads, 1, a.chunk, lib=lib)
    try:
        fr.reserve(size)
        _, sizes = fr._frame_buffers(n)
        first = (C.c_size_t * 2)()
        es = bytes([2]) + b"\0"
        bs = (C.c_size_t * 1)(size)
        fp = (C.c_ulonglong * n)()
        got = (C.c_ulonglong * n)()
        flags = C.create_string_buffer(n)
        fd = (C.c_size_t * n)()
        fbufs, fbase = fr.batch([(flat.data_ptr(), size)])[0], fr.batch([(bflat.data_ptr(), size)])[0]
        assert fr.lib.QZSTD_frontFingerprintDeviceBatch(fr.f, fbufs, 1, stream, fp, None) == n
        for based in (False, True):
            sl = [(0, r * width, width, view.data_ptr() + r * rowb, bview.data_ptr() + r * rowb if based else None) for r in range(rows_n)]
            arr = fr.src_slice_array(sl)
            assert fr.lib.QZSTD_frontCompressDeviceBatchDelta(fr.f, fbufs, fbase if based else None, es, 1, stream, fr._dst, len(fr._dst), sizes, first) == n
            cbuf = lambda t: fr.batch([(t.data_ptr(), size)])[0]  # noqa: E731
            calls = {
                "fingerprint": (lambda: fr.lib.QZSTD_frontFingerprintDeviceSlices(fr.f, bs, 1, arr, rows_n, stream, got, None),
                                lambda t, b: fr.lib.QZSTD_frontFingerprintDeviceBatch(fr.f, cbuf(t), 1, stream, got, None), n),
                "check": (lambda: fr.lib.QZSTD_frontCheckDeviceSlices(fr.f, bs, 1, arr, rows_n, stream, fp, n, flags),
                          lambda t, b: fr.lib.QZSTD_frontCheckDeviceBatch(fr.f, cbuf(t), 1, stream, fp, n, flags), 0),
                "verify": (lambda: fr.lib.QZSTD_frontVerifyDeviceSlices(fr.f, fr._dst, fr.stride, sizes, n, bs, es, 1, arr, rows_n, stream, fd),
                           lambda t, b: fr.lib.QZSTD_frontVerifyDeviceBatch(fr.f, fr._dst, fr.stride, sizes, n, cbuf(t), cbuf(b) if based else None, es, 1,
                                                                            stream, fd), 0)}
            for what, (on_slices, on_buffer, want) in calls.items():
                if based and what != "verify":
                    continue  # (a base is no part of a fingerprint)
                legs = (("slices", on_slices), ("contiguous", lambda: on_buffer(view.contiguous(), bview.contiguous() if based else None)),
                        ("typed", lambda: on_buffer(flat, bflat)))
                cell = out["cells"]["%s_%s" % (what, "base" if based else "nobase")] = {}
                for name, leg in legs:  # untimed, and checked
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    m0, p0 = torch.cuda.memory_allocated(), fr.slice_check_stats()
                    assert leg() == want, (what, name)
                    torch.cuda.synchronize()
                    cell[name] = {"peak_extra_device_bytes": torch.cuda.max_memory_allocated() - m0, "gbps": []}
                    if what == "fingerprint":
                        assert list(got) == list(fp), name
                    if name == "slices":
                        cell[name]["slice_check_stats"] = [y - x for x, y in zip(p0, fr.slice_check_stats())]
                for _ in range(a.reps):
                    for name, leg in legs:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert leg() == want, (what, name)
                        torch.cuda.synchronize()
                        cell[name]["gbps"].append(round(size / (time.perf_counter() - t0) / 1e9, 3))
    finally:
        fr.close()
    del mat, bmat, view, bview, flat, bflat
    torch.cuda.empty_cache()
    slicecheck_kernels(a, int(a.gib * (1 << 30)) & ~(64 * a.chunk - 1), out)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--srcslices", action="store_true")
    ap.add_argument("--slicecheck", action="store_true")
    ap.add_argument("--advise", action="store_true")
    ap.add_argument("--ediff", action="store_true")
    ap.add_argument("--fingerprint", action="store_true")
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--code", action="store_true", help="the plane code (QZSTD_frontSetPlaneCode) beside the plane probe; --kernels: the coder beside the cost kernel")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--skip", action="store_true")
    ap.add_argument("--slices", action="store_true")
    ap.add_argument("--delta", action="store_true")
    ap.add_argument("--restore", action="store_true")
    ap.add_argument("--group", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="--group, --restore, --delta, --skip, --verify: the passes to trace, nothing timed; --probe: the two kernels timed")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--checksum", action="store_true")
    ap.add_argument("--legs", default="host,device,batch", help="--checksum: the legs to run")
    ap.add_argument("--no-compare", action="store_true", help="--checksum: skip the closing comparison of the two paths' frames (kernel traces)")
    ap.add_argument("--ways", default="batch,loop,cat")
    ap.add_argument("--mixes", default="a_128k,b_loguniform,c_one")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=131072)
    ap.add_argument("--levels", default="1,6,12")
    a = ap.parse_args()
    if a.slicecheck:
        return slicecheck_main(a)
    if a.srcslices:
        if a.levels == "1,6,12":
            a.levels = "1,6"
        return srcslices_main(a)
    if a.advise:
        return advise_main(a)
    if a.ediff:
        if a.levels == "1,6,12":
            a.levels = "1,6"
        return ediff_main(a)
    if a.fingerprint:
        return fingerprint_main(a)
    if a.code:
        return code_main(a)
    if a.probe:
        return probe_main(a)
    if a.verify:
        return verify_main(a)
    if a.skip:
        if a.levels == "1,6,12":
            a.levels = "1,6"
        return skip_main(a)
    if a.slices:
        return slices_main(a)
    if a.delta:
        return delta_main(a)
    if a.restore:
        return restore_main(a)
    if a.group:
        if a.legs == "host,device,batch":
            a.legs = "off,on,torch,host"
        return group_main(a)
    if a.checksum:
        return checksum_main(a)
    if a.batch:
        return batch_main(a)
    B.Zstd()
    B.Plugin()
    lib = B.Front().lib
    size = int(a.gib * (1 << 30))
    n = (size + a.chunk - 1) // a.chunk
    data = K.by_name("system", size)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    del data
    torch.cuda.synchronize()
    out = {"bytes": size, "chunk": a.chunk, "threads": a.threads, "timed": "library calls (+ t.cpu() for the host way), best of %d" % a.reps,
           "levels": {}}
    for level in [int(x) for x in a.levels.split(",")]:
        fr = D.DeviceFront(a.threads, level, a.chunk, lib=lib)
        try:
            fr.reserve(size)
            stream = torch.cuda.current_stream().cuda_stream

            def host_pass():
                h = t.cpu()
                return fr.call_host(h.data_ptr(), size)

            def device_pass():
                return fr.call_device(t.data_ptr(), size, stream)

            for f in (host_pass, device_pass):  # untimed: first-touch of the destination, the device slots, the pinned arenas
                assert f()[0] == n
            best = {"host": None, "device": None}
            s0 = fr.stats()
            for _ in range(a.reps):
                for name, f in (("host", host_pass), ("device", device_pass)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r, _ = f()
                    dt = time.perf_counter() - t0
                    assert r == n, "%s pass failed" % name
                    best[name] = dt if best[name] is None else min(best[name], dt)
            s1 = fr.stats()
            r, sizes = host_pass()
            frames_h = fr.frames(n, sizes)
            r, sizes = device_pass()
            frames_d = fr.frames(n, sizes)
            out["levels"][str(level)] = {
                "host_gbps": round(size / best["host"] / 1e9, 3), "device_gbps": round(size / best["device"] / 1e9, 3),
                "host_ms": round(best["host"] * 1e3, 1), "device_ms": round(best["device"] * 1e3, 1),
                "d2h_bytes_per_input_byte": round((s1[2] - s0[2]) / a.reps / size, 4),
                "raw_fallback_frames": (s1[1] - s0[1]) // a.reps, "seqlit_frames": (s1[0] - s0[0]) // a.reps,
                "compressed_host": sum(len(x) for x in frames_h), "compressed_device": sum(len(x) for x in frames_d),
                "frames_identical_to_host_path": frames_h == frames_d}
        finally:
            fr.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
