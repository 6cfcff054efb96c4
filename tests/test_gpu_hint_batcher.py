"""GPU: the announcement batcher under the runtime's hardware queue counts.  Announced claims of every worker go into a few device-wide
launches on the batcher's own streams, so how many of them run at once no longer depends on GPU_MAX_HW_QUEUES.  The batch front-end (the
bench's headline leg) runs in child processes — the queue count is read once, when HIP starts — with 4 queues (the runtime's default)
and with 16: every frame is libzstd's frame from the ORACLE's sequences and every block is served from an announcement."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import qz_bind as B
import qz_corpus as K
level, chunk, threads = 1, 131072, 17
z = B.Zstd()
plug = B.Plugin()
assert plug.lib.qzstd_hip_device_count() > 0, plug.err()
front = B.Front()
data = K.by_name("system", 192 * chunk + 777, seed=81)
n = (len(data) + chunk - 1) // chunk
frames, st, fs = front.frames(data, chunk, level, threads, segment=16 * chunk, jobs=2)
zo = z.cctx(level, producer=B.Oracle().producer_addr, state=None, fallback=False, validate=True)
_, want = z.compress_chunks(zo, data, chunk)
z.free(zo)
plug.lib.QZSTD_stopQatDevice()
print(json.dumps({"n": n, "frames": len(frames), "differ": [c for c in range(n) if frames[c] != want[c]][:8],
                  "announced": st[0], "per_block_path": st[1], "errors": fs[0]}))
"""


@pytest.mark.parametrize("queues", ["4", "16"])
def test_front_end_served_from_batched_announcements(gpu_plugin, queues):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=queues)
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "tools")], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["frames"] == out["n"] and not out["differ"], out
    assert out["announced"] == 2 * out["n"] and out["per_block_path"] == 0 and out["errors"] == 0, out
