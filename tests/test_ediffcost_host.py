"""CPU: the element-difference cost (include/qzstd_ediffcost.h) under the sanitizers — the stand-alone checker
tests/ediffcost/ediffcost_check.c and frontend/qzstd_elemdiff.c compiled into ONE executable with -fsanitize=address,undefined and run as a
process of its own: QZSTD_ediffCostTile / QZSTD_ediffCostChunk against a naive recomputation (QZSTD_elemDiff over the whole chunk, then a
histogram per tile and plane) for every k, the edge lengths around an element and a tile, and six contents; the rule's edge.  The header
compiles as C99 with the product's warnings."""
import os
import subprocess

import qz_bind as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "include")]


def test_standalone_ediffcost_checker_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ediffcost_check")
    flags = ["-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer"] + INC
    subprocess.check_call(["gcc"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "ediffcost", "ediffcost_check.c"),
                                             os.path.join(B.PKG_DIR, "frontend", "qzstd_elemdiff.c")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])


def test_header_compiles_as_c99_with_the_products_warnings(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "qzstd_ediffcost.h"\n'
                   "int use(const void *p, unsigned long n)\n{\n    uint64_t s[2];\n    QZSTD_ediffCostChunk(p, n, 4, s);\n"
                   "    return QZSTD_ediffAdvised(s[0], s[1]);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-Wshadow", "-Wcast-align", "-Wundef", "-Wpointer-arith",
                           "-c", str(src), "-o", str(tmp_path / "use.o")] + INC)
