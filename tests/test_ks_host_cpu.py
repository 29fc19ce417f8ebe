"""CPU checks of csrc/ks_host.hpp, the host arithmetic that the key switch and its drivers share (spans and overlaps,
the key switch's block of the workspace, the launch geometry of the row kernels): tests/cpp/ks_host_main.cpp, which
includes that header alone, is built with the host compiler under the address and undefined-behaviour sanitizers, run
once, and every line it prints is compared with a restatement of the rule in Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"


def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return cc
    llvm = Path("/opt/rocm/lib/llvm/bin/clang++")
    return str(llvm) if llvm.exists() else None


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """The program's output, grouped by the first word of each line."""
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("ks_host") / "ks_host_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "ks_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        kind, *rest = ln.split()
        out.setdefault(kind, []).append(rest)
    return out


def _ints(rows):
    return [[int(v) for v in r] for r in rows]


def _prun(npoly, bx, rows, min_run=4):
    """runs = max(1, 4096 / (bx rows)) workgroup columns, prun = ceil(npoly / runs), but never below min_run (or the
    batch, when that is smaller): tests/test_ks_shapes_gpu.py's _prun."""
    runs = max(1, 4096 // (bx * rows))
    prun = -(-npoly // runs)
    return prun if prun >= min_run else min(npoly, min_run)


def test_the_header_includes_the_standard_library_alone():
    text = (CSRC / "ks_host.hpp").read_text()
    assert "#include <hip" not in text and '#include "' not in text


def test_block_and_bx(lines):
    want = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1 << 15):
        block = 256 if n >= 256 else -(-n // 64) * 64
        want.append([n, block, -(-n // block)])
    assert _ints(lines["grid"]) == want
    assert [w[1:] for w in want] == [[64, 1], [64, 1], [64, 1], [64, 1], [128, 1], [256, 1], [256, 1], [256, 2],
                                     [256, 128]]


def test_wide_decision_and_halving(lines):
    """16-byte form: every stride even (the row length among them) and every pointer 16-byte aligned; only then are
    the strides halved."""
    assert lines["wide"] == [["even-aligned", "1", "8", "16", "24"], ["odd-stride", "0", "16", "33", "48"],
                             ["pointer-off-8", "0", "16", "32", "48"], ["odd-ncoeff", "0", "15", "32", "48"]]


def test_prun_rule(lines):
    """Minimum run 4, one block column of 7 rows, the counts of tests/test_ks_shapes_gpu.py.  The limit of 65535 on grid z
    is part of the rule but cannot bind: runs <= max(1, 4096 / (bx rows)) <= 4096 before the minimum run, which only
    lowers it; the last case is the longest grid z there is."""
    got = _ints(lines["runs"])
    small = [0, 1, 3, 4, 2340, 2341, 3001]
    assert [g[0] for g in got] == small + [1 << 40]
    for n, bx, rows, min_run, prun, runs in got[:-1]:
        assert (bx, rows, min_run) == (1, 7, 4)
        assert prun == _prun(n, bx, rows), n
        assert runs == (-(-n // prun) if n else 0), n
    assert [g[4] for g in got[:-1]] == [0, 1, 3, 4, 4, 5, 6]
    n, bx, rows, min_run, prun, runs = got[-1]
    assert (bx, rows, min_run) == (1, 1, 4) and prun == _prun(n, 1, 1) == 1 << 28
    assert runs == 4096 <= 65535


def test_automorphism_fold(lines):
    want = []
    for rows, npoly in ((3, 21845), (3, 21846), (1, 65543)):
        total = rows * npoly
        gy = min(total, 65535)
        want.append([rows, npoly, gy, -(-total // gy)])
    assert _ints(lines["fold"]) == want
    assert [w[2:] for w in want] == [[65535, 1], [65535, 2], [65535, 2]]


def test_workspace_block(lines):
    got = _ints(lines["ws"])
    assert [g[:4] for g in got] == [[1, 1, 2, 2], [3, 3, 7, 16], [0, 2, 7, 16]]
    for npoly, beta, rows, n, raised, acc, scratch, end, words in got:
        pw = rows * n   # one raised polynomial
        assert raised == 0
        assert acc == beta * npoly * pw
        assert scratch == acc + 2 * npoly * pw
        assert end == scratch + 2 * npoly * pw
        assert end == words == (beta + 4) * npoly * pw


def test_span_and_overlap(lines):
    assert _ints(lines["span"]) == [[0, 10, 4, 0], [1, 10, 4, 4], [3, 10, 4, 24]]
    none, an_input, outputs = "0", "1", "2"
    assert lines["overlap"] == [["disjoint", none], ["touching", none], ["one-word-shared", an_input],
                                ["empty-input-inside-output", none], ["empty-output-inside-input", none],
                                ["output-against-output", outputs], ["second-output-against-input", an_input]]
