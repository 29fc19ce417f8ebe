"""CPU checks of the RNS basis conversion layer (include/mfhe.h mfhe_rns_bconv .. mfhe_ntt_moddown): exported
symbols, argument validation without a device, the host table builder against Python integers (a stand-alone
program built under the address and undefined-behaviour sanitizers), and the one-launch construction of
mfhe_rns_modup."""
import ctypes
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from primes import primes_of_size

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"
NEW = ["mfhe_rns_bconv_reserve", "mfhe_rns_bconv", "mfhe_rns_moddown", "mfhe_rns_modup", "mfhe_ntt_bconv_reserve",
       "mfhe_ntt_modup", "mfhe_ntt_moddown"]


def test_new_symbols_declared_and_exported(mfhe):
    names = mfhe.declared_symbols()
    for n in NEW:
        assert n in names, n
        assert hasattr(mfhe.lib, n), n
        assert getattr(mfhe.lib, n).argtypes is not None, n   # a _sig entry exists
    for m in ("rns_bconv", "rns_moddown", "rns_rescale", "rns_modup", "ntt_modup", "ntt_moddown",
              "rns_bconv_reserve", "rns_moddown_reserve", "rns_modup_reserve", "ntt_bconv_reserve"):
        assert callable(getattr(mfhe.Context, m)), m
    assert (mfhe.BCONV_FAST, mfhe.BCONV_CENTERED) == (0, 1)


def test_null_context_is_einval(mfhe):
    lib = mfhe.lib
    assert lib.mfhe_rns_bconv_reserve(None, 0, 1, 1, 1) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()
    assert lib.mfhe_rns_bconv(None, 8, 1, 8, 1, 1, 1, 0, 1, 1, 1, 0, None) == mfhe.EINVAL
    assert lib.mfhe_rns_moddown(None, 8, 2, 8, 1, 1, 1, 1, 1, 1, None) == mfhe.EINVAL
    assert lib.mfhe_rns_modup(None, 8, 1, 8, 2, 1, 1, 1, 0, 1, 1, 1, None) == mfhe.EINVAL
    assert lib.mfhe_ntt_bconv_reserve(None, 1, 2) == mfhe.EINVAL
    assert lib.mfhe_ntt_modup(None, 8, 1, 8, 2, 1, 1, 0, 1, 1, 1, None) == mfhe.EINVAL
    assert lib.mfhe_ntt_moddown(None, 8, 2, 8, 1, 1, 1, 1, 1, None) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()


def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return cc
    llvm = Path("/opt/rocm/lib/llvm/bin/clang++")
    return str(llvm) if llvm.exists() else None


@pytest.fixture(scope="module")
def tables_prog(tmp_path_factory):
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("bconv") / "bconv_tables_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "bconv_tables_main.cpp"), str(CSRC / "host_math.cpp"),
           "-pthread", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _expected_lines(src, dst):
    S = 1
    for s in src:
        S *= s
    out = []
    for i, s in enumerate(src):
        inv = pow(S // s, -1, s)
        out.append(f"inv {i} {inv} {(inv << 64) // s}")
        out.append(f"sinv {i} {struct.unpack('<Q', struct.pack('<d', 1.0 / float(s)))[0]}")
    for j, d in enumerate(dst):
        for i, s in enumerate(src):
            out.append(f"c {j} {i} {(S // s) % d}")
        out.append(f"smod {j} {S % d}")
        pinv = pow(S, -1, d)
        out.append(f"pinv {j} {pinv} {(pinv << 64) // d}")
    return out


MIXED = (primes_of_size(20, 2, 2) + primes_of_size(35, 2, 2) + primes_of_size(50, 2, 2) + primes_of_size(55, 2, 2) +
         primes_of_size(61, 2, 2))


@pytest.mark.parametrize("src,dst", [
    (MIXED[:1], MIXED[1:]),
    (MIXED[2:5], MIXED[:2] + MIXED[5:]),
    (primes_of_size(61, 2, 17), primes_of_size(55, 2, 3)),
    ([18014398515156481, 549757491457, 549759662593],
     [17592186435073, 17182765057, 17184541441, 17186120449, 17186515201, 17186909953, 17188883713, 17190462721,
      17190857473, 17191844353, 17192831233]),
], ids=["one-source", "mixed-sizes", "17-source-61-bit", "reference-P-to-Q"])
def test_host_tables_match_python_integers_under_sanitizers(tables_prog, src, dst):
    r = subprocess.run([str(tables_prog), str(len(src))] + [str(v) for v in src + dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == _expected_lines(src, dst)


def test_tables_prog_rejects_bad_input(tables_prog):
    assert subprocess.run([str(tables_prog), "1", "1", "7"], capture_output=True).returncode == 3   # modulus < 2


def _body(text, name):
    """Source text of the extern "C" function `name` in bconv.hip (up to the closing brace in column 0)."""
    m = re.search(r'^(?:extern "C" )?(?:static )?int ' + name + r"\(.*?^}", text, re.S | re.M)
    assert m, name
    return m.group(0)


def test_modup_and_moddown_are_one_launch_by_construction():
    text = (CSRC / "bconv.hip").read_text()
    launcher = _body(text, "launch_bconv")
    assert launcher.count("hipLaunchKernelGGL(") == 1
    for name in ("mfhe_rns_modup", "mfhe_rns_moddown", "mfhe_rns_bconv"):
        body = _body(text, name)
        assert body.count("launch_bconv(") == 1, name
        assert "hipLaunchKernelGGL" not in body and "mfhe_ntt_" not in body and "hipMemcpy" not in body, name
        # the only other launcher is the copy of a ModUp whose digit is the whole basis, an early return
        assert body.count("launch_copy_rows(") == (1 if name == "mfhe_rns_modup" else 0), name
    modup = _body(text, "mfhe_rns_modup")
    assert re.search(r"if \(pl\.nr == 0\)[^\n]*\n\s*return launch_copy_rows\(", modup)
