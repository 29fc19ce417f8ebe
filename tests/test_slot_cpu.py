"""CPU checks of the slot encoder's model (tests/slot_model.py) and of what the library declares: the longdouble FFT
model against the O(N^2) definition and against the Vandermonde encoder of tests/test_lintrans_cpu.py, the t_j map,
the slot order under the Galois automorphisms, the two-limb Garner lift, the launch geometry, workspace size and t_j
table of csrc/slot.hpp (a stand-alone host program built under the address and undefined-behaviour sanitizers), the
bytes model of tools/slot_bench.py, and the exported symbols."""
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

import galois_model as gm
import slot_model as sm
import test_lintrans_cpu as tl
from primes import primes_of_size

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"
NEW = ["mfhe_slot_reserve", "mfhe_slot_encode", "mfhe_slot_decode"]


def test_new_symbols_declared_and_exported(mfhe):
    names = mfhe.declared_symbols()
    for n in NEW:
        assert n in names, n
        assert hasattr(mfhe.lib, n), n
        assert getattr(mfhe.lib, n).argtypes is not None, n
    for m in ("slot_reserve", "slot_encode", "slot_decode"):
        assert callable(getattr(mfhe.Context, m)), m
    assert mfhe.SLOT_REAL == 1 and mfhe.SLOT_COEFF == 2
    lib = mfhe.lib
    assert lib.mfhe_slot_reserve(None, 1, 1, 0, 0) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()
    assert lib.mfhe_slot_encode(None, 8, 1, 1.0, 8, 1, 1, 1, 0, 0, 0, None) == mfhe.EINVAL
    assert lib.mfhe_slot_decode(None, 8, 1, 1.0, 8, 1, 1, 1, 0, None) == mfhe.EINVAL


@pytest.mark.parametrize("log_n", range(2, 9))
def test_model_equals_the_definition(log_n):
    """Both maps of the longdouble model against the O(N^2) sums, to a few longdouble ulps of the largest value."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    rng = np.random.default_rng(log_n)
    z = rng.random(n) + 1j * rng.random(n)
    m = rng.integers(-2 ** 40, 2 ** 40, N)
    eps = float(np.finfo(sm.LD).eps)
    c, cd = sm.slots_to_coeffs(z, log_n), sm.definition_encode(z, log_n)
    assert float(np.abs(c - cd).max()) <= 4 * log_n * eps * float(np.abs(cd).max() + 1)
    s, sd = sm.coeffs_to_slots(m, log_n), sm.definition_decode(m, log_n)
    assert float(np.abs(s - sd).max()) <= 4 * log_n * eps * N * 2.0 ** 40
    # the float64 forms agree with the model at float64's level, and the two maps invert each other
    assert float(np.abs(sm.slots_to_coeffs_f64(z, log_n) - c).max()) <= 16 * log_n * 2.0 ** -53
    assert float(np.abs(sm.coeffs_to_slots_f64(m, log_n) - s).max()) <= 16 * log_n * 2.0 ** -53 * N * 2.0 ** 40
    assert float(np.abs(sm.coeffs_to_slots(c, log_n) - z).max()) <= 16 * log_n * eps


def test_model_equals_the_vandermonde_encoder_at_16():
    """tests/test_lintrans_cpu.py's _encode / _decode (float64, N = 16) are the same maps in the same slot order."""
    rng = np.random.default_rng(16)
    z = rng.uniform(-1, 1, 8) + 1j * rng.uniform(-1, 1, 8)
    scale = float(1 << 30)
    ints, _ = sm.encode_int(z, 4, scale)
    theirs = tl._encode(z, 16, scale)
    assert max(abs(a - b) for a, b in zip(ints, theirs)) <= 1     # a half-way case may round either way
    back = sm.coeffs_to_slots(ints, 4) / sm.LD(scale)
    np.testing.assert_allclose(back.astype(np.complex128), tl._decode(ints, 16, scale), atol=1e-12)
    roots = tl._slot_roots(16)
    np.testing.assert_allclose(np.exp(1j * np.pi * (4 * sm.t_map(4) + 1) / 16), roots, atol=1e-15)


@pytest.mark.parametrize("log_n", range(2, 18))
def test_t_map_is_a_permutation(log_n):
    t = sm.t_map(log_n)
    n = 1 << (log_n - 1)
    assert sorted(t.tolist()) == list(range(n))
    assert t[0] == 0 and (log_n < 3 or t[1] == 1)
    g = 4 * t + 1
    assert all(int(g[j]) == pow(5, j, 2 << log_n) for j in (0, 1, n // 2, n - 1))


@pytest.mark.parametrize("log_n", [4, 7])
def test_galois_elements_rotate_and_conjugate_the_slots(log_n):
    """sigma_(5^k) of an encoded polynomial decodes to np.roll(z, -k), sigma_(2N - 1) to the conjugate."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    rng = np.random.default_rng(log_n)
    z = rng.random(n) + 1j * rng.random(n)
    scale = 2.0 ** 40
    ints, _ = sm.encode_int(z, log_n, scale)
    tol = N / scale
    for k in (1, 3, n - 1):
        got = sm.coeffs_to_slots(gm.sigma(ints, gm.galois_elt(k, log_n)), log_n) / sm.LD(scale)
        assert float(np.abs(got - np.roll(z, -k)).max()) <= tol, k
    got = sm.coeffs_to_slots(gm.sigma(ints, 2 * N - 1), log_n) / sm.LD(scale)
    assert float(np.abs(got - np.conj(z)).max()) <= tol


@pytest.mark.parametrize("bits", [(45, 49), (50, 61)])
def test_garner_lift_equals_python_integers(bits):
    q0 = primes_of_size(bits[0], 32, 1)[0]
    q1 = primes_of_size(bits[1], 32, 2)[-1]
    assert q0 != q1 and q0 * q1 < 2 ** 124
    half = (q0 * q1 - 1) // 2
    for x in (half, -half, 0, 1, -1, half - 1, 12345678901234567890123 % half):
        assert sm.garner_lift(x % q0, x % q1, q0, q1) == x
    assert sm.center((q0 - 1) // 2, q0) == (q0 - 1) // 2 and sm.center((q0 + 1) // 2, q0) == -((q0 - 1) // 2)


def _bench_module():
    spec = importlib.util.spec_from_file_location("slot_bench", ROOT / "tools" / "slot_bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bytes_model_of_the_bench_tool():
    sb = _bench_module()
    N, b = 1 << 16, 64
    assert sb.encode_bytes(N, b, 14) == 8 * N * b * 15                 # N doubles in, 14 rows of N words out
    assert sb.encode_bytes(N, b, 11) == 8 * N * b * 12
    assert sb.encode_bytes(N, b, 14, real=True) == 8 * N * b * 14.5    # N / 2 doubles in
    assert sb.decode_bytes(N, b, 2) == 8 * N * b * 3                   # two rows in, N doubles out
    assert sb.decode_bytes(N, b, 1) == 8 * N * b * 2
    assert sb.two_pass_bytes(16, b) == 2 * 8 * N * b                   # [b][N / 2] double2 written and read
    assert sb.two_pass_bytes(13, b) == 0 and sb.two_pass_bytes(14, b) == 2 * 8 * (1 << 14) * b   # the switch: see
    # test_launch_geometry_fits_the_tile_for_every_size_and_batch, which ties WHOLE_MAX_LOG to csrc/slot.hpp


# ---------------------------------------------------------------------------------------------------------------
# csrc/slot.hpp on the host: geometry, workspace, table
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geom_prog(tmp_path_factory):
    cc = tl._host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("slot") / "slot_geom_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "slot_geom_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(prog, *args):
    r = subprocess.run([str(prog)] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return [int(v) for v in r.stdout.split()]


def test_launch_geometry_fits_the_tile_for_every_size_and_batch(geom_prog):
    """Every launch's transform length times its columns fits the 2^tile_log tile, the two-pass tiles divide n1 and n2,
    the whole form holds 2^lcW polynomials per workgroup only while that leaves 512 workgroups, and the workspace is
    the intermediate plus the dense rows."""
    threads, tile_log, whole_max = _run(geom_prog, "consts")
    assert threads == 512 and tile_log == 12 and whole_max <= tile_log
    assert _bench_module().WHOLE_MAX_LOG == whole_max, "tools/slot_bench.py mirrors kSlotWholeMaxLog"
    for log_n in range(2, 18):
        for npoly in (1, 3, 511, 512, 1023, 1024, 2050, 4100, 1 << 20):
            ln, whole, l1, l2, lcA, lcB, lcW, ws = _run(geom_prog, "geom", log_n, npoly, 5)
            assert ln == log_n - 1 and whole == (ln <= whole_max)
            N = 1 << log_n
            if whole:
                assert 0 <= lcW and ln + lcW <= tile_log
                blocks = -(-npoly // (1 << lcW))
                assert lcW == 0 or blocks >= 512, "a tile holds several polynomials only in a large batch"
                assert lcW == tile_log - ln or -(-npoly // (2 << lcW)) < 512, "and as many as that allows"
                assert ws == npoly * N * 5
            else:
                assert l1 + l2 == ln and l1 == ln // 2
                assert l2 + lcA == tile_log and l1 + lcB == tile_log
                assert 1 <= lcA <= l1 and 1 <= lcB <= l2, "tiles divide n1 and n2; the 16-byte form needs lcB >= 1"
                assert ws == npoly * N * 6
    assert _run(geom_prog, "geom", 4, 2050, 2)[6] == 2 and _run(geom_prog, "geom", 6, 4100, 2)[6] == 3   # the GPU cases


@pytest.mark.parametrize("log_n", [2, 3, 4, 10, 17])
def test_jinv_table_inverts_the_t_map(geom_prog, log_n):
    jinv = np.array(_run(geom_prog, "jinv", log_n))
    t = sm.t_map(log_n)
    assert jinv.shape == t.shape
    np.testing.assert_array_equal(jinv[t], np.arange(len(t)))
