"""CPU checks of the Galois layer (include/mfhe.h mfhe_ntt_automorphism .. mfhe_galois_reserve): exported symbols, the
evaluation-domain gather of tests/galois_model.py against a direct evaluation at the slot points, its block property,
the Galois elements of rotations and the conjugation, the hoisted rotation model against the key switch's error bound
and its margin from +-P/2, and csrc/galois.hpp's index function in a stand-alone program built under the address and
undefined-behaviour sanitizers.

Shape of the model cases: N = 16, 5 Q primes + 2 special primes, alpha 2, levels 5, 3 and 2 (the key is made at
level 5), g in {5, 25, 3, 13, 31}."""
import shutil
import subprocess
from pathlib import Path

import pytest

import galois_model as gm
import ks_model as km
from primes import primes_of_size

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"
NEW = ["mfhe_ntt_automorphism", "mfhe_ksk_inner_product_galois", "mfhe_keyswitch_raise", "mfhe_galois_apply_raised",
       "mfhe_galois_apply", "mfhe_galois_reserve"]


def test_new_symbols_declared_and_exported(mfhe):
    names = mfhe.declared_symbols()
    for n in NEW:
        assert n in names, n
        assert hasattr(mfhe.lib, n), n
        assert getattr(mfhe.lib, n).argtypes is not None, n   # a _sig entry exists
    for m in ("automorphism", "ksk_inner_product_galois", "keyswitch_raise", "galois_apply_raised", "galois_apply",
              "galois_reserve", "gen_galois_key"):
        assert callable(getattr(mfhe.Context, m)), m
    assert callable(mfhe.galois_elt) and callable(mfhe.galois_conj)


def test_null_context_is_einval(mfhe):
    lib = mfhe.lib
    assert lib.mfhe_ntt_automorphism(None, 8, 16, 1024, 16, 1, 1, 3, None) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()
    assert lib.mfhe_ksk_inner_product_galois(None, 8, 1, 1, 8, 8, 1, 1, 1, 1, 1, 1, 1, 3, None) == mfhe.EINVAL
    assert lib.mfhe_keyswitch_raise(None, 8, 1, 8, 1, 1, 1, 1, 1, 1, 1, None) == mfhe.EINVAL
    assert lib.mfhe_galois_apply_raised(None, 8, 1, 8, 1, 1, 8, 8, 8, 1, 1, 1, 1, 1, 1, 1, 3, None) == mfhe.EINVAL
    assert lib.mfhe_galois_apply(None, 8, 8, 1, 8, 8, 8, 1, 1, 1, 1, 1, 1, 1, 3, None) == mfhe.EINVAL
    assert lib.mfhe_galois_reserve(None, 1, 1, 1, 1, 1, 1) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()


def _odd_elts(log_n):
    m = 2 << log_n
    return sorted({1, 3 % m, 5 % m, pow(5, 7, m), m - 1} | ({g for g in range(1, m, 2)} if log_n <= 4 else set()))


@pytest.mark.parametrize("log_n", [1, 2, 4, 6])
def test_perm_is_sigma_at_the_slot_points(log_n):
    """Slot i holds a(psi^(2 brev(i) + 1)) (tests/test_oracle_kat.py): evaluating sigma_g(a) there, by Horner in
    Python integers, gives the slots of a gathered through perm."""
    n = 1 << log_n
    q = primes_of_size(30, 2 * n, 1)[0]
    psi = next(w for w in (pow(x, (q - 1) // (2 * n), q) for x in range(2, 200)) if pow(w, n, q) == q - 1)
    rnd = __import__("random").Random(log_n)
    a = [rnd.randrange(q) for _ in range(n)]

    def slots(poly):
        out = []
        for i in range(n):
            x, acc = pow(psi, 2 * gm.brev(i, log_n) + 1, q), 0
            for v in reversed(poly):
                acc = (acc * x + v) % q
            out.append(acc)
        return out

    ev = slots(a)
    for g in _odd_elts(log_n):
        pi = gm.perm(log_n, g)
        assert sorted(pi) == list(range(n)), g
        assert slots(gm.sigma(a, g)) == [ev[j] for j in pi], g
    assert gm.perm(log_n, 1) == list(range(n))


@pytest.mark.parametrize("log_n", [1, 4, 8, 12])
def test_aligned_blocks_map_into_aligned_blocks(log_n):
    """An aligned block of 2^m consecutive outputs reads one aligned block of 2^m sources; m = 1 is what the 16-byte
    kernels use (the pair pi(2c) >> 1, swapped when pi(2c) is odd), m = 7 is one wave's 1 KiB."""
    n = 1 << log_n
    m2 = 2 * n
    for g in (1, 3 % m2, 5 % m2, pow(5, 7, m2), pow(5, 1000, m2), m2 - 1):
        pi = gm.perm(log_n, g)
        for m in (1, 7):
            if m > log_n:
                continue
            for b in range(0, n, 1 << m):
                assert len({pi[i] >> m for i in range(b, b + (1 << m))}) == 1, (g, m, b)
        for c in range(n // 2):
            assert pi[2 * c + 1] == pi[2 * c] ^ 1, (g, c)


def test_galois_elements_of_rotations_and_conjugation(mfhe):
    for log_n in (1, 4, 8, 16, 17):
        m = 2 << log_n
        assert mfhe.galois_conj(log_n) == m - 1
        assert mfhe.galois_elt(0, log_n) == 1
        for k in (1, 2, 7, 1000):
            g, gi = mfhe.galois_elt(k, log_n), mfhe.galois_elt(-k, log_n)
            assert g == 5 ** k % m == gm.galois_elt(k, log_n)
            assert g * gi % m == 1 and gi == gm.galois_elt(-k, log_n)
            assert g & 1 and 1 <= g < m and 1 <= gi < m


def test_sigma_composes_and_keeps_products():
    """sigma_g sigma_h = sigma_(gh mod 2N), and sigma_g is a ring homomorphism of Z[X] / (X^N + 1)."""
    n, m = 16, 1 << 40
    rnd = __import__("random").Random(1)
    a = [rnd.randrange(m) for _ in range(n)]
    b = [rnd.randrange(m) for _ in range(n)]
    for g in (3, 5, 25, 31):
        for h in (5, 13, 31):
            assert [v % m for v in gm.sigma(gm.sigma(a, h), g)] == [v % m for v in gm.sigma(a, g * h % 32)]
        lhs = [v % m for v in gm.sigma(km.negacyclic(a, b, m), g)]
        assert lhs == km.negacyclic([v % m for v in gm.sigma(a, g)], [v % m for v in gm.sigma(b, g)], m)


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["45-49", "50-61"])
@pytest.mark.parametrize("g", gm.CASE_ELTS)
def test_hoisted_rotation_decrypts_within_the_bound_and_keeps_its_margin(bits, g):
    """|out0 + out1 s - sigma_g(c0 + c1 s)|_inf <= ks_model.error_bound: sigma_g of a FAST-raised digit is again a
    representative of sigma_g(c1) mod Q_j below alpha Q_j in absolute value, which is all the bound uses.  Every centred
    remainder of both ModDowns stays at least 2^-30 P away from +-P/2 (the library's documented window is 2^-40), so
    tests/test_galois_gpu.py may demand exact equality on these seeded cases.  The hoisted result differs from the
    naive one (sigma_g first, then the key switch) although both obey the bound."""
    cs = gm.seeded_case(bits, g)
    q, p, alpha, n, s = cs["q"], cs["p"], cs["alpha"], cs["n"], cs["s"]
    assert all(abs(v) <= 1 for v in s)
    for level in km.CASE_LEVELS:
        c0, c1 = cs["ct"][level]
        Ql = km.prod(q[:level])
        out0, out1, margin = gm.rotate(q, p, alpha, level, c0, c1, cs["key"], g)
        err = gm.rotation_error(q, level, out0, out1, c0, c1, s, g)
        bound = km.error_bound(q, p, alpha, level, n, km.B_E)
        print(f"bits {bits} g {g} level {level}: error {err}, bound {bound:.2f}, margin {margin:.3e} P")
        assert bound < Ql // 4
        assert err <= bound, (level, err, bound)
        assert margin >= 2.0 ** -30, "pick another seed: a ModDown remainder sits at +-P/2"
        k0, k1, _ = km.keyswitch(q, p, alpha, level, [v % Ql for v in gm.sigma(c1, g)], cs["key"])
        naive0 = [(a + b) % Ql for a, b in zip(gm.sigma(c0, g), k0)]
        assert (naive0, k1) != (out0, out1), "hoisted and naive agree bit for bit: not expected"
        assert gm.rotation_error(q, level, naive0, k1, c0, c1, s, g) <= bound


def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return cc
    llvm = Path("/opt/rocm/lib/llvm/bin/clang++")
    return str(llvm) if llvm.exists() else None


@pytest.fixture(scope="module")
def perm_prog(tmp_path_factory):
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("galois") / "galois_perm_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "galois_perm_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("log_n", list(range(1, 18)))
def test_index_function_matches_the_model_under_sanitizers(perm_prog, log_n):
    m = 2 << log_n
    for g in sorted({1, 3 % m, 5 % m, pow(5, 1000, m), m - 3 if m > 4 else 1, m - 1}):
        r = subprocess.run([str(perm_prog), str(log_n), str(g)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
        assert [int(v) for v in r.stdout.split()] == gm.perm(log_n, g), (log_n, g)


def test_perm_prog_rejects_bad_input(perm_prog):
    assert subprocess.run([str(perm_prog), "4", "6"], capture_output=True).returncode == 3    # even
    assert subprocess.run([str(perm_prog), "4", "33"], capture_output=True).returncode == 3   # >= 2N
    assert subprocess.run([str(perm_prog), "0", "1"], capture_output=True).returncode == 3
