"""CPU checks of the linear-transform layer (include/mfhe.h mfhe_lt_baby_step .. mfhe_lt_apply): exported symbols, the
coefficient-domain model of tests/lt_model.py against its derived error bound and its margin from +-P/2, a slot-level
matrix-vector product through the model, mfhe.bsgs_plan against a hand-written plan, and csrc/lintrans.hpp's plan
validation in a stand-alone program built under the address and undefined-behaviour sanitizers.

Shape of the model cases: N = 16 (8 slots), 5 Q primes + 2 special primes, alpha 2, levels 5, 3 and 2, n1 = 4 baby and
n2 = 2 giant steps with the diagonal 6 missing, plaintext coefficients up to 2^20."""
import random
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import galois_model as gm
import ks_model as km
import lt_model as lm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"
NEW = ["mfhe_lt_baby_step", "mfhe_lt_pt_mac", "mfhe_lt_reserve", "mfhe_lt_apply"]


def test_new_symbols_declared_and_exported(mfhe):
    names = mfhe.declared_symbols()
    for n in NEW:
        assert n in names, n
        assert hasattr(mfhe.lib, n), n
        assert getattr(mfhe.lib, n).argtypes is not None, n   # a _sig entry exists
    for m in ("lt_baby_step", "lt_pt_mac", "lt_reserve", "lt_apply"):
        assert callable(getattr(mfhe.Context, m)), m
    assert callable(mfhe.bsgs_plan) and mfhe.LT_MAX_TERMS == 64


def test_null_context_is_einval(mfhe):
    lib = mfhe.lib
    assert lib.mfhe_lt_baby_step(None, 8, 1, 8, 1, 1, 8, 8, 1, 1, 1, 1, 1, 1, 1, 3, None) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()
    assert lib.mfhe_lt_pt_mac(None, 8, 1, 1, 1, 8, 1, 1, 1, 8, 1, None, None, 1, 1, 1, 1, 1, None) == mfhe.EINVAL
    assert lib.mfhe_lt_reserve(None, 1, 1, 1, 1, 1, 1, 1) == mfhe.EINVAL
    assert lib.mfhe_lt_apply(None, None, 8, 8, 1, 8, 1, 1, 8, 8, 1, 1, 1, 1, 1, 1, 1, None) == mfhe.EINVAL
    assert b"null ctx" in lib.mfhe_last_error()


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["45-49", "50-61"])
def test_transform_decrypts_within_the_derived_bound_and_keeps_its_margin(bits):
    """out0 + out1 s = sum_a sigma_G_a(sum_t pt_t sigma_g_b(c0 + c1 s)) within lt_model.error_bound, whose derivation is
    lt_model's docstring.  Every centred remainder of every ModDown (one per giant step and one per giant rotation)
    stays at least 2^-30 P away from +-P/2, so tests/test_lintrans_gpu.py may demand exact equality on these cases."""
    cs = lm.seeded_case(bits)
    q, p, alpha, n, s, plan = cs["q"], cs["p"], cs["alpha"], cs["n"], cs["s"], cs["plan"]
    assert all(abs(v) <= 1 for v in s)
    assert all(abs(v) <= lm.B_PT for pt in cs["pts"] for v in pt)
    assert plan["baby_elt"][0] == 1 and plan["giant_elt"][0] == 1
    for level in km.CASE_LEVELS:
        c0, c1 = cs["ct"][level]
        Ql = km.prod(q[:level])
        out0, out1, margin = lm.transform(q, p, alpha, level, c0, c1, plan, cs["keys"], cs["pts"])
        want = lm.expected_plain(q, level, c0, c1, s, plan, cs["pts"])
        err = lm.decryption_error(q, level, out0, out1, s, want)
        bound = lm.error_bound(q, p, alpha, level, n, km.B_E, lm.B_PT, plan)
        print(f"bits {bits} level {level}: error {err}, bound {bound:.2f}, margin {margin:.3e} P")
        assert bound < Ql // 4
        assert err <= bound, (level, err, bound)
        assert margin >= 2.0 ** -30, "pick another seed: a ModDown remainder sits at +-P/2"
        assert lm.decryption_error(q, level, c0, c1, s, want) > bound, "the transform did something"


def test_baby_step_is_the_rotation_before_its_moddown():
    """ModDown of a keyed baby step is galois_model.rotate: the baby step is the hoisted rotation left in Q u P."""
    cs = lm.seeded_case()
    q, p, alpha = cs["q"], cs["p"], cs["alpha"]
    P = km.prod(p)
    for level in km.CASE_LEVELS:
        c0, c1 = cs["ct"][level]
        Ql = km.prod(q[:level])
        for g in (5, 29):
            u0, u1 = lm.baby_step(q, p, alpha, level, c0, c1, cs["keys"][g], g)
            w0, w1, _ = gm.rotate(q, p, alpha, level, c0, c1, cs["keys"][g], g)
            assert km.moddown(u0, P, Ql)[0] == w0 and km.moddown(u1, P, Ql)[0] == w1
        u0, u1 = lm.baby_step(q, p, alpha, level, c0, c1, None, 1)
        assert km.moddown(u0, P, Ql)[0] == c0 and km.moddown(u1, P, Ql)[0] == c1


# ---------------------------------------------------------------------------------------------------------------
# slots: an 8 x 8 real matrix times an 8-vector
# ---------------------------------------------------------------------------------------------------------------
def _slot_roots(n):
    """zeta^(5^j), j < n / 2, zeta = e^(i pi / n): the points whose values are the slots, in rotation order."""
    return np.exp(1j * np.pi * np.array([pow(5, j, 2 * n) for j in range(n // 2)]) / n)


def _encode(z, n, scale):
    """The integer polynomial whose value at _slot_roots()[j] is about scale * z[j] (z real or complex)."""
    roots = _slot_roots(n)
    k = np.arange(n)
    coeff = (2.0 / n) * np.real((np.asarray(z, dtype=complex)[:, None] * roots[:, None] ** (-k[None, :])).sum(axis=0))
    return [int(round(float(v) * scale)) for v in coeff]


def _decode(poly, n, scale):
    roots = _slot_roots(n)
    k = np.arange(n)
    return (np.array([float(v) for v in poly])[None, :] * roots[:, None] ** k[None, :]).sum(axis=1) / scale


def test_matrix_times_vector_in_the_slots():
    """N = 16, level 3, 45 / 49-bit primes, scale 2^30 for the vector and for the diagonals: the model's transform of
    an encryption of v by the diagonals of M (diagonal k pre-rotated by minus its giant step) decodes to M @ v.
    Measured on this seeded case: max |got - M @ v| = 1.001e-07 (entries of M and v uniform in [-1, 1]); the assertion
    allows 16 times that."""
    measured = 1.001e-07
    n, level, scale, n1 = 16, 3, float(1 << 30), 4
    q, p = km.case_moduli((45, 49))
    alpha, Ql = km.CASE_ALPHA, km.prod(q[:level])
    rng = np.random.default_rng(8)
    rnd = random.Random("lintrans-slots")
    M = rng.uniform(-1, 1, (8, 8))
    v = rng.uniform(-1, 1, 8)
    steps = list(range(8))
    plan = {"baby_elt": [gm.galois_elt(b, 4) for b in range(n1)], "giant_elt": [1, gm.galois_elt(n1, 4)],
            "term_giant": [k // n1 for k in steps], "term_baby": [k % n1 for k in steps]}
    j = np.arange(8)
    pts = []
    for k in steps:
        diag = M[j, (j + k) % 8]                                   # diag_k[j] = M[j][j + k]
        pts.append(_encode(np.roll(diag, k - k % n1), n, scale))   # rotated by minus the giant step: d[j - a n1]
    s = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    elts = sorted({g for g in plan["baby_elt"] + plan["giant_elt"] if g != 1})
    keys = {g: kp["key"] for g, kp in lm.make_keys(q, p, alpha, n, s, elts, rnd).items()}
    m = _encode(v, n, scale)
    e = [rnd.randint(-km.B_E, km.B_E) for _ in range(n)]
    a = [rnd.randrange(Ql) for _ in range(n)]
    c0 = [(mv + ev - x) % Ql for mv, ev, x in zip(m, e, km.negacyclic(a, s, Ql))]
    np.testing.assert_allclose(_decode(m, n, scale).real, v, atol=1e-7)   # the encoder itself
    rot = _decode(gm.sigma(m, gm.galois_elt(1, 4)), n, scale).real
    np.testing.assert_allclose(rot, np.roll(v, -1), atol=1e-7)            # galois_elt(1) rotates the slots left by one
    out0, out1, margin = lm.transform(q, p, alpha, level, c0, a, plan, keys, pts)
    assert margin >= 2.0 ** -30
    dec = [km.centered(x + y, Ql) for x, y in zip(out0, km.negacyclic(out1, s, Ql))]
    got = _decode(dec, n, scale * scale)
    err = float(np.abs(got - M @ v).max())
    print(f"slot product: max error {err:.3e} (imaginary part {np.abs(got.imag).max():.3e})")
    assert err <= 16 * measured


# ---------------------------------------------------------------------------------------------------------------
# bsgs_plan
# ---------------------------------------------------------------------------------------------------------------
def test_bsgs_plan_equals_a_hand_written_plan(mfhe):
    pl = mfhe.bsgs_plan([0, 1, 2, 3, 4, 5, 7], 4, 4)
    assert pl == {
        "baby_steps": [0, 1, 2, 3], "giant_steps": [0, 4],
        "baby_elt": [1, 5, 25, 29], "giant_elt": [1, 17],
        "term_step": [0, 1, 2, 3, 4, 5, 7],
        "term_giant": [0, 0, 0, 0, 1, 1, 1], "term_baby": [0, 1, 2, 3, 0, 1, 3],
        "key_steps": [1, 2, 3, 4],
    }
    for name in ("baby_elt", "giant_elt", "term_giant", "term_baby"):
        assert pl[name] == lm.CASE_PLAN[name], name
    # negative and repeated steps fold mod N / 2; a sparse set uses only the steps it needs; log_n 16 elements
    pl = mfhe.bsgs_plan([-1, 32767, 9, 9, 40], 8, 16)
    assert pl["term_step"] == [9, 40, 32767]
    assert pl["baby_steps"] == [0, 1, 7] and pl["giant_steps"] == [0, 8, 40, 32760]
    assert pl["term_giant"] == [1, 2, 3] and pl["term_baby"] == [1, 0, 2]
    assert pl["baby_elt"] == [1, 5, pow(5, 7, 1 << 17)] and pl["giant_elt"][3] == pow(5, 32760, 1 << 17)
    assert pl["key_steps"] == [1, 7, 8, 40, 32760]
    assert mfhe.bsgs_plan([], 4, 4)["term_step"] == [] and mfhe.bsgs_plan([0], 1, 4)["key_steps"] == []
    with pytest.raises(ValueError):
        mfhe.bsgs_plan([1], 0, 4)


# ---------------------------------------------------------------------------------------------------------------
# the plan validation of csrc/lintrans.hpp, stand-alone under sanitizers
# ---------------------------------------------------------------------------------------------------------------
def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return cc
    llvm = Path("/opt/rocm/lib/llvm/bin/clang++")
    return str(llvm) if llvm.exists() else None


@pytest.fixture(scope="module")
def plan_prog(tmp_path_factory):
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("lintrans") / "lt_plan_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "lt_plan_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _csv(xs):
    return ",".join(str(x) for x in xs) if len(xs) else "-"


def _run_plan(prog, n, baby, giant, kb, kg, tg, tb):
    args = [x if isinstance(x, str) else _csv(x) for x in (baby, giant, kb, kg, tg, tb)]
    r = subprocess.run([str(prog), str(n)] + args, capture_output=True, text=True)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return r


def test_valid_plans_are_grouped_by_giant_step(plan_prog):
    pl = lm.CASE_PLAN
    r = _run_plan(plan_prog, 16, pl["baby_elt"], pl["giant_elt"], [0, 1, 1, 1], [0, 1], pl["term_giant"], pl["term_baby"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:3] == ["group 0 0 4", "group 1 4 3", "used 0 1 2 3"]
    # a giant step without terms, a baby step nobody uses (its key may be null), keys of step 0 ignored
    r = _run_plan(plan_prog, 16, [1, 5, 25], [1, 3, 17], [0, 0, 1], [0, 0, 1], [0, 2, 2], [0, 2, 0])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:3] == ["group 0 0 1", "group 2 1 2", "used 0 2"]
    # 64 terms in each of two giant steps, one baby step; element 2N - 1
    r = _run_plan(plan_prog, 16, [1], [1, 31], [0], [0, 1], [0] * 64 + [1] * 64, [0] * 128)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:3] == ["group 0 0 64", "group 1 64 64", "used 0"]
    # only a later giant step has terms
    r = _run_plan(plan_prog, 1 << 16, [1, 5], [1, 25], [0, 1], [0, 1], [1], [1])
    assert r.returncode == 0 and r.stdout.split("\n")[:2] == ["group 1 0 1", "used 1"]


# (reason, exit status, N, baby_elt, giant_elt, baby keys, giant keys, term_giant, term_baby)
REJECTED = [
    ("null plan", 10, 16, "noplan", "-", "-", "-", "-", "-"),
    ("null baby_elt", 10, 16, "null:2", [1, 3], [0, 1], [0, 1], [0, 1], [0, 1]),
    ("null giant keys", 10, 16, [1, 5], [1, 3], [0, 1], "null:2", [0, 1], [0, 1]),
    ("null term_baby", 10, 16, [1, 5], [1, 3], [0, 1], [0, 1], "null:2", "null:2"),
    ("no terms", 11, 16, [1, 5], [1, 3], [0, 1], [0, 1], [], []),
    ("no baby steps", 11, 16, [], [1, 3], [], [0, 1], [0], [0]),
    ("no giant steps", 11, 16, [1], [], [0], [], [0], [0]),
    ("baby_elt[0] != 1", 12, 16, [5, 1], [1, 3], [0, 1], [0, 1], [0, 1], [0, 1]),
    ("giant_elt[0] != 1", 13, 16, [1, 5], [3, 1], [0, 1], [0, 1], [0, 1], [0, 1]),
    ("even baby element", 14, 16, [1, 6], [1, 3], [0, 1], [0, 1], [0, 1], [0, 1]),
    ("giant element 2N + 1", 14, 16, [1, 5], [1, 33], [0, 1], [0, 1], [0, 1], [0, 1]),
    ("negative element", 14, 16, [1, -5], [1, 3], [0, 1], [0, 1], [0, 1], [0, 1]),
    ("element of an unused step", 14, 16, [1, 5, 4], [1, 3], [0, 1, 1], [0, 1], [0, 1], [0, 1]),
    ("term_baby == n_baby", 15, 16, [1, 5], [1, 3], [0, 1], [0, 1], [0, 1], [0, 2]),
    ("term_giant == n_giant", 15, 16, [1, 5], [1, 3], [0, 1], [0, 1], [0, 2], [0, 1]),
    ("negative term_baby", 15, 16, [1, 5], [1, 3], [0, 1], [0, 1], [0, 1], [-1, 1]),
    ("term_giant decreases", 16, 16, [1, 5], [1, 3], [0, 1], [0, 1], [0, 1, 0], [0, 1, 1]),
    ("65 terms in one giant step", 17, 16, [1, 5], [1, 3], [0, 1], [0, 1], [0] * 65, [0] * 65),
    ("65 terms in the second giant step", 17, 16, [1, 5], [1, 3], [0, 1], [0, 1], [0] + [1] * 65, [0] * 66),
    ("used baby step without a key", 18, 16, [1, 5], [1, 3], [0, 0], [0, 1], [0, 1], [0, 1]),
    ("used giant step without a key", 18, 16, [1, 5], [1, 3], [0, 1], [0, 0], [0, 1], [0, 1]),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_rejected_plans_exit_with_their_reason(plan_prog, case):
    name, status, n, *lists = case
    r = _run_plan(plan_prog, n, *lists)
    assert r.returncode == status, (name, r.returncode, r.stderr[-500:])
    assert r.stdout == ""


def test_rejection_reasons_are_distinct():
    assert sorted({c[1] for c in REJECTED}) == list(range(10, 19))
