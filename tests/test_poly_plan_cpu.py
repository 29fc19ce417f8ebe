"""CPU checks of csrc/poly_plan.hpp, the host planner of encrypted polynomial evaluation: tests/cpp/poly_plan_main.cpp,
which includes that header alone, is built with the host compiler under the address and undefined-behaviour sanitizers,
run once, and every plan it prints (both bases at degrees 1, 2, 3, 4, 7, 8, 15, 16, 31, 63, 127, and a degree-15 case
whose upper half is zero) is checked here: register discipline, term counts, depth, product count, every constant
against its exact rational, the residues, and the node list interpreted on exact rationals against p(x)."""
import math
import random
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import pytest

import poly_model as pm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"
DEGREES = [1, 2, 3, 4, 7, 8, 15, 16, 31, 63, 127]


def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return cc
    llvm = Path("/opt/rocm/lib/llvm/bin/clang++")
    return str(llvm) if llvm.exists() else None


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    """(plans by id, rejections by name) from the program's one run."""
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("poly_plan") / "poly_plan_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "poly_plan_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    plans, rejects = {}, {}
    fh = float.fromhex
    for ln in r.stdout.splitlines():
        kind, *f = ln.split()
        if kind == "reject":
            rejects[f[0]] = int(f[1])
            continue
        assert kind in ("plan", "mod", "coef", "node", "const", "res"), ln
        pid = int(f[0])
        if kind == "plan":
            basis, degree, level = int(f[1]), int(f[2]), int(f[3])
            nnodes, nreg, nk, nmul, depth, out_reg, out_level = (int(v) for v in f[5:12])
            plans[pid] = dict(basis=basis, degree=degree, level=level, in_scale=fh(f[4]), nnodes=nnodes, nreg=nreg,
                              nk=nk, nmul=nmul, depth=depth, out_reg=out_reg, out_level=out_level,
                              out_scale=fh(f[12]), nodes=[], consts=[], residues=[])
        elif kind == "mod":
            plans[pid]["moduli"] = [int(v) for v in f[1:]]
        elif kind == "coef":
            plans[pid]["coeffs"] = [fh(v) for v in f[1:]]
        elif kind == "node":
            assert int(f[1]) == len(plans[pid]["nodes"])
            dst, level, mul_a, mul_b, k_mul, addend_k = (int(v) for v in f[2:8])
            nt = int(f[11])
            terms = [(int(f[12 + 3 * j]), int(f[13 + 3 * j]), fh(f[14 + 3 * j])) for j in range(nt)]
            assert len(f) == 12 + 3 * nt
            plans[pid]["nodes"].append(dict(dst=dst, level=level, mul_a=mul_a, mul_b=mul_b, k_mul=k_mul, terms=terms,
                                            addend_k=addend_k, addend_coef=fh(f[8]), scale_in=fh(f[9]),
                                            scale_out=fh(f[10])))
        elif kind == "const":
            assert int(f[1]) == len(plans[pid]["consts"])
            v = (int(f[3]) << 64) | int(f[4])
            plans[pid]["consts"].append(-v if int(f[2]) else v)
        else:
            assert int(f[1]) == len(plans[pid]["residues"])
            plans[pid]["residues"].append([int(v) for v in f[2:]])
    for p in plans.values():
        assert len(p["nodes"]) == p["nnodes"] and len(p["consts"]) == p["nk"] == len(p["residues"])
    return plans, rejects


def test_the_header_includes_the_standard_library_alone():
    text = (CSRC / "poly_plan.hpp").read_text()
    assert "#include <hip" not in text and '#include "' not in text


def test_the_cases_are_the_ones_asked_for(output):
    plans, _ = output
    got = [(p["basis"], p["degree"]) for _, p in sorted(plans.items())]
    assert got == [(b, d) for b in (0, 1) for d in DEGREES] + [(0, 15), (1, 15)]
    for pid, p in plans.items():
        assert len(p["coeffs"]) == p["degree"] + 1 and all(-1 <= a <= 1 for a in p["coeffs"])
        assert p["level"] == 10 and p["in_scale"] == 2.0 ** 45
    assert sum(a == 0 for p in plans.values() for a in p["coeffs"]) > 20, "some coefficients are exactly zero"
    for pid in (22, 23):
        assert plans[pid]["coeffs"][8:] == [0.0] * 8 and plans[pid]["coeffs"][7] != 0


def test_registers_levels_terms_and_depth(output):
    """Every register is written before it is read and never at a level below a reader's; a node's destination is none
    of its sources and never register 0; at most 64 terms; the result is the last node's; depth <= ceil(log2(d + 1)) + 1."""
    plans, _ = output
    for pid, p in plans.items():
        level_of = {0: p["level"]}
        for n in p["nodes"]:
            reads = [s for s, _, _ in n["terms"]] + ([n["mul_a"], n["mul_b"]] if n["mul_a"] >= 0 else [])
            assert reads, (pid, n)
            for r in reads:
                assert r in level_of, (pid, n, "read before it is written")
                assert level_of[r] >= n["level"], (pid, n, "a source below the node's level")
            assert n["level"] == min(level_of[r] for r in reads), (pid, n)
            assert n["dst"] not in reads and 0 < n["dst"] < p["nreg"], (pid, n)
            assert len(n["terms"]) + (n["mul_a"] >= 0) <= 64
            assert (n["mul_a"] >= 0) == (n["mul_b"] >= 0) == (n["k_mul"] >= 0)
            assert n["level"] >= 2
            level_of[n["dst"]] = n["level"] - 1
        assert p["nodes"][-1]["dst"] == p["out_reg"] and level_of[p["out_reg"]] == p["out_level"]
        assert p["depth"] == p["level"] - p["out_level"] <= math.ceil(math.log2(p["degree"] + 1)) + 1, pid
        assert p["nreg"] <= len(p["nodes"]) + 1
    # the stated degrees reach the bound where d + 1 is a power of two, and a zero upper half costs nothing
    assert [plans[i]["depth"] for i in range(11)] == [1, 2, 2, 4, 4, 5, 5, 6, 6, 7, 8]
    assert plans[22]["depth"] == plans[4]["depth"] and plans[23]["depth"] == plans[15]["depth"]


def test_product_count_is_the_rule_s(output):
    plans, _ = output
    for pid, p in plans.items():
        assert sum(n["mul_a"] >= 0 for n in p["nodes"]) == p["nmul"] == pm.predicted_products(p["coeffs"], p["basis"]), pid
    # monomial, no zero top coefficients in the way: Paterson-Stockmeyer's count is about 2 sqrt(d)
    assert plans[8]["nmul"] <= 12 and plans[10]["nmul"] <= 26


def test_scales_follow_the_node_form(output):
    """S = D_a D_b with a product (k_mul 1, or 2 in the Chebyshev powers), else in_scale q_(l-1); scale_out = S / q_(l-1),
    all as the doubles a C++ compiler computes."""
    plans, _ = output
    for pid, p in plans.items():
        D = {0: p["in_scale"]}
        for n in p["nodes"]:
            q = p["moduli"][n["level"] - 1]
            if n["mul_a"] >= 0:
                assert n["scale_in"] == D[n["mul_a"]] * D[n["mul_b"]]
                assert p["consts"][n["k_mul"]] in (1, 2)
            else:
                assert n["scale_in"] == p["in_scale"] * float(q)
            assert n["scale_out"] == n["scale_in"] / float(q)
            D[n["dst"]] = n["scale_out"]
        assert p["out_scale"] == D[p["out_reg"]]
        assert 0.99 < p["out_scale"] / p["in_scale"] < 1.01, "the result stays near the input's scale"


def test_every_constant_is_its_rational_rounded(output):
    """|k - a S / D| <= max(1, 2^-60 |k|) with a, S, D the printed doubles taken exactly (D = 1 for an addend); no
    constant is zero; the residues are k mod q_r."""
    plans, _ = output
    worst = Fraction(0)
    for pid, p in plans.items():
        D = {0: Fraction(p["in_scale"])}
        for n in p["nodes"]:
            S = Fraction(n["scale_in"])
            uses = [(k, Fraction(a) * S / D[src]) for src, k, a in n["terms"]]
            if n["addend_k"] >= 0:
                uses.append((n["addend_k"], Fraction(n["addend_coef"]) * S))
            for k, want in uses:
                kv = p["consts"][k]
                assert kv != 0
                err = abs(kv - want)
                assert err <= max(1, Fraction(abs(kv), 1 << 60)), (pid, n, kv, float(want))
                assert abs(kv) < 1 << 126
                if abs(kv) < 1 << 60:
                    worst = max(worst, err)
            D[n["dst"]] = Fraction(n["scale_out"])
        for kv, res in zip(p["consts"], p["residues"]):
            assert res == [kv % q for q in p["moduli"]], (pid, kv)
        assert len(set(p["consts"])) == len(p["consts"]), "constants are stored once"
    assert worst <= Fraction(1, 2) + Fraction(1, 1 << 40), "a constant below 2^60 is the nearest integer"


def test_the_node_list_evaluates_the_polynomial(output):
    """On exact rationals (each register a value times its scale, the rescale a division by q without rounding) the
    node list reproduces p(x) at 16 seeded points of [-1, 1] to within the sum of the constants' rounding terms
    (poly_model.propagate) and, in the Chebyshev basis, the planner's double arithmetic on the coefficients."""
    plans, _ = output
    rnd = random.Random(2718)
    xs = [Fraction(rnd.randrange(-(1 << 30), (1 << 30) + 1), 1 << 30) for _ in range(14)] + [Fraction(1), Fraction(-1)]
    for pid, p in plans.items():
        coeffs = [Fraction(a) for a in p["coeffs"]]
        slack = Fraction(pm.coefficient_arithmetic(p["coeffs"], p["basis"]))
        worst = Fraction(0)
        for x in xs:
            want = pm.evaluate(coeffs, p["basis"], x)
            intended, bound = pm.propagate(p, x)
            got = pm.interpret_exact(p, x)
            assert abs(intended - want) <= slack, (pid, float(x), float(intended - want))
            assert abs(got - intended) <= bound, (pid, float(x), float(got - intended), float(bound))
            assert bound < Fraction(1, 1 << 36), (pid, float(bound))
            worst = max(worst, abs(got - want))
        assert worst <= Fraction(1, 1 << 36)


def test_rejections(output):
    _, rej = output
    assert rej == {"degree-0": 11, "degree-128": 11, "basis": 12, "levels": 15, "levels-cheb": 15, "level-0": 15,
                   "nan-coefficient": 13, "inf-coefficient": 13, "nan-scale": 13, "inf-scale": 13, "zero-scale": 13,
                   "constant-too-large": 16, "constant-polynomial": 14}
