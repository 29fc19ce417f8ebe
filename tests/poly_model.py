"""Test helper (not a test): the node list of a polynomial evaluation plan (csrc/poly_plan.hpp, include/mfhe.h
mfhe_poly_plan_*) interpreted in Python, and the error it may make, propagated through the nodes in the slot domain.

A plan here is a dict: basis, degree, level, in_scale, out_scale, out_reg, out_level, moduli (limbs [0, level)), consts
(Python integers) and nodes, each a dict dst, level, mul_a, mul_b, k_mul, terms [(src, k, coef)], addend_k, addend_coef,
scale_in, scale_out: what tests/cpp/poly_plan_main.cpp prints and what mfhe.PolyPlan exports (from_handle).

Every register j holds a ciphertext whose decryption is w_j D_j, D_j its tracked scale (a double, taken exactly) and
w_j what the plan says it holds up to an error e_j.  A node computes, with q = q_(level-1), S = scale_in, rho =
S / (q D_dst) (the tracked scale_out is the double nearest to S / q),
    w_dst = rho (k_mul (D_a D_b / S) w_a w_b + sum_j (k_j D_src / S) w_src + k_0 / S) + fresh,
against the intended a_mul W_a W_b + sum_j a_j W_src + a_0 (a_mul = k_mul, the a_j the real coefficients).  So with
c = rho k D / S the effective coefficient of a term,
    e_dst <= |c_mul - a_mul| |W_a W_b| + |c_mul| (e_a |W_b| + e_b |W_a| + e_a e_b + relin / (D_a D_b))
             + sum_j (|c_j - a_j| |W_src| + |c_j| e_src) + |rho k_0 / S - a_0| + rescale / D_dst.
The canonical embedding is a ring homomorphism, so this holds slot by slot with |.| the largest slot: nothing
compounds with N.  relin and rescale are the fresh slot errors in units of one integer coefficient's worth, N times
the coefficient bound: ks_model.error_bound per relinearisation, (1 + N) / 2 per rescale.  With exact rationals and no
fresh terms (tests/test_poly_plan_cpu.py) what is left is the sum of the constants' rounding terms, and the bound is
rigorous for the exact interpretation of the node list."""
from fractions import Fraction

import numpy as np

MONOMIAL, CHEBYSHEV = 0, 1


def from_handle(plan, moduli):
    """The dict of an mfhe.PolyPlan; moduli: the context's."""
    info = plan.info()
    return dict(basis=info.basis, degree=info.degree, level=info.level, in_scale=info.in_scale,
                out_scale=info.out_scale, out_reg=info.out_reg, out_level=info.out_level, nreg=info.nreg,
                nmul=info.nmul, depth=info.depth, moduli=[int(q) for q in moduli[:info.level]],
                consts=plan.constants(), nodes=plan.nodes())


def evaluate(coeffs, basis, x):
    """p(x) for numpy arrays (float or complex) or Fractions: Horner, or the Chebyshev recurrence."""
    if basis == MONOMIAL:
        acc = 0 * x
        for a in reversed(coeffs):
            acc = acc * x + a
        return acc
    t0, t1 = 0 * x + 1, x
    acc = coeffs[0] * t0
    for a in coeffs[1:]:
        acc = acc + a * t1
        t0, t1 = t1, 2 * x * t1 - t0
    return acc


def _mag(v):
    return float(np.abs(v).max()) if isinstance(v, np.ndarray) else abs(v)


def propagate(plan, x, e_in=0, relin=None, rescale=0):
    """(W_out, e_out): the value the plan intends for its result at x (a numpy array of slots, or a Fraction) and the
    bound of the docstring on what the node list makes of it.  e_in: the error of the input; relin: {level: fresh slot
    error of a relinearisation at that level, in integer units}; rescale: the same for a rescale.  With a Fraction x
    everything is exact."""
    exact = isinstance(x, Fraction)
    num = (lambda v: Fraction(v)) if exact else (lambda v: float(Fraction(v)))
    F = Fraction
    D = {0: F(plan["in_scale"])}
    W = {0: x}
    E = {0: num(e_in)}
    for n in plan["nodes"]:
        S, q, Dd = F(n["scale_in"]), plan["moduli"][n["level"] - 1], F(n["scale_out"])
        rho = S / (q * Dd)
        w, e = 0 * x, num(0)
        if n["mul_a"] >= 0:
            a, b = n["mul_a"], n["mul_b"]
            am = plan["consts"][n["k_mul"]]
            c = rho * am * D[a] * D[b] / S
            w = am * W[a] * W[b]
            fresh = F(relin[n["level"]]) / (D[a] * D[b]) if relin else 0
            e += num(abs(c - am)) * _mag(W[a] * W[b])
            e += num(abs(c)) * (E[a] * _mag(W[b]) + E[b] * _mag(W[a]) + E[a] * E[b] + num(fresh))
        for src, k, coef in n["terms"]:
            c = rho * plan["consts"][k] * D[src] / S
            w = w + num(coef) * W[src]
            e += num(abs(c - F(coef))) * _mag(W[src]) + num(abs(c)) * E[src]
        if n["addend_k"] >= 0:
            w = w + num(n["addend_coef"])
            e += num(abs(rho * plan["consts"][n["addend_k"]] / S - F(n["addend_coef"])))
        e += num(F(rescale) / Dd)
        D[n["dst"]], W[n["dst"]], E[n["dst"]] = Dd, w, e
    r = plan["out_reg"]
    return W[r], E[r]


def interpret_exact(plan, x):
    """The node list on exact rationals at the Fraction x: each register a value times its scale, the rescale a
    division by q without rounding; returns the result divided by the tracked out_scale."""
    V = {0: x * Fraction(plan["in_scale"])}
    for n in plan["nodes"]:
        y = Fraction(0)
        if n["mul_a"] >= 0:
            y += plan["consts"][n["k_mul"]] * V[n["mul_a"]] * V[n["mul_b"]]
        for src, k, _ in n["terms"]:
            y += plan["consts"][k] * V[src]
        if n["addend_k"] >= 0:
            y += plan["consts"][n["addend_k"]]
        V[n["dst"]] = y / plan["moduli"][n["level"] - 1]
    return V[plan["out_reg"]] / Fraction(plan["out_scale"])


def coefficient_arithmetic(coeffs, basis):
    """What the planner's own arithmetic on the coefficients may move p(x) by for |T_i(x)| <= 1: none in the monomial
    basis (quotient and remainder are copies); in the Chebyshev basis every remainder coefficient is one rounded
    difference per split (at most 4 splits deep, a quotient's coefficients doubled at each), so 2^-53 16 sum |a_i|."""
    return 0.0 if basis == MONOMIAL else 2.0 ** -53 * 16 * sum(abs(a) for a in coeffs)


def predicted_products(coeffs, basis):
    """The product count the planner's rule predicts, restated: the powers read (each from ceil(j / 2) and
    floor(j / 2), down to 1) plus one product per giant step whose quotient is not a constant."""
    c = list(coeffs)

    def deg(v):
        d = len(v) - 1
        while d > 0 and v[d] == 0:
            d -= 1
        return d

    d = deg(c)
    e = 0
    while (1 << e) < d + 1:
        e += 1
    m = 1 << ((e + 1) // 2)
    powers, steps = set(), [0]

    def need(j):
        if j > 1 and j not in powers:
            powers.add(j)
            need((j + 1) // 2)
            need(j // 2)

    def walk(v):
        dv = deg(v)
        if dv == 0:
            return False            # a constant
        if dv < m:
            for j in range(1, dv + 1):
                if v[j] != 0:
                    need(j)
            return True
        g = m
        while 2 * g <= dv:
            g *= 2
        q, r = [0.0] * (dv - g + 1), list(v[:g])
        if basis == MONOMIAL:
            q = list(v[g:dv + 1])
        else:
            q[0] = v[g]
            for i in range(g + 1, dv + 1):
                q[i - g] = 2.0 * v[i]
                r[2 * g - i] -= v[i]
        if walk(q):
            steps[0] += 1
        walk(r)
        need(g)
        return True

    walk(c)
    return len(powers) + steps[0]
