"""Test helper (not a test): the baby-step giant-step linear transform (include/mfhe.h mfhe_lt_baby_step,
mfhe_lt_pt_mac, mfhe_lt_apply) in Python integers, in the coefficient domain, built on tests/ks_model.py and
tests/galois_model.py.  It is the yardstick of tests/test_lintrans_cpu.py and tests/test_lintrans_gpu.py.

Notation: Q_l the product of the first `level` Q primes, P the product of the special primes, M = Q_l P.  A plan is
Galois elements of the baby steps (baby_elt, entry 0 is 1) and of the giant steps (giant_elt, entry 0 is 1) and, per
term t, its giant step term_giant[t] (non-decreasing) and baby step term_baby[t]; plaintext t (an integer polynomial)
belongs to term t.

  baby step b  : U_b = (sum_j sigma_g(d~_j) k_j,0 + P sigma_g(c0), sum_j sigma_g(d~_j) k_j,1) mod M, d~_j the FAST-raised
                 digits of c1, k_j the Galois key of g = baby_elt[b]; U_0 = (P c0, P c1).  No ModDown.
  giant step a : A_a = sum_{t in a} pt_t U_b(t) mod M (negacyclic products), (w0, w1) = ModDown_P(A_a),
                 a == 0: out += (w0, w1);  a != 0: out += the hoisted rotation of (w0, w1) by giant_elt[a]
                 (galois_model.rotate).

Error bound (error_bound below), derived from the terms of ks_model.error_bound, for a ternary secret s and
|pt_t|_inf <= B_pt.  Write m = c0 + c1 s mod Q_l.
  * A keyed baby step satisfies U_b,0 + U_b,1 s = P sigma_g(m) + E_b mod M with E_b = sum_j sigma_g(d~_j) e_j, and
    |d~_j| < alpha Q_j, so |E_b|_inf <= beta alpha N B_e max_j Q_j =: E.  This is the third term of
    ks_model.error_bound before its division by P.  The unrotated step has E_0 = 0.
  * A_a,0 + A_a,1 s = P sum_t pt_t sigma_g(m) + sum_t pt_t E_b(t): a negacyclic product with pt_t amplifies the
    infinity norm by at most N B_pt, so the noise is at most T_a N B_pt E with T_a the keyed terms of giant step a.
  * ModDown replaces A_c by (A_c - r_c) / P with |r_c| <= P / 2: w0 + w1 s is off by at most T_a N B_pt E / P from the
    division plus |r_0 + r_1 s| / P <= (1 + N) / 2 from the rounding: one ModDown rounding per giant step.
  * A giant rotation (a != 0) permutes and negates what it is given and adds its own ks_model.error_bound.
So |out0 + out1 s - sum_a sigma_G_a(sum_t pt_t sigma_g_b(t)(m))|_inf
     <= sum over the giant steps a that have terms of  T_a N B_pt E / P + (N + 1) / 2 + [a != 0] ks_model.error_bound.
"""
import random

import galois_model as gm
import ks_model as km


def baby_step(q, p, alpha, level, c0, c1, key, g):
    """U = (u0, u1) mod Q_l P; key None (g must be 1) is the unrotated term."""
    Ql, P = km.prod(q[:level]), km.prod(p)
    M = Ql * P
    if key is None:
        assert g == 1
        return [v * P % M for v in c0], [v * P % M for v in c1]
    raised = [gm.sigma(km.raise_digit(c1, q, s, n), g) for s, n in km.digits(level, alpha)]
    acc = km.inner_product(raised, key, M)
    u0 = [(a + P * b) % M for a, b in zip(acc[0], gm.sigma(c0, g))]
    return u0, acc[1]


def pt_mac(us, pts, M):
    """(A_0, A_1) = sum_t pts[t] us[t] mod M, us a list of (u0, u1)."""
    n = len(pts[0])
    acc = [[0] * n, [0] * n]
    for (u0, u1), pt in zip(us, pts):
        ptm = [v % M for v in pt]
        for c, u in enumerate((u0, u1)):
            acc[c] = [(x + y) % M for x, y in zip(acc[c], km.negacyclic(ptm, u, M))]
    return acc


def transform(q, p, alpha, level, c0, c1, plan, keys, pts):
    """(out0, out1, margin) mod Q_l.  keys: {Galois element: switching key from sigma_g(s) to s made over all of q};
    margin: the smallest distance of any ModDown remainder from +-P/2, as a fraction of P."""
    Ql, P = km.prod(q[:level]), km.prod(p)
    n = len(c0)
    U = {}
    for b in sorted(set(plan["term_baby"])):
        g = plan["baby_elt"][b]
        U[b] = baby_step(q, p, alpha, level, c0, c1, None if b == 0 else keys[g], g)
    out0, out1, margin = [0] * n, [0] * n, 1.0
    for a in sorted(set(plan["term_giant"])):
        ts = [t for t, ta in enumerate(plan["term_giant"]) if ta == a]
        A = pt_mac([U[plan["term_baby"][t]] for t in ts], [pts[t] for t in ts], Ql * P)
        w0, m0 = km.moddown(A[0], P, Ql)
        w1, m1 = km.moddown(A[1], P, Ql)
        margin = min(margin, m0, m1)
        if a != 0:
            g = plan["giant_elt"][a]
            w0, w1, m2 = gm.rotate(q, p, alpha, level, w0, w1, keys[g], g)
            margin = min(margin, m2)
        out0 = [(x + y) % Ql for x, y in zip(out0, w0)]
        out1 = [(x + y) % Ql for x, y in zip(out1, w1)]
    return out0, out1, margin


def expected_plain(q, level, c0, c1, s, plan, pts):
    """sum_a sigma_G_a(sum_{t in a} pt_t sigma_g_b(t)(c0 + c1 s)) mod Q_l: what the transform's output decrypts to, up
    to the error."""
    Ql = km.prod(q[:level])
    m = [(a + b) % Ql for a, b in zip(c0, km.negacyclic(c1, s, Ql))]
    total = [0] * len(c0)
    for a in sorted(set(plan["term_giant"])):
        inner = [0] * len(c0)
        for t, ta in enumerate(plan["term_giant"]):
            if ta != a:
                continue
            rot = [v % Ql for v in gm.sigma(m, plan["baby_elt"][plan["term_baby"][t]])]
            inner = [(x + y) % Ql for x, y in zip(inner, km.negacyclic([v % Ql for v in pts[t]], rot, Ql))]
        total = [(x + y) % Ql for x, y in zip(total, gm.sigma(inner, plan["giant_elt"][a]))]
    return [v % Ql for v in total]


def decryption_error(q, level, out0, out1, s, want):
    """max |out0 + out1 s - want| over the coefficients, centred mod Q_l."""
    Ql = km.prod(q[:level])
    got = [(a + b) % Ql for a, b in zip(out0, km.negacyclic(out1, s, Ql))]
    return max(abs(km.centered(a - b, Ql)) for a, b in zip(got, want))


def error_bound(q, p, alpha, level, n, b_e, b_pt, plan):
    """The bound derived in the module docstring."""
    dg = km.digits(level, alpha)
    qmax = max(km.prod(q[s:s + c]) for s, c in dg)
    e_over_p = len(dg) * alpha * n * b_e * qmax / km.prod(p)
    total = 0.0
    for a in sorted(set(plan["term_giant"])):
        keyed = sum(1 for t, ta in enumerate(plan["term_giant"]) if ta == a and plan["term_baby"][t] != 0)
        total += keyed * n * b_pt * e_over_p + (n + 1) / 2
        if a != 0:
            total += km.error_bound(q, p, alpha, level, n, b_e)
    return total


# N = 16 has 8 slots: n1 = 4 baby steps, n2 = 2 giant steps (a rotation by 4), the diagonal k = 6 missing
CASE_PLAN = {
    "steps": [0, 1, 2, 3, 4, 5, 7],
    "baby_elt": [gm.galois_elt(b, 4) for b in range(4)],
    "giant_elt": [1, gm.galois_elt(4, 4)],
    "term_giant": [0, 0, 0, 0, 1, 1, 1],
    "term_baby": [0, 1, 2, 3, 0, 1, 3],
}
B_PT = 1 << 20


def make_keys(q, p, alpha, n, s, elts, rnd):
    """{g: the parts of the Galois key of g for the secret s}: a_j uniform mod Q P, |e_j| <= B_E, s_from = sigma_g(s),
    s_to = s, and "key" = ks_model.assemble of them."""
    M = km.prod(q) * km.prod(p)
    beta = len(km.digits(len(q), alpha))
    keys = {}
    for g in elts:
        a = [[rnd.randrange(M) for _ in range(n)] for _ in range(beta)]
        e = [[rnd.randint(-km.B_E, km.B_E) for _ in range(n)] for _ in range(beta)]
        keys[g] = {"a": a, "e": e, "s_from": gm.sigma(s, g), "s_to": s,
                   "key": km.assemble(q, p, alpha, gm.sigma(s, g), s, a, e)}
    return keys


def seeded_case(bits=(45, 49), seed=2026):
    """The seeded inputs the CPU and GPU tests share (N = 16, ks_model's moduli, alpha and levels, CASE_PLAN): a ternary
    s, one Galois key per step in use ("keys" for transform, "key_parts" to assemble them elsewhere), plaintexts with
    |coefficients| <= B_PT and per level a uniform ciphertext."""
    q, p = km.case_moduli(bits)
    n, alpha = km.CASE_N, km.CASE_ALPHA
    rnd = random.Random(f"lintrans-{seed}-{bits}")
    s = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    elts = sorted({g for g in CASE_PLAN["baby_elt"] + CASE_PLAN["giant_elt"] if g != 1})
    parts = make_keys(q, p, alpha, n, s, elts, rnd)
    pts = [[rnd.randint(-B_PT, B_PT) for _ in range(n)] for _ in CASE_PLAN["term_giant"]]
    ct = {lv: ([rnd.randrange(km.prod(q[:lv])) for _ in range(n)], [rnd.randrange(km.prod(q[:lv])) for _ in range(n)])
          for lv in km.CASE_LEVELS}
    return {"q": q, "p": p, "alpha": alpha, "n": n, "s": s, "keys": {g: v["key"] for g, v in parts.items()},
            "key_parts": parts, "pts": pts, "ct": ct, "plan": CASE_PLAN}
