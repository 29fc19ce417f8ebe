"""Test helper (not a test): Galois automorphisms and the hoisted rotation in Python integers, built on
tests/ks_model.py.  It is the yardstick of tests/test_galois_cpu.py and tests/test_galois_gpu.py.

  sigma(a, g)  : a(X) -> a(X^g) mod X^N + 1 in the coefficient domain: coefficient i moves to i g mod 2N, negated when
                 that index is >= N
  perm(log_n,g): the same map in the evaluation domain.  Slot i of a phantom-convention transform holds
                 a(psi^(2 brev(i) + 1)), so sigma_g(a) has in slot i what a has in slot
                 pi_g(i) = brev(((2 brev(i) + 1) g mod 2N - 1) / 2)
  rotate       : the hoisted rotation of a ciphertext (c0, c1): raise the digits of c1 (the FAST formula), apply sigma_g
                 to each raised digit, inner product with the Galois key, ModDown, add sigma_g(c0)
"""
import random

import ks_model as km


def brev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def sigma(a, g):
    """a(X^g) mod X^N + 1 for an odd g; integer coefficients stay integers (some negated)."""
    n = len(a)
    out = [0] * n
    for i, v in enumerate(a):
        k = i * g % (2 * n)
        if k < n:
            out[k] = v
        else:
            out[k - n] = -v
    return out


def perm(log_n, g):
    """[pi_g(i)]: slot i of the transform of sigma_g(a) is slot pi_g(i) of the transform of a."""
    n = 1 << log_n
    return [brev(((2 * brev(i, log_n) + 1) * g % (2 * n) - 1) // 2, log_n) for i in range(n)]


def galois_elt(step, log_n):
    m = 2 << log_n
    return pow(5, step, m) if step >= 0 else pow(pow(5, -1, m), -step, m)


def rotate(q, p, alpha, level, c0, c1, key, g):
    """(out0, out1, margin) of the hoisted rotation of (c0, c1) mod Q_level with `key` a switching key from
    sigma_g(s) to s made over all of q: out0 = sigma_g(c0) + k0, out1 = k1."""
    Ql, P = km.prod(q[:level]), km.prod(p)
    raised = [sigma(km.raise_digit(c1, q, s, n), g) for s, n in km.digits(level, alpha)]
    acc = km.inner_product(raised, key, Ql * P)
    k0, m0 = km.moddown(acc[0], P, Ql)
    k1, m1 = km.moddown(acc[1], P, Ql)
    out0 = [(a + b) % Ql for a, b in zip(sigma(c0, g), k0)]
    return out0, k1, min(m0, m1)


def rotation_error(q, level, out0, out1, c0, c1, s, g):
    """max |out0 + out1 s - sigma_g(c0 + c1 s)| over the coefficients, centred mod Q_level."""
    Ql = km.prod(q[:level])
    got = [(a + b) % Ql for a, b in zip(out0, km.negacyclic(out1, s, Ql))]
    dec = [(a + b) % Ql for a, b in zip(c0, km.negacyclic(c1, s, Ql))]
    want = sigma(dec, g)
    return max(abs(km.centered(a - b, Ql)) for a, b in zip(got, want))


CASE_ELTS = (5, 25, 3, 13, 31)


def seeded_case(bits=(45, 49), g=5, seed=2025):
    """The seeded inputs the CPU and GPU tests share (N = 16, ks_model's moduli, alpha and levels): a ternary s, the
    Galois key of g (from sigma_g(s) to s, a_j uniform mod Q P, |e_j| <= B_E) and per level a uniform ciphertext
    (c0, c1) mod Q_level."""
    q, p = km.case_moduli(bits)
    n, alpha = km.CASE_N, km.CASE_ALPHA
    rnd = random.Random(f"galois-{seed}-{bits}-{g}")
    M = km.prod(q) * km.prod(p)
    s = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    s_from = sigma(s, g)
    beta = len(km.digits(len(q), alpha))
    a = [[rnd.randrange(M) for _ in range(n)] for _ in range(beta)]
    e = [[rnd.randint(-km.B_E, km.B_E) for _ in range(n)] for _ in range(beta)]
    ct = {lv: ([rnd.randrange(km.prod(q[:lv])) for _ in range(n)], [rnd.randrange(km.prod(q[:lv])) for _ in range(n)])
          for lv in km.CASE_LEVELS}
    return {"q": q, "p": p, "alpha": alpha, "n": n, "g": g, "s": s, "s_from": s_from, "s_to": s, "a": a, "e": e,
            "ct": ct, "key": km.assemble(q, p, alpha, s_from, s, a, e)}
