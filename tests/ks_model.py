"""Test helper (not a test): hybrid key switching in Python integers, in the coefficient domain, with the negacyclic
schoolbook product.  It is the yardstick of tests/test_keyswitch_cpu.py and tests/test_keyswitch_gpu.py.

Notation (include/mfhe.h): Q limbs q_0 .. q_(key_level-1), K special primes with product P, digits of alpha
consecutive Q limbs (digit j at `level` = limbs [j alpha, min((j+1) alpha, level)), product Q_j).  A polynomial is a
list of N Python integers.

  key        : k_j = (e_j - a_j s_to + F_j s_from, a_j) mod Q_keylevel P, with F_j = P mod q_r for the limbs r of digit
               j and 0 mod every other prime of the key (the special ones included)
  raise      : d~_j = sum_i y_i (Q_j / q_i), y_i = [c_i (Q_j / q_i)^-1]_(q_i): the FAST formula, 0 <= d~_j < alpha Q_j
  inner      : acc_c = sum_j d~_j k_j,c mod Q_level P
  ModDown    : r = centred remainder of acc mod P, out = (acc - r) / P mod Q_level = round(acc / P)
"""
import random

from primes import primes_of_size


def prod(xs):
    r = 1
    for x in xs:
        r *= int(x)
    return r


def centered(x, m):
    """The representative of x mod m in (-m/2, m/2]."""
    x %= m
    return x - m if x > m // 2 else x


def negacyclic(a, b, m):
    """a b mod (X^N + 1, m), schoolbook."""
    n = len(a)
    out = [0] * n
    for i, ai in enumerate(a):
        if ai == 0:
            continue
        for j, bj in enumerate(b):
            k = i + j
            if k < n:
                out[k] += ai * bj
            else:
                out[k - n] -= ai * bj
    return [v % m for v in out]


def digits(level, alpha):
    """[(first limb, count)] of the digits at `level`; the last may be partial."""
    return [(s, min(alpha, level - s)) for s in range(0, level, alpha)]


def key_factor(q, p, alpha, j):
    """F_j mod Q P for a key over the Q limbs q (key_level of them) and the special primes p."""
    P, M = prod(p), prod(q) * prod(p)
    s, n = digits(len(q), alpha)[j]
    Qj = prod(q[s:s + n])
    rest = M // Qj                       # every other prime of the key, the special ones included
    return (P % Qj) * rest * pow(rest, -1, Qj) % M


def assemble(q, p, alpha, s_from, s_to, a, e):
    """[(k_j0, k_j1)] mod Q P from integer polynomials s_from, s_to, a_j (mod Q P) and e_j (small)."""
    M = prod(q) * prod(p)
    key = []
    for j, (aj, ej) in enumerate(zip(a, e)):
        F = key_factor(q, p, alpha, j)
        as_ = negacyclic(aj, s_to, M)
        b = [(ev - av + F * sv) % M for ev, av, sv in zip(ej, as_, s_from)]
        key.append((b, [v % M for v in aj]))
    return key


def raise_digit(c, q, start, count):
    """FAST raise of the digit [start, start + count) of c (integer coefficients, any representative mod Q)."""
    src = q[start:start + count]
    S = prod(src)
    out = [0] * len(c)
    for s in src:
        m = S // s
        inv = pow(m, -1, s)
        for k, v in enumerate(c):
            out[k] += (v % s) * inv % s * m
    return out


def inner_product(raised, key, m):
    """(acc_0, acc_1) = sum_j raised_j key_j mod m."""
    n = len(raised[0])
    acc = [[0] * n, [0] * n]
    for d, kj in zip(raised, key):
        for c in range(2):
            t = negacyclic(d, [v % m for v in kj[c]], m)
            acc[c] = [(x + y) % m for x, y in zip(acc[c], t)]
    return acc


def moddown(x, P, Ql):
    """round(x / P) mod Ql per coefficient, and the smallest distance of a centred remainder from +-P/2 as a fraction
    of P."""
    out, margin = [], 1.0
    for v in x:
        r = centered(v, P)
        out.append(((v - r) // P) % Ql)
        margin = min(margin, (P // 2 - abs(r)) / P)
    return out, margin


def keyswitch(q, p, alpha, level, c, key):
    """(k_0, k_1, margin) of the switch of c (mod Q_level) with a key made over all of q."""
    Ql, P = prod(q[:level]), prod(p)
    raised = [raise_digit(c, q, s, n) for s, n in digits(level, alpha)]
    acc = inner_product(raised, key, Ql * P)
    k0, m0 = moddown(acc[0], P, Ql)
    k1, m1 = moddown(acc[1], P, Ql)
    return k0, k1, min(m0, m1)


def decryption_error(q, level, k0, k1, c, s_from, s_to):
    """max |k_0 + k_1 s_to - c s_from| over the coefficients, centred mod Q_level."""
    Ql = prod(q[:level])
    lhs = negacyclic(k1, s_to, Ql)
    rhs = negacyclic(c, s_from, Ql)
    return max(abs(centered(a + b - d, Ql)) for a, b, d in zip(k0, lhs, rhs))


def error_bound(q, p, alpha, level, n, b_e):
    """(N + 1)/2 + 1 + beta alpha N B_e max_j Q_j / P: the rounding of two ModDowns times (1 + N |s|_inf) for ternary
    s_to, and the raised digits |d~_j| < alpha Q_j against the noise."""
    dg = digits(level, alpha)
    qmax = max(prod(q[s:s + c]) for s, c in dg)
    return (n + 1) / 2 + 1 + len(dg) * alpha * n * b_e * qmax / prod(p)


B_E = 19          # |e| <= 6 sigma rounded, sigma = 3.2
CASE_N = 16
CASE_ALPHA = 2
CASE_LEVELS = (5, 3, 2)
PRIME_CLASSES = ((45, 49), (50, 61))


def case_moduli(bits):
    """5 Q primes and 2 special primes of the given bit sizes with q = 1 mod 2N, N = 16."""
    return primes_of_size(bits[0], 2 * CASE_N, 5), primes_of_size(bits[1], 2 * CASE_N, 2)


def seeded_case(bits=(45, 49), kind="switch", noise=True, seed=2024):
    """The seeded inputs the CPU and GPU tests share: ternary s_to, s_from another ternary secret (kind "switch") or
    s_to^2 (kind "relin"), a_j uniform mod Q P, |e_j| <= B_E (0 without noise), and per level a uniform c mod Q_level."""
    q, p = case_moduli(bits)
    n, alpha = CASE_N, CASE_ALPHA
    rnd = random.Random(f"{seed}-{bits}-{kind}-{noise}")
    M = prod(q) * prod(p)
    s_to = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    if kind == "relin":
        s_from = [centered(v, M) for v in negacyclic(s_to, s_to, M)]
    else:
        s_from = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    beta = len(digits(len(q), alpha))
    a = [[rnd.randrange(M) for _ in range(n)] for _ in range(beta)]
    e = [[rnd.randint(-B_E, B_E) if noise else 0 for _ in range(n)] for _ in range(beta)]
    c = {lv: [rnd.randrange(prod(q[:lv])) for _ in range(n)] for lv in CASE_LEVELS}
    return {"q": q, "p": p, "alpha": alpha, "n": n, "s_from": s_from, "s_to": s_to, "a": a, "e": e, "c": c,
            "key": assemble(q, p, alpha, s_from, s_to, a, e)}
