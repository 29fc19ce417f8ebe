"""Test helper (not a test): the product of ciphertexts in Python integers, in the coefficient domain, on top of
tests/ks_model.py.  It is the yardstick of tests/test_ctmul_cpu.py and tests/test_ctmul_gpu.py.

A ciphertext is a pair (c0, c1) of integer polynomials mod Q_level that decrypts as c0 + c1 s.  A product is a sum over
T pairs of ciphertexts, relinearised once:

  tensor   : d0 = sum_t a0 b0, d1 = sum_t (a0 b1 + a1 b0), d2 = sum_t a1 b1 mod (X^N + 1, Q_level), by km.negacyclic;
             the square form is b = a
  relin    : (k0, k1) = km.keyswitch(d2) with a key from s^2 to s (km.seeded_case(bits, "relin")),
             r0 = d0 + k0, r1 = d1 + k1 mod Q_level
  rescale  : rho_i = centred remainder of r_i mod q_(level-1), out_i = (r_i - rho_i) / q_(level-1) mod Q_(level-1)
             (km.moddown with P = q_(level-1))

The bound.  Let D = d0 + d1 s + d2 s^2 mod Q_level, the exact degree-2 decryption (s^2 = s_from of the key).
Without rescale, r0 + r1 s - D = k0 + k1 s - d2 s^2, the key switch's own error, so
  |r0 + r1 s - D|_inf <= km.error_bound(q, p, alpha, level, n, B_E)                        centred mod Q_level.
With rescale, write q = q_(level-1) and r0 + r1 s = D + e + k Q_level with |e| <= that bound.  Then
  out0 + out1 s = (r0 + r1 s) / q - (rho0 + rho1 s) / q = D / q + e / q + k Q_(level-1) - (rho0 + rho1 s) / q,
and |rho_i| <= q / 2, |s|_inf <= 1, so |(rho0 + rho1 s) / q|_inf <= 1/2 + N/2:
  |out0 + out1 s - D / q|_inf <= km.error_bound(...) / q + (N + 1) / 2                     centred mod Q_(level-1).
The checks multiply through by q, so they stay in integers: |q (out0 + out1 s) - D| <= bound + q (N + 1) / 2 centred
mod Q_level.

The margin returned is the smallest distance of any centred remainder from +- half of its modulus (P for the two
ModDowns of the key switch, q_(level-1) for the two rescales), as a fraction of that modulus, as km.moddown reports
it: the library may differ from the model only within 2^-40 of such a tie.
"""
import random

import ks_model as km

LEVELS = km.CASE_LEVELS      # 5, 3, 2: the key is made at level 5
TERMS = (1, 3, 9)
MSG_MAX = 1000


def add(x, y, m):
    return [(u + v) % m for u, v in zip(x, y)]


def tensor_sum(cts_a, cts_b, Ql):
    """(d0, d1, d2) mod Ql of sum_t a[t] (x) b[t]; cts_b None: the squares of a."""
    n = len(cts_a[0][0])
    d0, d1, d2 = [0] * n, [0] * n, [0] * n
    for t, (a0, a1) in enumerate(cts_a):
        b0, b1 = cts_b[t] if cts_b is not None else (a0, a1)
        d0 = add(d0, km.negacyclic(a0, b0, Ql), Ql)
        d1 = add(d1, add(km.negacyclic(a0, b1, Ql), km.negacyclic(a1, b0, Ql), Ql), Ql)
        d2 = add(d2, km.negacyclic(a1, b1, Ql), Ql)
    return d0, d1, d2


def product(q, p, alpha, level, cts_a, cts_b, key, rescale):
    """The model's result: {"d": (d0, d1, d2), "relin": (r0, r1) mod Q_level, "out": (out0, out1) -- the rescaled pair
    mod Q_(level-1) with `rescale`, else (r0, r1) --, "margin"}."""
    Ql = km.prod(q[:level])
    d0, d1, d2 = tensor_sum(cts_a, cts_b, Ql)
    k0, k1, margin = km.keyswitch(q, p, alpha, level, d2, key)
    r0, r1 = add(d0, k0, Ql), add(d1, k1, Ql)
    out = (r0, r1)
    if rescale:
        ql = q[level - 1]
        o0, m0 = km.moddown(r0, ql, Ql // ql)
        o1, m1 = km.moddown(r1, ql, Ql // ql)
        out, margin = (o0, o1), min(margin, m0, m1)
    return {"d": (d0, d1, d2), "relin": (r0, r1), "out": out, "margin": margin}


def degree2_decryption(d, s, s2, Ql):
    """D = d0 + d1 s + d2 s^2 mod Ql."""
    return add(d[0], add(km.negacyclic(d[1], s, Ql), km.negacyclic(d[2], s2, Ql), Ql), Ql)


def decryption_error(q, level, res, s, s2, rescale):
    """max |q' (out0 + out1 s) - D| centred mod Q_level, q' = q_(level-1) with rescale (the bound multiplied through),
    else 1."""
    Ql = km.prod(q[:level])
    D = degree2_decryption(res["d"], s, s2, Ql)
    f = q[level - 1] if rescale else 1
    o0, o1 = res["out"]
    dec = add(o0, km.negacyclic(o1, s, Ql), Ql)
    return max(abs(km.centered(f * x - y, Ql)) for x, y in zip(dec, D))


def bound(q, p, alpha, level, n, rescale):
    """The bound of the docstring, multiplied through by q_(level-1) with rescale."""
    b = km.error_bound(q, p, alpha, level, n, km.B_E)
    return b + q[level - 1] * (n + 1) / 2 if rescale else b


def seeded_inputs(bits, level, nterms, square, seed=1):
    """The ciphertexts the CPU and GPU tests share: per term (b, a) with a uniform mod Q_level and b = m - a s for a
    message |m| <= MSG_MAX, under the secret of km.seeded_case(bits, "relin").  Returns (case, cts_a, cts_b, msgs_a,
    msgs_b); cts_b and msgs_b are None in the square form."""
    cs = km.seeded_case(bits, "relin", True)
    q, n, s = cs["q"], cs["n"], cs["s_to"]
    Ql = km.prod(q[:level])
    rnd = random.Random(f"ctmul-{seed}-{bits}-{level}-{nterms}-{square}")

    def encrypt():
        a = [rnd.randrange(Ql) for _ in range(n)]
        m = [rnd.randint(-MSG_MAX, MSG_MAX) for _ in range(n)]
        b = [(mv - v) % Ql for mv, v in zip(m, km.negacyclic(a, s, Ql))]
        return (b, a), m

    ea = [encrypt() for _ in range(nterms)]
    eb = None if square else [encrypt() for _ in range(nterms)]
    return (cs, [c for c, _ in ea], None if square else [c for c, _ in eb], [m for _, m in ea],
            None if square else [m for _, m in eb])


def message_product(msgs_a, msgs_b):
    """sum_t m_a[t] m_b[t] mod X^N + 1 over the integers (msgs_b None: the squares)."""
    n = len(msgs_a[0])
    big = 1 << 200
    tot = [0] * n
    for t, ma in enumerate(msgs_a):
        mb = msgs_b[t] if msgs_b is not None else ma
        tot = [x + km.centered(y, big) for x, y in zip(tot, km.negacyclic(ma, mb, big))]
    return tot
