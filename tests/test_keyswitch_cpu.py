"""CPU checks of the key-switching model (tests/ks_model.py), the yardstick of tests/test_keyswitch_gpu.py: it
decrypts within the bound the algorithm promises, and its seeded inputs stay clear of the one place where the
library's ModDown is allowed to differ from it.

Shape: N = 16, 5 Q primes + 2 special primes, alpha 2, levels 5, 3 and 2 (the key is made at level 5)."""
import pytest

import ks_model as km


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["45-49", "50-61"])
@pytest.mark.parametrize("kind", ["switch", "relin"])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "noise-free"])
def test_model_decrypts_within_the_bound(bits, kind, noise):
    """|k_0 + k_1 s_to - c s_from|_inf <= (N + 1)/2 + 1 + beta alpha N B_e max_j Q_j / P for ternary s_to and
    |e| <= B_e; with e = 0 the noise term vanishes from the bound."""
    cs = km.seeded_case(bits, kind, noise)
    q, p, alpha, n = cs["q"], cs["p"], cs["alpha"], cs["n"]
    assert len(q) == 5 and len(p) == 2 and len(set(q + p)) == 7
    assert all(abs(v) <= 1 for v in cs["s_to"])
    assert all(abs(v) <= (km.B_E if noise else 0) for ej in cs["e"] for v in ej)
    for level in km.CASE_LEVELS:
        k0, k1, _ = km.keyswitch(q, p, alpha, level, cs["c"][level], cs["key"])
        err = km.decryption_error(q, level, k0, k1, cs["c"][level], cs["s_from"], cs["s_to"])
        bound = km.error_bound(q, p, alpha, level, n, km.B_E if noise else 0)
        print(f"bits {bits} {kind} level {level}: error {err}, bound {bound:.2f}")
        assert bound < km.prod(q[:level]) // 4, "the bound must mean something mod Q_level"
        assert err <= bound, (level, err, bound)
        if not noise:
            assert bound == (n + 1) / 2 + 1


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["45-49", "50-61"])
@pytest.mark.parametrize("kind", ["switch", "relin"])
def test_seeded_inputs_keep_their_margin_from_half_of_p(bits, kind):
    """Every centred remainder of both ModDowns stays at least 2^-30 P away from +-P/2, so the library's documented
    2^-40 window (MFHE_BCONV_CENTERED) cannot matter and the GPU test may demand exact equality."""
    cs = km.seeded_case(bits, kind, True)
    for level in km.CASE_LEVELS:
        _, _, margin = km.keyswitch(cs["q"], cs["p"], cs["alpha"], level, cs["c"][level], cs["key"])
        print(f"bits {bits} {kind} level {level}: margin {margin:.3e} P")
        assert margin >= 2.0 ** -30, (level, margin)


def test_key_factor_is_p_on_its_digit_and_zero_elsewhere():
    q, p = km.case_moduli((45, 49))
    P = km.prod(p)
    for j, (s, n) in enumerate(km.digits(5, 2)):
        F = km.key_factor(q, p, 2, j)
        for r, m in enumerate(q):
            assert F % m == (P % m if s <= r < s + n else 0)
        assert all(F % m == 0 for m in p)


def test_raised_digit_is_the_fast_formula():
    """d~_j = c mod Q_j + u Q_j with 0 <= u < alpha: congruent to c on the digit's limbs and below alpha Q_j."""
    cs = km.seeded_case()
    q = cs["q"]
    for level in km.CASE_LEVELS:
        for s, n in km.digits(level, 2):
            Qj = km.prod(q[s:s + n])
            d = km.raise_digit(cs["c"][level], q, s, n)
            assert all(0 <= v < n * Qj and (v - c) % Qj == 0 for v, c in zip(d, cs["c"][level]))
