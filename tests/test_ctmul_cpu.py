"""CPU checks of the ciphertext-product model (tests/ctmul_model.py), the yardstick of tests/test_ctmul_gpu.py: it
decrypts within the bound its docstring derives, with and without rescale, and its seeded inputs stay clear of the one
place where the library's ModDown is allowed to differ from it.  Separately: the C ABI and the Python layer declare
the three entry points (that test needs no GPU and fails without the feature).

Shape: N = 16, 5 Q primes + 2 special primes, alpha 2, levels 5, 3 and 2 (the key is made at level 5), 1, 3 and 9
terms, general and square form."""
import pytest

import ctmul_model as cm
import ks_model as km

BITS = pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["45-49", "50-61"])
FORMS = pytest.mark.parametrize("square", [False, True], ids=["general", "square"])


@BITS
@FORMS
@pytest.mark.parametrize("nterms", cm.TERMS)
def test_model_decrypts_within_the_bound_and_keeps_its_margin(bits, square, nterms):
    """|out0 + out1 s - D|_inf <= km.error_bound without rescale and <= km.error_bound / q + (N + 1)/2 with it (checked
    multiplied through by q = q_(level-1)); messages |m| <= 1000 come out as round(sum m_a m_b / q) within that bound;
    every centred remainder of the two ModDowns and the two rescales stays 2^-30 of its modulus away from a tie."""
    for level in cm.LEVELS:
        cs, cts_a, cts_b, ma, mb = cm.seeded_inputs(bits, level, nterms, square)
        q, p, alpha, n, s, s2 = cs["q"], cs["p"], cs["alpha"], cs["n"], cs["s_to"], cs["s_from"]
        Ql = km.prod(q[:level])
        M = cm.message_product(ma, mb)
        assert max(abs(v) for v in M) <= nterms * n * cm.MSG_MAX ** 2
        for rescale in (False, True):
            res = cm.product(q, p, alpha, level, cts_a, cts_b, cs["key"], rescale)
            err = cm.decryption_error(q, level, res, s, s2, rescale)
            bnd = cm.bound(q, p, alpha, level, n, rescale)
            print(f"bits {bits} level {level} terms {nterms} square {square} rescale {rescale}: "
                  f"error / bound = {err / bnd:.4f}, margin {res['margin']:.3e}")
            assert bnd < Ql // 4, "the bound must mean something mod Q_level"
            assert err <= bnd, (level, rescale, err, bnd)
            assert res["margin"] >= 2.0 ** -30, "pick another seed: a remainder sits at a tie"
            # the ciphertexts carry no noise, so D is the product of the messages exactly
            D = cm.degree2_decryption(res["d"], s, s2, Ql)
            assert [km.centered(v, Ql) for v in D] == M
            if rescale:
                ql = q[level - 1]
                Qn = Ql // ql
                o0, o1 = res["out"]
                dec = [km.centered(x + y, Qn) for x, y in zip(o0, km.negacyclic(o1, s, Qn))]
                want = [(2 * v + ql) // (2 * ql) for v in M]          # round(M / q)
                assert max(abs(x - y) for x, y in zip(dec, want)) <= bnd / ql + 0.5


@BITS
def test_the_square_form_is_the_general_form_on_equal_operands(bits):
    cs, cts_a, _, _, _ = cm.seeded_inputs(bits, 3, 3, True)
    Ql = km.prod(cs["q"][:3])
    assert cm.tensor_sum(cts_a, None, Ql) == cm.tensor_sum(cts_a, cts_a, Ql)
    d0, d1, d2 = cm.tensor_sum(cts_a[:1], None, Ql)
    a0, a1 = cts_a[0]
    assert d1 == [2 * v % Ql for v in km.negacyclic(a0, a1, Ql)]


def test_the_abi_and_the_python_layer_declare_the_product(mfhe):
    names = mfhe.declared_symbols()
    for name in ("mfhe_ctmul_tensor", "mfhe_ctmul_apply", "mfhe_ctmul_reserve"):
        assert name in names, name
        assert hasattr(mfhe.lib, name), name
    for method in ("ctmul_tensor", "ctmul_reserve", "ctmul"):
        assert callable(getattr(mfhe.Context, method, None)), method
    assert mfhe.CTMUL_RESCALE == 1
