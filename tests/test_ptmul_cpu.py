"""CPU checks behind the plaintext x ciphertext products (csrc/ptmul.hip): the exact integer reference of
tests/ptmul_model.py against Python integers, the bytes models of tools/ptmat_bench.py against their closed forms, the
bound behind the kernels' fold, and the slot error bound of the end-to-end GPU test.  No device code runs."""
import sys
from pathlib import Path

import numpy as np

import ptmul_model as pmm
from test_keyswitch_gpu import _moduli, _random_rows

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import ptmat_bench as pb  # noqa: E402


def _int_sum(terms, q):
    """sum of products of Python integers mod q, elementwise over flat arrays."""
    acc = [0] * len(terms[0][0])
    for a, b in terms:
        acc = [s + int(u) * int(v) for s, u, v in zip(acc, a, b)]
    return [s % q for s in acc]


def test_the_limb_reference_equals_python_integers():
    """A 17-term sum with repeated indices, an addend and a carry, per-polynomial and shared plaintexts, and the same
    terms as a 2 x 2 product with a bias: 32-bit limb sums against Python integers."""
    mod, n = _moduli(4, (50, 61))[:3], 16
    rng = np.random.default_rng(11)
    P, nsrc, npt, nt = 2, 5, 4, 17
    x0, x1 = (_random_rows(rng, (nsrc, P), mod, n) for _ in range(2))
    carry = tuple(_random_rows(rng, (P,), mod, n) for _ in range(2))
    term_x = [int(v) for v in rng.integers(0, nsrc, nt)]
    term_pt = [int(v) for v in rng.integers(0, npt, nt)]
    for shared in (False, True):
        pt = _random_rows(rng, (npt, 1 if shared else P), mod, n)
        got = pmm.sum_int(x0, x1, pt, term_x, term_pt, mod, addend_pt=3, carry=carry)
        for p in range(P):
            for r, q in enumerate(mod):
                for c, x in enumerate((x0, x1)):
                    terms = [(pt[tp, 0 if shared else p, r], x[tx, p, r]) for tx, tp in zip(term_x, term_pt)]
                    terms.append((carry[c][p, r], np.ones(n, np.uint64)))
                    if c == 0:
                        terms.append((pt[3, 0 if shared else p, r], np.ones(n, np.uint64)))
                    assert got[c][p, r].tolist() == _int_sum(terms, q), (shared, p, r, c)
    # the matrix form: entry (i, j) is the sum over row i of W and column j of X
    w = _random_rows(rng, (2, nt, P), mod, n)
    y0, y1 = (_random_rows(rng, (nt, 2, P), mod, n) for _ in range(2))
    bias = _random_rows(rng, (2, 2, P), mod, n)
    got = pmm.matprod_int(w, y0, y1, mod, 2, 2, nt, bias=bias)
    for i in range(2):
        for j in range(2):
            pts = np.concatenate([w[i], bias[i, j][None]])
            want = pmm.sum_int(y0[:, j], y1[:, j], pts, list(range(nt)), list(range(nt)), mod, addend_pt=nt)
            for c in range(2):
                np.testing.assert_array_equal(got[c][i, j], want[c])


def test_the_bytes_models_equal_their_closed_forms():
    N, level, P = 1 << 16, 11, 4
    unit = 8 * N * level * P
    # one output, one term: a plaintext and two components in, two components out -- one ptmul_sum of one term
    assert pb.tensor_model_bytes(N, level, P, 1, 1, 1, 2, 2) == unit * (3 + 2)
    assert pb.tensor_model_bytes(N, level, P, 1, 1, 1, 2, 2) == pb.sum_model_bytes(N, level, P, 1)
    assert pb.tensor_model_bytes(N, level, P, 1, 1, 1, 4, 2, bias=True, add=True) == unit * (3 + 1 + 2 + 2)
    assert pb.sum_model_bytes(N, level, P, 7, addend=True) == unit * (21 + 1 + 2)
    # an edge-tile shape: 5 x 3 with k = 7; a 2 x 2 tile has 3 x 2 tiles, a 4 x 2 tile 2 x 2
    assert pb.tensor_model_bytes(N, level, P, 5, 3, 7, 2, 2) == unit * (7 * (5 * 2 + 2 * 3 * 3) + 2 * 15)
    assert pb.tensor_model_bytes(N, level, P, 5, 3, 7, 4, 2, bias=True) == unit * (7 * (5 * 2 + 2 * 3 * 2) + 15 + 30)
    # full tiles: (TM + 2 TN) / (TM TN) streams per term and output, against 3 for separate sums
    for (tm, tn), per in (((2, 2), 1.5), ((4, 2), 1.0), ((4, 1), 1.5), ((1, 1), 3.0)):
        k = 8
        assert pb.tensor_model_bytes(N, level, P, 4, 4, k, tm, tn) == unit * (16 * per * k + 32)


def test_the_fold_fits_a_u128_and_is_the_longest_that_does():
    """16 products of residues of a 62-bit modulus, and beside them two residues (the bias and the MFHE_PTMUL_ADD
    carry-in at the start, one reduced residue afterwards): below 2^128; 17 products are not."""
    assert pmm.FOLD == 16
    assert pmm.fold_headroom(pmm.FOLD) >= 0
    assert pmm.fold_headroom(pmm.FOLD + 1) < 0
    assert pmm.fold_headroom(pmm.FOLD) == (1 << 128) - 1 - (16 * ((1 << 62) - 2) ** 2 + 2 * ((1 << 62) - 2))
    assert pmm.MAX_TERMS % pmm.FOLD == 0


def test_the_slot_error_bound_is_the_sum_of_its_terms():
    """The bound against the terms worked out by hand at N = 2^10, k = 5, scales 2^45 and a 45-bit dropped limb, f64
    terms zero: the encryption noise dominates, and the result is far below the spread of slots of size 1."""
    N, k, s, q = 1 << 10, 5, 2.0 ** 45, 2.0 ** 45
    dw = N / 2 / s
    dx = N * (0.5 + 21 * (2 * N + 1)) / s
    want = k * (1.0 * dx + 1.0 * dw + dw * dx) + N / 2 / s + N * (N + 1) / 2 / (s * s / q)
    got = pmm.slot_error_bound(N, k, 1.0, 1.0, s, s, q, 0.0, 0.0, 0.0, 0.0)
    assert abs(got - want) <= 1e-12 * want
    assert k * dx > 0.9 * got and got < 2.0 ** -16
    # without a bias its term leaves, and each f64 term enters with the weight stated
    assert pmm.slot_error_bound(N, k, 1.0, 1.0, s, s, q, 0.0, 0.0, 0.0, 0.0, bias=False) < got
    assert pmm.slot_error_bound(N, k, 2.0, 3.0, s, s, q, 1e-9, 1e-9, 1e-9, 1e-9) > got + k * 5e-9 + 2e-9
