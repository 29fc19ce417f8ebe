"""Model of the plaintext x ciphertext products (csrc/ptmul.hip; no GPU, no product code): the exact integer reference
of the plaintext-weighted sum and of Y = W X + B, the bound behind the kernels' fold, and the slot error bound of the
end-to-end test of tests/test_ptmul_gpu.py."""
import numpy as np

from test_ctmat_gpu import _add_products, _limbs_mod

FOLD = 16            # csrc/ptmul.hpp kPtmulFold: the sums are reduced every 16 terms
MAX_TERMS = 64       # csrc/ptmul.hpp kPtmulMaxTerms
B_PK = 21            # |e| of one noise draw (tests/rlwe_model.py NOISE_BITS)


def _add_residue(acc, x):
    """acc (four uint64 arrays of 32-bit limbs with headroom) += x, exactly."""
    acc[0] += x & np.uint64(0xFFFFFFFF)
    acc[1] += x >> np.uint64(32)


def sum_int(x0, x1, pt, term_x, term_pt, moduli, addend_pt=-1, carry=None):
    """(out0, out1), each [P][level][N] uint64: sum_t pt[term_pt[t]] x_c[term_x[t]] (+ pt[addend_pt] on component 0, +
    carry_c) mod q_r in exact integers.  x0, x1 [nsrc][P][level][N]; pt [npt][P or 1][level][N] (1: shared by the
    batch); carry None or a pair of [P][level][N].  Every product is summed in 32-bit limbs (at most 128 products of
    residues below 2^62: no limb exceeds 2^41) and the sum reduced once."""
    assert len(term_x) == len(term_pt) and 1 <= len(term_x) <= 128
    q = np.array([int(v) for v in moduli], dtype=object)[:, None]
    shape = x0.shape[1:]
    s = [[np.zeros(shape, np.uint64) for _ in range(4)] for _ in range(2)]
    for tx, tp in zip(term_x, term_pt):
        w = np.broadcast_to(pt[tp], shape)
        _add_products(s[0], w, x0[tx])
        _add_products(s[1], w, x1[tx])
    if addend_pt >= 0:
        _add_residue(s[0], np.broadcast_to(pt[addend_pt], shape))
    if carry is not None:
        _add_residue(s[0], carry[0])
        _add_residue(s[1], carry[1])
    return tuple(_limbs_mod(acc, q) for acc in s)


def matprod_int(w, x0, x1, moduli, m, n, k, bias=None, carry=None):
    """(out0, out1), each [m][n][P][level][N] uint64, of W X + B in exact integers: w [>= m][>= k][P or 1][level][N],
    x0, x1 [>= k][>= n][P][level][N], bias None or anything that broadcasts to the outputs' shape, carry None or a
    pair of arrays of that shape (what MFHE_PTMUL_ADD finds in the outputs).  Limb sums as sum_int, at most 128 terms."""
    assert 1 <= k <= 128
    q = np.array([int(v) for v in moduli], dtype=object)[:, None]
    shape = (m, n) + x0.shape[2:]
    s = [[np.zeros(shape, np.uint64) for _ in range(4)] for _ in range(2)]
    for t in range(k):
        wt = np.broadcast_to(w[:m, t][:, None], shape)
        _add_products(s[0], wt, x0[t, :n][None])
        _add_products(s[1], wt, x1[t, :n][None])
    if bias is not None:
        _add_residue(s[0], np.broadcast_to(bias, shape))
    if carry is not None:
        _add_residue(s[0], carry[0])
        _add_residue(s[1], carry[1])
    return tuple(_limbs_mod(acc, q) for acc in s)


def fold_headroom(fold=FOLD, qbits=62):
    """2^128 - 1 minus the largest value a running sum of the kernels can hold: `fold` products of canonical residues
    of a modulus below 2^qbits, and beside them what a fold carries in: the residue of the terms before, or at the
    start the bias (the addend) and the outputs' contents under MFHE_PTMUL_ADD, two residues.  Negative: it overflows."""
    top = (1 << qbits) - 2                      # the largest residue of the largest modulus
    return (1 << 128) - 1 - (fold * top * top + 2 * top)


def slot_error_bound(n_ring, k, w_max, x_max, scale_w, scale_x, q_drop, fp_w, fp_x, fp_b, fp_out, bias=True):
    """What a slot of the decoded Y = W X + B may differ by from numpy's, W m x k plaintexts and X k x n public-key
    encryptions, after one rescale by q_drop, the secret ternary; every term derived, none fitted.

    A coefficient error of at most B moves a slot by at most N B (a slot is a sum of the N coefficients with weights
    of modulus 1), and decoding maps the ring product to the slot-wise one, so in the slots, in units of the values:
      dw = N (1/2) / scale_w + fp_w                      the rounded encoding of a weight and the encoder's f64 term
      dx = N (1/2 + B_PK (2 N + 1)) / scale_x + fp_x     the same for x, and the noise of rlwe_encrypt_pk: e0 + e1 s +
                                                         e u with |e*| <= B_PK and s, u ternary
      db = N (1/2) / scale_b + fp_b                      the bias, rounded at scale_b and lifted by the integer
                                                         scale_w scale_x / scale_b (exact): scale_b = scale_x here
      (w + dw)(x + dx) - w x <= |w| dx + |x| dw + dw dx  per term, k terms
      N (N + 1) / 2 / (scale_w scale_x / q_drop)         the rescale: each component is rounded by at most 1/2 per
                                                         coefficient and the second meets the ternary secret
      fp_out                                             the decoder's f64 term on the expected result
    fp_*: the codec's terms as tests/test_slot_gpu.py _fp_terms states them on tests/slot_model.py."""
    N = n_ring
    dw = N * 0.5 / scale_w + fp_w
    dx = N * (0.5 + B_PK * (2 * N + 1)) / scale_x + fp_x
    db = (N * 0.5 / scale_x + fp_b) if bias else 0.0
    out_scale = scale_w * scale_x / q_drop
    return k * (w_max * dx + x_max * dw + dw * dx) + db + N * (N + 1) / 2 / out_scale + fp_out
