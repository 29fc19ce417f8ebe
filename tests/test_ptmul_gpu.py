"""GPU checks of the plaintext x ciphertext products (csrc/ptmul.hip; include/mfhe.h mfhe_ptmul_sum, mfhe_ptmat_tensor,
mfhe_ptmat_reserve, mfhe_ptmat_apply and the Python layer's ptmul_sum / ptmat_tensor / ptmat_reserve / ptmat),
bit-exact: the formulas in the exact integers of tests/ptmul_model.py, m n calls of ptmul_sum, and ptmat_tensor
followed by ntt_moddown.  Every comparison is exact equality (the arithmetic is integer; ModDown's one f64 sum only
selects the multiple of its modulus and runs in a fixed order per coefficient) except the end-to-end test, which
holds the decoded slots to the derived bound of ptmul_model.slot_error_bound."""
import numpy as np
import pytest

import ptmul_model as pmm
from primes import primes_of_size
from test_ctmat_gpu import _Matrix
from test_keyswitch_gpu import LAYOUTS, _ctx, _moduli, _polys, _random_rows, _u64

pytestmark = pytest.mark.gpu

CLASSES = pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
LOGNS = pytest.mark.parametrize("log_n", [4, 10])
FOLD = pmm.FOLD
KEY = bytes((29 * i + 5) & 0xFF for i in range(32))


def _shapes(tm, tn):
    """(m, n, k): one output, a full tile, every edge remainder of the tile in m alone, in n alone and in both, a 1 x n
    and an m x 1 line, k on both sides of the fold and the largest sum."""
    s = [(1, 1, 1), (tm, tn, 1)]
    s += [(tm + r, tn, 7) for r in range(1, tm)]
    s += [(tm, tn + c, FOLD) for c in range(1, tn)]
    s += [(tm + r, tn + c, FOLD + 1) for r in range(1, max(tm, 2)) for c in range(1, max(tn, 2))]
    s += [(1, 2 * tn, FOLD - 1), (2 * tm, 1, 64)]
    return s


def test_shapes_cover_every_edge_of_the_built_tile(mfhe):
    tm, tn = mfhe.PTMAT_TILE
    s = _shapes(tm, tn)
    assert {m % tm for m, _, _ in s} >= set(range(tm)) and {n % tn for _, n, _ in s} >= set(range(tn))
    assert {k for _, _, k in s} >= {1, FOLD - 1, FOLD, FOLD + 1, 64}
    if (tm, tn) == (2, 2):
        assert s == [(1, 1, 1), (2, 2, 1), (3, 2, 7), (2, 3, 16), (3, 3, 17), (1, 4, 15), (4, 1, 64)]


# ---------------------------------------------------------------------------------------------------------------
# 1. the plaintext-weighted sum against exact integers
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_sum_bit_exact(mfhe, log_n, bits):
    """nterms 1, 2, both sides of every fold up to 64, random (so repeated) indices, every layout of LAYOUTS with 1 and
    3 polynomials each, shared and per-polynomial plaintexts, with and without the addend; sources and plaintexts are
    stored one row above the call's level.  The pads stay canaries and the inputs are unchanged."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(80 + log_n)
    level, P, nsrc, npt = (3, 3, 5, 4) if log_n == 4 else (2, 3, 5, 4)
    rows = level + 1
    x0, x1 = (_random_rows(rng, (1, nsrc, P), mod[:rows], N) for _ in range(2))
    pt = _random_rows(rng, (1, npt, P), mod[:rows], N)
    counts = [1, 2, FOLD - 1, FOLD, FOLD + 1, 2 * FOLD, 2 * FOLD + 1, 64]
    terms = {nt: ([int(v) for v in rng.integers(0, nsrc, nt)], [int(v) for v in rng.integers(0, npt, nt)])
             for nt in counts}
    want = {}
    for nt, (tx, tp) in terms.items():
        for shared in (False, True):
            for addend in (-1, 2):
                want[nt, shared, addend] = pmm.sum_int(x0[0, :, :, :level], x1[0, :, :, :level],
                                                       pt[0, :, :1 if shared else P, :level], tx, tp, mod[:level], addend)
    for name, ppad, tpad, off in LAYOUTS:
        for npoly in (1, 3):
            X0, X1 = (_Matrix(mfhe, 1, nsrc, npoly, rows, N, ppad, tpad, 0, off, x) for x in (x0, x1))
            PT = _Matrix(mfhe, 1, npt, npoly, rows, N, ppad + 2, tpad + 2, 0, off, pt)
            for (nt, shared, addend), w in want.items():
                o0, o1 = (_polys(mfhe, npoly, level, N, ppad, off) for _ in range(2))
                ctx.ptmul_sum(X0.t, X1.t, PT.t, o0.t, o1.t, *terms[nt], npoly, level, nsrc, npt, addend,
                              src_stride=X0.cs, x_poly_stride=X0.pst, pt_stride=PT.cs,
                              pt_poly_stride=0 if shared else PT.pst, out_stride=o0.stride)
                torch.cuda.synchronize()
                for c, o in enumerate((o0, o1)):
                    np.testing.assert_array_equal(o.blocks((npoly, level, N)), w[c][:npoly],
                                                  err_msg=f"out{c} {name} npoly {npoly} nterms {nt} shared {shared} "
                                                          f"addend {addend}")
                    o.check_pads()
            for blk in (X0, X1, PT):
                np.testing.assert_array_equal(blk.get(), blk.src, err_msg=name)
                blk.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 2. the tiled product against exact integers and against m n sums
# ---------------------------------------------------------------------------------------------------------------
BIASES = ("none", "full", "row", "col", "shared")


def _bias_case(kind, B, b, m, n, npoly):
    """(tensor, strides, expected array) of a bias variant on the matrix B holding b."""
    if kind == "none":
        return None, None, None
    rs, cs, ps = B.strides
    if kind == "row":        # one row of bias for every row
        return B.t, (0, cs, ps), b[:1, :n, :npoly]
    if kind == "col":        # one column for every column
        return B.t, (rs, 0, ps), b[:m, :1, :npoly]
    if kind == "shared":     # one polynomial for the batch
        return B.t, (rs, cs, 0), b[:m, :n, :1]
    return B.t, B.strides, b[:m, :n, :npoly]


@CLASSES
@LOGNS
def test_tensor_bit_exact(mfhe, log_n, bits):
    """Every shape of _shapes(tile) in the 16-byte form (dense, padded) and the scalar one (padded-odd, misaligned), W
    and X at different strides, 1 and 3 polynomials, once with X stored transposed and once with W shared over the
    batch; the bias absent, full, one row, one column and one polynomial (all five on the dense layout, the absent one
    and one of the others in turn elsewhere); the pads around every output entry stay
    canaries and the inputs are unchanged.  On the dense and the misaligned layout every entry also equals its own
    ptmul_sum bit for bit (one polynomial without a bias, three with the full one)."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(90 + log_n)
    shapes = _shapes(*mfhe.PTMAT_TILE)
    level, P = (3, 3) if log_n == 4 else (2, 3)
    R, K, C = max(s[0] for s in shapes), max(s[2] for s in shapes), max(s[1] for s in shapes)
    w = _random_rows(rng, (R, K, P), mod[:level], N)
    x0, x1 = (_random_rows(rng, (K, C, P), mod[:level], N) for _ in range(2))
    b = _random_rows(rng, (R, C, P), mod[:level], N)
    qrow = _u64(mod[:level])[:, None]
    products = {}

    def product(wshared, m, n, k):
        """W X in exact integers for all P polynomials, computed once per shape (the bias is added in uint64)."""
        if (wshared, m, n, k) not in products:
            products[wshared, m, n, k] = pmm.matprod_int(w[:, :, :1] if wshared else w, x0, x1, mod[:level], m, n, k)
        return products[wshared, m, n, k]

    runs = [layout + (False, False) for layout in LAYOUTS]
    runs += [("dense, X transposed", 0, 0, 0, True, False), ("dense, W shared", 0, 0, 0, False, True)]
    for name, ppad, tpad, off, tr, wshared in runs:
        for npoly in (1, 3):
            W = _Matrix(mfhe, R, K, npoly, level, N, ppad, tpad, tpad, off, w)
            X0, X1 = (_Matrix(mfhe, K, C, npoly, level, N, ppad + 2, tpad + 2, tpad, off, x, tr) for x in (x0, x1))
            B = _Matrix(mfhe, R, C, npoly, level, N, ppad, tpad + 4, tpad, off, b)
            assert W.strides != X0.strides and (X0.cs > X0.rs) == tr
            ws = (W.rs, W.cs, 0) if wshared else W.strides
            for si, (m, n, k) in enumerate(shapes):
                # every bias form on every shape of the dense layout; elsewhere none, the full one on the layouts the
                # sums are compared on and the other forms in turn
                turn = BIASES[1 + (si + npoly) % 4]
                for kind in BIASES if name == "dense" else ("none", "full" if name == "misaligned" else turn):
                    bt, bs, bv = _bias_case(kind, B, b, m, n, npoly)
                    want = [v[:, :, :npoly] for v in product(wshared, m, n, k)]
                    if bv is not None:                         # residues below 2^62: the sum fits a uint64
                        want[0] = (want[0] + bv) % qrow
                    o0, o1 = (_Matrix(mfhe, m, n, npoly, level, N, ppad, 2, 4, off) for _ in range(2))
                    ctx.ptmat_tensor(W.t, X0.t, X1.t, o0.t, o1.t, m, n, k, npoly, level, bias=bt, w_strides=ws,
                                     x_strides=X0.strides, bias_strides=bs, out_strides=o0.strides)
                    torch.cuda.synchronize()
                    msg = f"{name} npoly {npoly} shape {(m, n, k)} bias {kind}"
                    for c, o in enumerate((o0, o1)):
                        np.testing.assert_array_equal(o.get(), want[c], err_msg=f"out{c} " + msg)
                        o.check_pads()
                    if (kind, npoly) not in (("none", 1), ("full", 3)) or name not in ("dense", "misaligned"):
                        continue
                    got = (o0.get(), o1.get())
                    for i in range(m):                         # entry (i, j) is one plaintext-weighted sum
                        for j in range(n):
                            e0, e1 = (_polys(mfhe, npoly, level, N, 0, off) for _ in range(2))
                            # the plaintexts of the sum are row i of W; the bias lies in another buffer, so it is no
                            # addend of that call and is added here
                            ctx.ptmul_sum(X0.t[j * X0.cs:], X1.t[j * X1.cs:], W.t[i * W.rs:], e0.t, e1.t,
                                          list(range(k)), list(range(k)), npoly, level, k, k, src_stride=X0.rs,
                                          x_poly_stride=X0.pst, pt_stride=W.cs, pt_poly_stride=ws[2])
                            torch.cuda.synchronize()
                            h0, h1 = (e.blocks((npoly, level, N)) for e in (e0, e1))
                            if kind == "full":                 # followed by an addition mod q_r
                                h0 = (h0 + b[i, j, :npoly]) % qrow
                            np.testing.assert_array_equal(got[0][i, j], h0, err_msg=f"out0[{i}][{j}] vs sum, " + msg)
                            np.testing.assert_array_equal(got[1][i, j], h1, err_msg=f"out1[{i}][{j}] vs sum, " + msg)
            for blk in (W, X0, X1, B):
                np.testing.assert_array_equal(blk.get(), blk.src, err_msg=name)
                blk.check_pads()


@CLASSES
def test_add_chains_two_chunks_of_40_terms(mfhe, bits):
    """MFHE_PTMUL_ADD: an inner dimension of 80 as two calls of 40 terms, the second adding into the first's outputs,
    equals the exact 80-term sum with its bias; a product with a full tile and every edge tile, both forms."""
    import torch
    log_n = 4
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 16
    rng = np.random.default_rng(97)
    tm, tn = mfhe.PTMAT_TILE
    m, n, K, level, npoly = 2 * tm - 1 if tm > 1 else 2, 2 * tn - 1 if tn > 1 else 2, 80, 3, 2
    w = _random_rows(rng, (m, K, npoly), mod[:level], N)
    x0, x1 = (_random_rows(rng, (K, n, npoly), mod[:level], N) for _ in range(2))
    b = _random_rows(rng, (m, n, npoly), mod[:level], N)
    want = pmm.matprod_int(w, x0, x1, mod[:level], m, n, K, bias=b)
    for name, ppad, tpad, off in (LAYOUTS[0], LAYOUTS[3]):
        W = _Matrix(mfhe, m, K, npoly, level, N, ppad, tpad, tpad, off, w)
        X0, X1 = (_Matrix(mfhe, K, n, npoly, level, N, ppad, tpad, tpad, off, x) for x in (x0, x1))
        B = _Matrix(mfhe, m, n, npoly, level, N, ppad, tpad, tpad, off, b)
        o0, o1 = (_Matrix(mfhe, m, n, npoly, level, N, ppad, 2, 4, off) for _ in range(2))
        ctx.ptmat_tensor(W.t, X0.t, X1.t, o0.t, o1.t, m, n, 40, npoly, level, bias=B.t, w_strides=W.strides,
                         x_strides=X0.strides, bias_strides=B.strides, out_strides=o0.strides)
        ctx.ptmat_tensor(W.t[40 * W.cs:], X0.t[40 * X0.rs:], X1.t[40 * X1.rs:], o0.t, o1.t, m, n, 40, npoly, level,
                         flags=mfhe.PTMUL_ADD, w_strides=W.strides, x_strides=X0.strides, out_strides=o0.strides)
        torch.cuda.synchronize()
        for c, o in enumerate((o0, o1)):
            np.testing.assert_array_equal(o.get(), want[c], err_msg=f"out{c} {name}")
            o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 3. the fold at the worst case
# ---------------------------------------------------------------------------------------------------------------
def test_all_q_minus_1_with_62_bit_primes(mfhe):
    """Every operand, the bias and the MFHE_PTMUL_ADD carry-in q - 1 with 62-bit primes, products with a full tile and
    every edge tile: each product is just below 2^124, so a fold of 16 is 16 maximal products and two maximal
    residues in one u128, and one more term overflows it unless the sums were reduced after 16.  (q - 1)^2 = 1 mod q:
    the plain product is k in both components; with the bias and the carry-in out0 = k - 2 and out1 = k - 1."""
    import torch
    mod = primes_of_size(62, 32, 3)
    assert len(mod) == 3 and all(2 ** 61 < v < 2 ** 62 for v in mod)
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    N, level, npoly, K = 16, 3, 2, 64
    tm, tn = mfhe.PTMAT_TILE
    top = _u64(mod) - np.uint64(1)
    for m in sorted({tm + r for r in range(1, max(tm, 2))}):
        for n in sorted({tn + c for c in range(1, max(tn, 2))}):
            full = lambda lead: np.broadcast_to(top[:, None], lead + (npoly, level, N)).copy()
            for name, ppad, tpad, off in (LAYOUTS[0], LAYOUTS[3]):   # the 16-byte and the scalar form
                W = _Matrix(mfhe, m, K, npoly, level, N, ppad, tpad, tpad, off, full((m, K)))
                X0, X1 = (_Matrix(mfhe, K, n, npoly, level, N, ppad, tpad, tpad, off, full((K, n))) for _ in range(2))
                B = _Matrix(mfhe, m, n, npoly, level, N, ppad, tpad, tpad, off, full((m, n)))
                for k in (FOLD, FOLD + 1, 2 * FOLD, 2 * FOLD + 1, 64):
                    for loaded in (False, True):
                        o0, o1 = (_Matrix(mfhe, m, n, npoly, level, N, ppad, 2, 4, off,
                                          full((m, n)) if loaded else None) for _ in range(2))
                        ctx.ptmat_tensor(W.t, X0.t, X1.t, o0.t, o1.t, m, n, k, npoly, level,
                                         bias=B.t if loaded else None, flags=mfhe.PTMUL_ADD if loaded else 0,
                                         w_strides=W.strides, x_strides=X0.strides, bias_strides=B.strides,
                                         out_strides=o0.strides)
                        torch.cuda.synchronize()
                        for c, o in enumerate((o0, o1)):
                            e = k - (2 - c if loaded else 0)
                            assert (o.get() == np.uint64(e)).all(), f"out{c} {name} {(m, n, k)} loaded {loaded}"
                            o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 4. more tiles x polynomials than grid z holds
# ---------------------------------------------------------------------------------------------------------------
def test_tensor_folds_work_items_over_grid_z(mfhe):
    """One tile of 65538 polynomials of one 16-word row: grid z is 65535, so work items 0, 1 and 2 share their blocks
    with 65535, 65536 and 65537.  Operands below 2^31 and one term: the expected values are uint64 arithmetic."""
    import torch
    bits, log_n = (50, 61), 4
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 16
    m, n = mfhe.PTMAT_TILE
    npoly, level = 65538, 1
    rng = np.random.default_rng(64)
    w = rng.integers(0, 2 ** 31, (m, 1, npoly, level, N), dtype=np.uint64)
    x0, x1 = (rng.integers(0, 2 ** 31, (1, n, npoly, level, N), dtype=np.uint64) for _ in range(2))
    q = np.uint64(mod[0])
    assert int(q) < 2 ** 62
    want = ((w[:, 0][:, None] * x0[0][None]) % q, (w[:, 0][:, None] * x1[0][None]) % q)   # each [m][n][npoly][1][N]
    dev = [mfhe.to_device_u64(v.ravel()) for v in (w, x0, x1)]
    outs = [_polys(mfhe, m * n * npoly, level, N) for _ in range(2)]
    ctx.ptmat_tensor(dev[0], dev[1], dev[2], outs[0].t, outs[1].t, m, n, 1, npoly, level)
    torch.cuda.synchronize()
    for c, o in enumerate(outs):
        got = o.blocks((m, n, npoly, level, N))
        for i in range(m):
            for j in range(n):
                bad = np.flatnonzero((got[i, j] != want[c][i, j]).reshape(npoly, -1).any(axis=1))
                assert bad.size == 0, f"out{c}[{i}][{j}]: {bad.size} wrong polynomials, the first {bad[:8].tolist()}"
        o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 5. the driver = tensor + ntt_moddown
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_ptmat_equals_tensor_then_moddown(mfhe, log_n, bits):
    """ptmat of a 2 x 3 product of 3 terms and 2 polynomials with a bias at levels 5, 3 and 2: without a flag the
    tensor's bits; with PTMUL_RESCALE rows [0, level - 1) equal ptmat_tensor followed by ntt_moddown on each component,
    run over the whole batch of 12 polynomials and entry by entry over 2 (the batch size does not enter the result);
    with PTMUL_ADD on top, the same on the tensor with PTMUL_ADD.  The pads of the outputs stay canaries."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(100 + log_n)
    m, n, k, npoly = 2, 3, 3, 2
    batch = m * n * npoly
    for level in (5, 3, 2):
        lw, keep = level * N, level - 1
        w = _random_rows(rng, (m, k, npoly), mod[:level], N)
        x0, x1 = (_random_rows(rng, (k, n, npoly), mod[:level], N) for _ in range(2))
        b = _random_rows(rng, (m, n, npoly), mod[:level], N)
        seed = [_random_rows(rng, (m, n, npoly), mod[:level], N) for _ in range(2)]   # what PTMUL_ADD finds
        W = _Matrix(mfhe, m, k, npoly, level, N, 2, 4, 2, 0, w)
        X0, X1 = (_Matrix(mfhe, k, n, npoly, level, N, 0, 6, 0, 0, x) for x in (x0, x1))
        B = mfhe.to_device_u64(b.ravel())
        for add in (0, mfhe.PTMUL_ADD):
            t = [mfhe.to_device_u64(s.ravel()) for s in seed]
            ctx.ptmat_tensor(W.t, X0.t, X1.t, t[0], t[1], m, n, k, npoly, level, bias=B, flags=add,
                             w_strides=W.strides, x_strides=X0.strides)
            torch.cuda.synchronize()
            tensor = [mfhe.to_host_u64(v).reshape(batch, level, N).copy() for v in t]
            want = pmm.matprod_int(w, x0, x1, mod[:level], m, n, k, bias=b, carry=seed if add else None)
            for c in range(2):
                np.testing.assert_array_equal(tensor[c], want[c].reshape(batch, level, N))
            whole = [v.clone() for v in t]
            for v in whole:                                    # one ModDown over the 12 polynomials
                ctx.ntt_moddown(v, v, batch, keep, keep, 1)
            parts = [v.clone() for v in t]
            for v in parts:                                    # one per entry, 2 polynomials each
                for e in range(m * n):
                    entry = v[e * npoly * lw:]
                    ctx.ntt_moddown(entry, entry, npoly, keep, keep, 1)
            torch.cuda.synchronize()
            for flags in (add, add | mfhe.PTMUL_RESCALE):
                opad = 2 if log_n == 10 else 3
                o = [_polys(mfhe, batch, level, N, opad, 0, s if add else None) for s in seed]
                ctx.ptmat(W.t, X0.t, X1.t, o[0].t, o[1].t, m, n, k, npoly, level, bias=B, flags=flags,
                          w_strides=W.strides, x_strides=X0.strides, out_stride=o[0].stride)
                torch.cuda.synchronize()
                msg = f"level {level} flags {flags}"
                for c in range(2):
                    got = o[c].blocks((batch, level, N))
                    o[c].check_pads()
                    if not flags & mfhe.PTMUL_RESCALE:
                        np.testing.assert_array_equal(got, tensor[c], err_msg=f"out{c} " + msg)
                        continue
                    for ref, what in ((whole, "12"), (parts, "2")):
                        np.testing.assert_array_equal(
                            got[:, :keep], mfhe.to_host_u64(ref[c]).reshape(batch, level, N)[:, :keep],
                            err_msg=f"out{c} {msg} against ntt_moddown over batches of {what}")
        for blk in (W, X0, X1):
            np.testing.assert_array_equal(blk.get(), blk.src)
            blk.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------
def _prod(q):
    p = 1
    for v in q:
        p *= int(v)
    return p


@CLASSES
def test_end_to_end_with_no_host_arithmetic(mfhe, bits):
    """N = 2^10, level 3: secret and public key, slot_encode of a 3 x 5 weight matrix, of a 3 x 2 bias and of a 5 x 2
    matrix of slot vectors, rlwe_encrypt_pk of the latter, ptmat with PTMUL_RESCALE, rlwe_decrypt, slot_decode;
    compared with numpy's W X + B slot by slot.  Every step between the encoder and the decoder is a library call on
    device tensors.  Weights and inputs are encoded at scale 2^45 (45-bit class) or 2^50 (50-bit class); the bias
    belongs at the product's scale, the square, which is outside slot_encode's domain (|scale c| < 2^63), so it is
    encoded at the same scale and lifted by the integer scale with ct_lincomb, exactly.  The tolerance is
    ptmul_model.slot_error_bound with the codec's f64 terms of test_slot_gpu._fp_terms; it is asserted below 2^-10
    before anything runs on the GPU.

    Measured on an MI355X (slot error / bound): 45-bit class 5.16e-10 / 6.24e-6, 50-bit class
    1.63e-11 / 1.95e-7; the bound is the worst case of the encryption noise, which a sum of 5 random terms stays far
    below."""
    import torch
    import test_slot_gpu as tsg
    log_n, level = 10, 3
    N, ns = 1 << log_n, 1 << (log_n - 1)
    mod = _moduli(log_n, bits)
    q = list(mod[:level])
    scale = 2.0 ** bits[0]
    m, k, n = 3, 5, 2
    rng = np.random.default_rng(123)
    cplx = lambda *lead: (rng.uniform(-1, 1, lead + (ns,)) + 1j * rng.uniform(-1, 1, lead + (ns,))) / np.sqrt(2)
    w, x, b = cplx(m, k), cplx(k, n), cplx(m, n)
    want = np.einsum("its,tjs->ijs", w, x) + b
    out_scale = scale * scale / q[level - 1]
    fp = lambda vs, sc, which: max(tsg._fp_terms(v, log_n, sc)[which] for v in vs.reshape(-1, ns))
    bound = pmm.slot_error_bound(N, k, float(np.abs(w).max()), float(np.abs(x).max()), scale, scale, q[level - 1],
                                 fp(w, scale, 0), fp(x, scale, 0), fp(b, scale, 0), fp(want, out_scale, 1))
    print(f"ptmat end to end ({bits[0]}-bit class): bound {bound:.3g}")
    assert bound < 2.0 ** -10
    assert (float(np.abs(want).max()) + bound) * out_scale * N < int(q[0]) * int(q[1]) // 2
    assert float(np.abs(want).max()) * scale * scale * N < _prod(q) // 2
    # ---- everything above ran on the CPU; from here on the GPU, library calls alone ----
    ctx = _ctx(log_n, bits)
    seed = mfhe.Seed(KEY)
    lw = level * N
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    dev = lambda z: torch.from_numpy(np.ascontiguousarray(z.reshape(-1, ns))).cuda()
    s = ctx.rlwe_sample_small(seed, mfhe.RLWE_SECRET, seed.take(), zeros(lw), 1, level)
    pk0, pk1 = ctx.rlwe_encrypt_sk(seed, seed.take(), s, None, zeros(lw), zeros(lw), 1, level)
    pw = ctx.slot_encode(dev(w), zeros(m * k * lw), m * k, level, scale)
    px = ctx.slot_encode(dev(x), zeros(k * n * lw), k * n, level, scale)
    pb = ctx.slot_encode(dev(b), zeros(m * n * lw), m * n, level, scale)
    lift = mfhe.to_device_u64(_u64([(1 << bits[0]) % v for v in q]))       # the integer scale, per limb
    pb2, _ = ctx.ct_lincomb(pb, pb, lift, zeros(m * n * lw), zeros(m * n * lw), [0], [0], m * n, level, 1, 1)
    c0, c1 = ctx.rlwe_encrypt_pk(seed, seed.take(k * n), pk0, pk1, px, zeros(k * n * lw), zeros(k * n * lw), k * n,
                                 level)
    o0, o1 = ctx.ptmat(pw, c0, c1, zeros(m * n * lw), zeros(m * n * lw), m, n, k, 1, level, bias=pb2,
                       flags=mfhe.PTMUL_RESCALE)
    dec = ctx.rlwe_decrypt(o0, o1, s, zeros(m * n * 2 * N), m * n, 2, in_stride=lw)
    slots = ctx.slot_decode(dec, torch.zeros(m * n * ns, dtype=torch.complex128, device="cuda"), m * n, 2, out_scale)
    torch.cuda.synchronize()
    err = float(np.abs(slots.cpu().numpy().reshape(m, n, ns) - want).max())
    tsg._report(f"ptmat 3 x 5 by 5 x 2 end to end ({bits[0]}-bit class)", err, bound)
    assert err > 0 and float(np.abs(want).max()) > 64 * bound


# ---------------------------------------------------------------------------------------------------------------
# 7. graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After ptmat_reserve, ptmat with PTMUL_RESCALE allocates nothing and copies nothing to the device: it is
    captured into a graph on one stream (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed
    on the captured inputs and then twice on changed ones; each replay equals the eager call on those inputs."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, N = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    m, n, k, npoly, level = 3, 2, 3, 2, 5
    flags = mfhe.PTMUL_RESCALE
    ctx.ptmat_reserve(m, n, npoly, level, flags)
    rng = np.random.default_rng(10)
    lead = [(m, k, npoly), (k, n, npoly), (k, n, npoly), (m, n, npoly)]
    ops = [mfhe.to_device_u64(_random_rows(rng, l, mod[:level], N).ravel()) for l in lead]
    words = m * n * npoly * level * N
    o0 = torch.zeros(words, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(words, dtype=torch.int64, device="cuda")

    def apply(y0, y1):
        ctx.ptmat(ops[0], ops[1], ops[2], y0, y1, m, n, k, npoly, level, bias=ops[3], flags=flags)

    def kept(t):
        return mfhe.to_host_u64(t).reshape(m * n * npoly, level, N)[:, :level - 1].copy()

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        apply(o0, o1)
    first = None
    for _ in range(3):                                         # the captured inputs, then twice fresh ones
        o0.zero_()
        o1.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = (kept(o0), kept(o1))
        e0, e1 = torch.zeros_like(o0), torch.zeros_like(o1)
        apply(e0, e1)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[0], kept(e0))
        np.testing.assert_array_equal(got[1], kept(e1))
        assert got[0].any() and got[1].any()
        if first is not None:
            assert (first[0] != got[0]).any() and (first[1] != got[1]).any()
        first = got
        for t, l in zip(ops, lead):
            t.copy_(mfhe.to_device_u64(_random_rows(rng, l, mod[:level], N).ravel()))


# ---------------------------------------------------------------------------------------------------------------
# 8. argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(mfhe):
    import ctypes
    import torch
    lib = mfhe.lib
    mod, N = _moduli(4, (45, 49)), 16
    ctx = mfhe.Context(list(mod), 4, mfhe.CONV_PHANTOM)
    h = ctx.handle
    names = ("w", "x0", "x1", "bias", "o0", "o1")
    bufs = {name: _polys(mfhe, 1, 3 * 2 * 7, N) for name in names}
    pw, px0, px1, pb, p0, p1 = (bufs[name].t.data_ptr() for name in names)
    E = mfhe.EINVAL
    L5 = 5 * N          # a polynomial at level 5
    EN = 2 * L5         # an entry: 2 polynomials
    LN = 2 * EN         # a line of 2 entries; every matrix here is 2 x 2, 4 EN = 640 of the buffers' 672 words
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    T01 = ints([0, 1])

    def psum(x0=px0, x1=px1, sst=EN, xp=L5, nsrc=2, pt=pw, pst=EN, pp=L5, npt=2, tx=T01, tp=T01, nt=2, addend=-1,
             o0=p0, o1=p1, ost=L5, npoly=2, level=5):
        return lib.mfhe_ptmul_sum(h, x0, x1, sst, xp, nsrc, pt, pst, pp, npt, tx, tp, nt, addend, o0, o1, ost, npoly,
                                  level, None)

    def tensor(w=pw, wr=LN, wc=EN, wp=L5, x0=px0, x1=px1, xr=LN, xc=EN, xp=L5, m=2, n=2, k=2, b=pb, br=LN, bc=EN,
               bp=L5, o0=p0, o1=p1, orow=LN, oc=EN, op=L5, npoly=2, level=5, flags=0):
        return lib.mfhe_ptmat_tensor(h, w, wr, wc, wp, x0, x1, xr, xc, xp, m, n, k, b, br, bc, bp, o0, o1, orow, oc, op,
                                     npoly, level, flags, None)

    def apply(w=pw, wr=LN, wc=EN, wp=L5, x0=px0, x1=px1, xr=LN, xc=EN, xp=L5, m=2, n=2, k=2, b=pb, br=LN, bc=EN,
              bp=L5, o0=p0, o1=p1, ost=L5, npoly=2, level=5, flags=0):
        return lib.mfhe_ptmat_apply(h, w, wr, wc, wp, x0, x1, xr, xc, xp, m, n, k, b, br, bc, bp, o0, o1, ost, npoly,
                                    level, flags, None)

    def reserve(m=2, n=2, npoly=2, level=5, flags=0):
        return lib.mfhe_ptmat_reserve(h, m, n, npoly, level, flags)

    cases = {
        "sum null x0": lambda: psum(x0=None),
        "sum null x1": lambda: psum(x1=None),
        "sum null pt": lambda: psum(pt=None),
        "sum null out0": lambda: psum(o0=None),
        "sum null out1": lambda: psum(o1=None),
        "sum null term_x": lambda: psum(tx=None),
        "sum null term_pt": lambda: psum(tp=None),
        "sum nterms 0": lambda: psum(nt=0),
        "sum nterms 65": lambda: psum(nt=65, tx=ints([0] * 65), tp=ints([0] * 65), npoly=0),
        "sum nsrc 0": lambda: psum(nsrc=0),
        "sum npt 0": lambda: psum(npt=0),
        "sum term_x out of range": lambda: psum(tx=ints([0, 2])),
        "sum term_x negative": lambda: psum(tx=ints([-1, 0])),
        "sum term_pt out of range": lambda: psum(tp=ints([2, 0])),
        "sum term_pt negative": lambda: psum(tp=ints([0, -1])),
        "sum addend -2": lambda: psum(addend=-2),
        "sum addend npt": lambda: psum(addend=2),
        "sum level 0": lambda: psum(level=0),
        "sum level outside": lambda: psum(level=8),
        "sum x poly stride": lambda: psum(xp=L5 - 1),
        "sum pt poly stride": lambda: psum(pp=L5 - 1),
        "sum out stride": lambda: psum(ost=L5 - 1),
        "sum source stride": lambda: psum(sst=EN - 1),
        "sum pt stride": lambda: psum(pst=EN - 1),
        "sum shared pt stride": lambda: psum(pp=0, pst=L5 - 1),
        "sum out0 is x0": lambda: psum(o0=px0),
        "sum out1 overlaps x1": lambda: psum(o1=px1 + 8 * (LN - 1)),
        "sum out0 is pt": lambda: psum(o0=pw),
        "sum out1 overlaps pt": lambda: psum(o1=pw + 8 * N),
        "sum out0 is out1": lambda: psum(o1=p0),
        "sum out1 overlaps out0": lambda: psum(o1=p0 + 8 * (EN - 1)),
        "tensor null w": lambda: tensor(w=None),
        "tensor null x0": lambda: tensor(x0=None),
        "tensor null x1": lambda: tensor(x1=None),
        "tensor null out0": lambda: tensor(o0=None),
        "tensor null out1": lambda: tensor(o1=None),
        "tensor m 0": lambda: tensor(m=0),
        "tensor n 0": lambda: tensor(n=0),
        "tensor m -1": lambda: tensor(m=-1),
        "tensor k 0": lambda: tensor(k=0),
        "tensor k 65": lambda: tensor(k=65, npoly=0),
        "tensor level 0": lambda: tensor(level=0),
        "tensor level outside": lambda: tensor(level=8),
        "tensor rescale flag": lambda: tensor(flags=1),
        "tensor unknown flag": lambda: tensor(flags=4),
        "tensor w poly stride": lambda: tensor(wp=L5 - 1),
        "tensor x poly stride": lambda: tensor(xp=L5 - 1),
        "tensor x poly stride 0": lambda: tensor(xp=0),
        "tensor bias poly stride": lambda: tensor(bp=L5 - 1),
        "tensor out poly stride": lambda: tensor(op=L5 - 1),
        "tensor out poly stride 0": lambda: tensor(op=0),
        "tensor w col stride": lambda: tensor(wc=EN - 1),
        "tensor w col stride 0": lambda: tensor(wc=0),
        "tensor w row stride": lambda: tensor(wr=LN - 1),
        "tensor w row stride 0": lambda: tensor(wr=0),
        "tensor w transposed row stride": lambda: tensor(wr=EN - 1, wc=LN),
        "tensor w equal strides": lambda: tensor(wr=EN, wc=EN),
        "tensor shared w col stride": lambda: tensor(wp=0, wc=L5 - 1, wr=2 * L5),
        "tensor x col stride": lambda: tensor(xc=EN - 1),
        "tensor x row stride": lambda: tensor(xr=LN - 1),
        "tensor x row stride 0": lambda: tensor(xr=0),
        "tensor x transposed col stride": lambda: tensor(xr=EN, xc=LN - 1),
        "tensor bias col stride": lambda: tensor(bc=EN - 1),
        "tensor bias row stride": lambda: tensor(br=LN - 1),
        "tensor out col stride": lambda: tensor(oc=EN - 1),
        "tensor out col stride 0": lambda: tensor(oc=0),
        "tensor out row stride": lambda: tensor(orow=LN - 1),
        "tensor out row stride 0": lambda: tensor(orow=0),
        "tensor out0 is w": lambda: tensor(o0=pw),
        "tensor out1 overlaps x1": lambda: tensor(o1=px1 + 8 * (2 * LN - 1)),
        "tensor out0 is x0": lambda: tensor(o0=px0),
        "tensor out1 is the bias": lambda: tensor(o1=pb),
        "tensor out0 overlaps a broadcast bias": lambda: tensor(o0=pb + 8 * (L5 - 1), br=0, bc=0, bp=0),
        "tensor out0 is out1": lambda: tensor(o1=p0),
        "tensor out1 overlaps out0": lambda: tensor(o1=p0 + 8 * (2 * LN - 1)),
        "apply null w": lambda: apply(w=None),
        "apply null x1": lambda: apply(x1=None),
        "apply null out0": lambda: apply(o0=None),
        "apply null out1": lambda: apply(o1=None),
        "apply m 0": lambda: apply(m=0),
        "apply n 0": lambda: apply(n=0),
        "apply k 0": lambda: apply(k=0),
        "apply k 65": lambda: apply(k=65, npoly=0),
        "apply level 0": lambda: apply(level=0),
        "apply level outside": lambda: apply(level=8),
        "apply w poly stride": lambda: apply(wp=L5 - 1),
        "apply w col stride": lambda: apply(wc=EN - 1),
        "apply x row stride": lambda: apply(xr=LN - 1),
        "apply bias col stride": lambda: apply(bc=EN - 1),
        "apply out stride": lambda: apply(ost=L5 - 1),
        "apply out0 is w": lambda: apply(o0=pw),
        "apply out1 overlaps x1": lambda: apply(o1=px1 + 8 * N),
        "apply out1 is the bias": lambda: apply(o1=pb),
        "apply out0 is out1": lambda: apply(o1=p0),
        "apply out1 overlaps out0": lambda: apply(o1=p0 + 8 * (2 * LN - 1)),
        "apply unknown flag": lambda: apply(flags=4),
        "apply rescale at level 1": lambda: apply(level=1, wp=N, wc=2 * N, wr=4 * N, xp=N, xc=2 * N, xr=4 * N, bp=N,
                                                  bc=2 * N, br=4 * N, ost=N, flags=1),
        "reserve m 0": lambda: reserve(m=0),
        "reserve n 0": lambda: reserve(n=0),
        "reserve level 0": lambda: reserve(level=0),
        "reserve level outside": lambda: reserve(level=8),
        "reserve unknown flag": lambda: reserve(flags=4),
        "reserve rescale at level 1": lambda: reserve(level=1, flags=1),
    }
    entry = {"sum": b"ptmul_sum", "tensor": b"ptmat_tensor", "apply": b"ptmat_apply", "reserve": b"ptmat_reserve"}
    for name, call in cases.items():
        assert lib.mfhe_ptmat_tile(None, None) == E            # leaves another entry point's message behind
        stale = lib.mfhe_last_error()
        assert call() == E, name
        msg = lib.mfhe_last_error()
        assert msg != stale and msg.startswith(entry[name.split()[0]] + b": "), (name, msg)
    # no polynomials: nothing to do, and nothing is launched
    assert psum(npoly=0) == mfhe.OK
    assert tensor(npoly=0) == mfhe.OK
    assert apply(npoly=0) == mfhe.OK
    assert apply(npoly=0, flags=3) == mfhe.OK
    # a context without the phantom tables
    plain = mfhe.Context(list(mod), 4, 0)
    hp = plain.handle
    R = mfhe.ENOTREADY
    assert lib.mfhe_ptmul_sum(hp, px0, px1, EN, L5, 2, pw, EN, L5, 2, T01, T01, 2, -1, p0, p1, L5, 2, 5, None) == R
    assert lib.mfhe_ptmat_tensor(hp, pw, LN, EN, L5, px0, px1, LN, EN, L5, 2, 2, 2, pb, LN, EN, L5, p0, p1, LN, EN, L5,
                                 2, 5, 0, None) == R
    assert lib.mfhe_ptmat_apply(hp, pw, LN, EN, L5, px0, px1, LN, EN, L5, 2, 2, 2, pb, LN, EN, L5, p0, p1, L5, 2, 5, 0,
                                None) == R
    assert lib.mfhe_ptmat_reserve(hp, 2, 2, 2, 5, 0) == R
    torch.cuda.synchronize()
    for name, b in bufs.items():   # nothing ran: every word is still the canary
        assert b.all_canary(), name
