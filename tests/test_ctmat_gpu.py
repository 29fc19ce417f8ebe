"""GPU checks of products of ciphertext matrices (csrc/ctmat.hip; include/mfhe.h mfhe_ctmat_tensor, mfhe_ctmat_apply,
mfhe_ctmat_reserve and the Python layer's ctmat_tensor / ctmat / ctmat_reserve), bit-exact: the tensor formulas in exact
integers computed here, m n calls of ctmul_tensor and ctmul, and the coefficient-domain model of tests/ctmul_model.py.
Every comparison is exact equality: the arithmetic is integer (ModDown's one f64 sum only selects the multiple of its
modulus and runs in a fixed order per coefficient, so the size of the batch does not enter it)."""
import numpy as np
import pytest

import ctmul_model as cm
import ks_model as km
from primes import primes_of_size
from test_ctmul_gpu import _tensor_int
from test_keyswitch_gpu import (CANARY, KS_CASES, LAYOUTS, _Blocks, _ctx, _device_key, _moduli, _polys, _random_rows,
                                _residues, _row_limbs, _u64)

pytestmark = pytest.mark.gpu

CLASSES = pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
LOGNS = pytest.mark.parametrize("log_n", [4, 10])
FOLD = 8     # csrc/ctmul.hpp kCtmulFold: the sums are reduced every 8 terms
# a full tile, an edge in each dimension alone and in both, degenerate rows and columns, both sides of the fold at 8
# and 16 and the largest sum (the tile is 2 x 2)
SHAPES = [(1, 1, 1), (2, 2, 1), (3, 2, 7), (2, 3, 8), (5, 5, 9), (1, 4, 17), (4, 1, 64)]
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


class _Matrix(_Blocks):
    """x [R][C][P][level][n] (its first npoly polynomials; None: canaries, an output) on the device, `off` words into a
    canary-filled allocation: polynomials level n + ppad apart, the entries of a line npoly of those + ipad apart and
    the lines one line + opad apart.  A line is a row, or with `transposed` a column (col stride > row stride)."""

    def __init__(self, mfhe, R, C, npoly, level, n, ppad, ipad, opad, off, x=None, transposed=False):
        self.pst = level * n + ppad
        inner = npoly * self.pst + ipad
        if transposed:
            self.rs, self.cs = inner, R * inner + opad
        else:
            self.cs, self.rs = inner, C * inner + opad
        self.shape = (R, C, npoly, level, n)
        self.src = None if x is None else np.ascontiguousarray(x[:R, :C, :npoly])
        offsets = [r * self.rs + c * self.cs + p * self.pst for r in range(R) for c in range(C) for p in range(npoly)]
        super().__init__(mfhe, offsets, level * n, off, self.src)
        self.strides = (self.rs, self.cs, self.pst)

    def get(self):
        return self.blocks(self.shape)


def _add_products(acc, x, y):
    """acc (four uint64 arrays of 32-bit limbs with headroom) += x y, exactly."""
    x0, x1, y0, y1 = x & M32, x >> S32, y & M32, y >> S32
    p00, p01, p10, p11 = x0 * y0, x0 * y1, x1 * y0, x1 * y1
    acc[0] += p00 & M32
    acc[1] += (p00 >> S32) + (p01 & M32) + (p10 & M32)
    acc[2] += (p01 >> S32) + (p10 >> S32) + (p11 & M32)
    acc[3] += p11 >> S32


def _limbs_mod(acc, q):
    """The integer acc[0] + 2^32 acc[1] + 2^64 acc[2] + 2^96 acc[3] mod q (an object array that broadcasts)."""
    v = acc[0].astype(object)
    for k in (1, 2, 3):
        v = v + (acc[k].astype(object) << (32 * k))
    return (v % q).astype(np.uint64)


def _matprod_int(a0, a1, b0, b1, moduli, m, n, k):
    """(d0, d1, d2), each [m][n][P][level][N] uint64, of the m x k by k x n product of a [>= m][>= k][P][level][N] and
    b [>= k][>= n][P][level][N] in exact integers: every product is summed in 32-bit limbs (at most 128 products of
    residues below 2^62: no limb exceeds 2^41) and the sum reduced once."""
    q = np.array([int(v) for v in moduli], dtype=object)[:, None]
    shape = (m, n) + a0.shape[2:]
    s = [[np.zeros(shape, np.uint64) for _ in range(4)] for _ in range(3)]
    for t in range(k):
        x0, x1 = a0[:m, t][:, None], a1[:m, t][:, None]
        y0, y1 = b0[t, :n][None], b1[t, :n][None]
        _add_products(s[0], x0, y0)
        _add_products(s[1], x0, y1)
        _add_products(s[1], x1, y0)
        _add_products(s[2], x1, y1)
    return tuple(_limbs_mod(acc, q) for acc in s)


def test_the_limb_reference_equals_python_integers():
    """The reference of this file against the Python integers of tests/test_ctmul_gpu.py (no device code runs)."""
    mod, n = _moduli(4, (50, 61)), 16
    rng = np.random.default_rng(3)
    a0, a1 = (_random_rows(rng, (2, 17, 2), mod[:3], n) for _ in range(2))
    b0, b1 = (_random_rows(rng, (17, 2, 2), mod[:3], n) for _ in range(2))
    got = _matprod_int(a0, a1, b0, b1, mod[:3], 2, 2, 17)
    for i in range(2):
        for j in range(2):
            want = _tensor_int(a0[i], a1[i], b0[:, j], b1[:, j], mod[:3], [17])[17]
            for c in range(3):
                np.testing.assert_array_equal(got[c][i, j], want[c])


# ---------------------------------------------------------------------------------------------------------------
# 1. the tiled tensor sum against exact integers
# ---------------------------------------------------------------------------------------------------------------
def _run_tensor(mfhe, ctx, A0, A1, B0, B1, m, n, k, npoly, level, N, ppad, off):
    """One call on prepared operands; returns the three outputs (d0, d1 share their strides, d2 has its own)."""
    import torch
    o0 = _Matrix(mfhe, m, n, npoly, level, N, ppad, 2, 4, off)
    o1 = _Matrix(mfhe, m, n, npoly, level, N, ppad, 2, 4, off)
    o2 = _Matrix(mfhe, m, n, npoly, level, N, ppad + 2, 0, 6, off)
    ctx.ctmat_tensor(A0.t, A1.t, B0.t, B1.t, o0.t, o1.t, o2.t, m, n, k, npoly, level, a_strides=A0.strides,
                     b_strides=B0.strides, d01_strides=o0.strides, d2_strides=o2.strides)
    torch.cuda.synchronize()
    return o0, o1, o2


@CLASSES
@LOGNS
def test_tensor_bit_exact(mfhe, log_n, bits):
    """Every shape of SHAPES in the 16-byte form (dense, padded) and the scalar one (padded-odd, misaligned), A and B
    at different strides, 1 and 3 polynomials, and once with B stored transposed; the pads around every output entry
    stay canaries and the inputs are unchanged.  1 x 1 products also equal ctmul_tensor bit for bit."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(60 + log_n)
    level, P = (3, 3) if log_n == 4 else (2, 3)
    R, K, C = max(s[0] for s in SHAPES), max(s[2] for s in SHAPES), max(s[1] for s in SHAPES)
    a0, a1 = (_random_rows(rng, (R, K, P), mod[:level], N) for _ in range(2))
    b0, b1 = (_random_rows(rng, (K, C, P), mod[:level], N) for _ in range(2))
    want = {s: _matprod_int(a0, a1, b0, b1, mod[:level], *s) for s in SHAPES + [(1, 1, 17)]}
    runs = [layout + (False,) for layout in LAYOUTS] + [("dense, B transposed", 0, 0, 0, True)]
    for name, ppad, tpad, off, tr in runs:
        for npoly in ((1, 3) if name in ("dense", "misaligned") else (3,)):
            A0, A1 = (_Matrix(mfhe, R, K, npoly, level, N, ppad, tpad, tpad, off, x) for x in (a0, a1))
            B0, B1 = (_Matrix(mfhe, K, C, npoly, level, N, ppad + 2, tpad + 2, tpad, off, x, tr) for x in (b0, b1))
            assert A0.strides != B0.strides and (B0.cs > B0.rs) == tr
            for m, n, k in SHAPES + [(1, 1, 17)]:
                outs = _run_tensor(mfhe, ctx, A0, A1, B0, B1, m, n, k, npoly, level, N, ppad, off)
                for c, o in enumerate(outs):
                    np.testing.assert_array_equal(o.get(), want[m, n, k][c][:, :, :npoly],
                                                  err_msg=f"d{c} {name} npoly {npoly} shape {(m, n, k)}")
                    o.check_pads()
                if (m, n) == (1, 1):                          # one dot product: ctmul_tensor's result
                    e = [_polys(mfhe, npoly, level, N, 0, off) for _ in range(3)]
                    ctx.ctmul_tensor(A0.t, A1.t, B0.t, B1.t, e[0].t, e[1].t, e[2].t, npoly, level, k,
                                     a_term_stride=A0.cs, a_poly_stride=A0.pst, b_term_stride=B0.rs,
                                     b_poly_stride=B0.pst)
                    torch.cuda.synchronize()
                    for c in range(3):
                        np.testing.assert_array_equal(outs[c].get()[0, 0], e[c].blocks((npoly, level, N)),
                                                      err_msg=f"d{c} against ctmul_tensor, {name} k {k}")
            for blk in (A0, A1, B0, B1):                      # the inputs are untouched
                np.testing.assert_array_equal(blk.get(), blk.src, err_msg=name)
                blk.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 2. the fold boundary at the worst case
# ---------------------------------------------------------------------------------------------------------------
def test_tensor_of_all_q_minus_1_with_62_bit_primes(mfhe):
    """Every operand q - 1 with 62-bit primes, a 3 x 3 product (a full tile and every edge tile): each product is just
    below 2^124 and d1 takes two per term, so 8 terms are 16 maximal products in one u128 and the ninth overflows it
    unless the sums were reduced after 8.  (q - 1)^2 = 1 mod q: d0 = d2 = k, d1 = 2 k."""
    mod = primes_of_size(62, 32, 3)
    assert len(mod) == 3 and all(2 ** 61 < v < 2 ** 62 for v in mod)
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    N, level, npoly, K = 16, 3, 2, 64
    top = _u64(mod) - np.uint64(1)
    xa = np.broadcast_to(top[None, None, None, :, None], (3, K, npoly, level, N)).copy()
    xb = np.broadcast_to(top[None, None, None, :, None], (K, 3, npoly, level, N)).copy()
    for name, ppad, tpad, off in (LAYOUTS[0], LAYOUTS[3]):   # the 16-byte and the scalar form
        A0, A1 = (_Matrix(mfhe, 3, K, npoly, level, N, ppad, tpad, tpad, off, xa) for _ in range(2))
        B0, B1 = (_Matrix(mfhe, K, 3, npoly, level, N, ppad, tpad, tpad, off, xb) for _ in range(2))
        for k in (FOLD, FOLD + 1, 2 * FOLD, 2 * FOLD + 1, 64):
            outs = _run_tensor(mfhe, ctx, A0, A1, B0, B1, 3, 3, k, npoly, level, N, ppad, off)
            for c, o in enumerate(outs):
                assert (o.get() == np.uint64(2 * k if c == 1 else k)).all(), f"d{c} {name} k {k}"
                o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 3. more tiles x polynomials than grid z holds
# ---------------------------------------------------------------------------------------------------------------
def test_tensor_folds_work_items_over_grid_z(mfhe):
    """A 2 x 2 product (one tile) of 65538 polynomials of one 16-word row: grid z is 65535, so work items 0, 1 and 2
    share their blocks with 65535, 65536 and 65537.  Operands below 2^31 keep the two-product sums of one term below
    2^63: the expected values are uint64 arithmetic."""
    import torch
    bits, log_n = (50, 61), 4
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 16
    npoly, level, m, n = 65538, 1, 2, 2
    rng = np.random.default_rng(63)
    a0, a1 = (rng.integers(0, 2 ** 31, (m, 1, npoly, level, N), dtype=np.uint64) for _ in range(2))
    b0, b1 = (rng.integers(0, 2 ** 31, (1, n, npoly, level, N), dtype=np.uint64) for _ in range(2))
    q = np.uint64(mod[0])
    assert int(q) < 2 ** 62
    x0, x1, y0, y1 = a0[:, 0][:, None], a1[:, 0][:, None], b0[0][None], b1[0][None]
    want = ((x0 * y0) % q, (x0 * y1 + x1 * y0) % q, (x1 * y1) % q)       # each [m][n][npoly][1][N]
    dev = [mfhe.to_device_u64(x.ravel()) for x in (a0, a1, b0, b1)]
    outs = [_polys(mfhe, m * n * npoly, level, N) for _ in range(3)]
    ctx.ctmat_tensor(dev[0], dev[1], dev[2], dev[3], outs[0].t, outs[1].t, outs[2].t, m, n, 1, npoly, level)
    torch.cuda.synchronize()
    for c, o in enumerate(outs):
        got = o.blocks((m, n, npoly, level, N))
        for i in range(m):
            for j in range(n):
                bad = np.flatnonzero((got[i, j] != want[c][i, j]).reshape(npoly, -1).any(axis=1))
                assert bad.size == 0, f"d{c}[{i}][{j}]: {bad.size} wrong polynomials, the first {bad[:8].tolist()}"
        o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 4. the driver against m n calls of ctmul
# ---------------------------------------------------------------------------------------------------------------
def _check_against_separate_products(mfhe, ctx, mod, rng, rlk, m, n, k, npoly, level, key_level, alpha, sp, nsp, opad):
    """ctmat on fresh random operands against m n calls of ctmul, one per entry, with the same flags (with
    CTMUL_RESCALE rows [0, level - 1) are compared); the outputs lie opad words apart and their pads stay canaries.
    (tests/test_client_shapes_gpu.py runs it where the NTT plan changes.)"""
    import torch
    N = ctx.N
    lw = level * N
    a0, a1 = (_random_rows(rng, (m, k, npoly), mod[:level], N) for _ in range(2))
    b0, b1 = (_random_rows(rng, (k, n, npoly), mod[:level], N) for _ in range(2))
    A0, A1 = (_Matrix(mfhe, m, k, npoly, level, N, 2, 4, 2, 0, x) for x in (a0, a1))
    B0, B1 = (_Matrix(mfhe, k, n, npoly, level, N, 0, 6, 0, 0, x) for x in (b0, b1))
    for flags in (0, mfhe.CTMUL_RESCALE):
        keep = level - 1 if flags else level
        msg = f"alpha {alpha} K {nsp} level {level} flags {flags}"
        o0, o1 = (_polys(mfhe, m * n * npoly, level, N, opad) for _ in range(2))
        ctx.ctmat(A0.t, A1.t, B0.t, B1.t, rlk, o0.t, o1.t, m, n, k, npoly, level, key_level, alpha, sp, nsp,
                  flags, a_strides=A0.strides, b_strides=B0.strides, out_stride=o0.stride)
        torch.cuda.synchronize()
        got = [o.blocks((m, n, npoly, level, N)) for o in (o0, o1)]
        for o in (o0, o1):
            o.check_pads()
        for i in range(m):
            for j in range(n):
                e0, e1 = (torch.zeros(npoly * lw, dtype=torch.int64, device="cuda") for _ in range(2))
                ctx.ctmul(A0.t[i * A0.rs:], A1.t[i * A1.rs:], B0.t[j * B0.cs:], B1.t[j * B1.cs:], rlk, e0, e1,
                          npoly, level, key_level, alpha, sp, nsp, k, flags, a_term_stride=A0.cs,
                          a_poly_stride=A0.pst, b_term_stride=B0.rs, b_poly_stride=B0.pst)
                torch.cuda.synchronize()
                for c, e in enumerate((e0, e1)):
                    np.testing.assert_array_equal(
                        got[c][i, j][:, :keep], mfhe.to_host_u64(e).reshape(npoly, level, N)[:, :keep],
                        err_msg=f"out{c}[{i}][{j}] " + msg)
    for blk in (A0, A1, B0, B1):
        np.testing.assert_array_equal(blk.get(), blk.src)
        blk.check_pads()


@CLASSES
@LOGNS
def test_ctmat_equals_the_separate_products(mfhe, log_n, bits):
    """ctmat of a 2 x 3 product of 3 terms and 2 polynomials = six calls of ctmul, one per entry, on the same operands
    with the same flags (with CTMUL_RESCALE rows [0, level - 1) are compared); the pads of the outputs stay canaries."""
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(70 + log_n)
    m, n, k, npoly = 2, 3, 3, 2
    for key_level, alpha, sp, nsp, levels in KS_CASES:
        kmod = [mod[l] for l in _row_limbs(key_level, sp, nsp)]
        rlk = mfhe.to_device_u64(_random_rows(rng, (-(-key_level // alpha), 2), kmod, N).ravel())
        for level in levels:
            _check_against_separate_products(mfhe, ctx, mod, rng, rlk, m, n, k, npoly, level, key_level, alpha, sp, nsp,
                                              2 if log_n == 10 else 3)


# ---------------------------------------------------------------------------------------------------------------
# 5. the driver against the coefficient-domain model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
def test_ctmat_equals_the_model(mfhe, bits):
    """N = 16, the seeded ciphertexts of tests/ctmul_model.py as a 2 x 3 matrix A and a 3 x 2 matrix B (six each): the
    product on the device, back through ntt_inv, equals the model's product of row i and column j residue for residue
    at levels 5, 3 and 2, with and without rescale, and every entry decrypts within the model's bound."""
    import torch
    cs = km.seeded_case(bits, "relin", True)
    q, p, N, alpha, s, s2 = cs["q"], cs["p"], cs["n"], cs["alpha"], cs["s_to"], cs["s_from"]
    ctx = mfhe.Context(q + p, 4, mfhe.CONV_PHANTOM)
    rlk = _device_key(mfhe, ctx, cs)
    m, n, k = 2, 2, 3
    for level in cm.LEVELS:
        Ql = km.prod(q[:level])
        _, cts_a, cts_b, _, _ = cm.seeded_inputs(bits, level, m * k, False)
        A = [[cts_a[i * k + t] for t in range(k)] for i in range(m)]          # A[i][t]
        B = [[cts_b[t * n + j] for j in range(n)] for t in range(k)]          # B[t][j]

        def device(cts, comp):   # dense [len(cts)][1][level][N]
            res = _residues([ct[comp] for ct in cts], q[:level])
            return ctx.ntt_fwd(mfhe.to_device_u64(res.ravel()), len(cts), 0, level)

        a0, a1 = device(cts_a, 0), device(cts_a, 1)
        b0, b1 = device(cts_b, 0), device(cts_b, 1)
        for flags in (0, mfhe.CTMUL_RESCALE):
            keep = level - 1 if flags else level
            o0 = torch.zeros(m * n * level * N, dtype=torch.int64, device="cuda")
            o1 = torch.zeros(m * n * level * N, dtype=torch.int64, device="cuda")
            ctx.ctmat(a0, a1, b0, b1, rlk, o0, o1, m, n, k, 1, level, 5, alpha, 5, 2, flags)
            for e in range(m * n):
                ctx.ntt_inv(o0[e * level * N:], 1, 0, keep)
                ctx.ntt_inv(o1[e * level * N:], 1, 0, keep)
            torch.cuda.synchronize()
            h = [mfhe.to_host_u64(o).reshape(m, n, level, N) for o in (o0, o1)]
            for i in range(m):
                for j in range(n):
                    res = cm.product(q, p, alpha, level, A[i], [B[t][j] for t in range(k)], cs["key"], bool(flags))
                    assert res["margin"] >= 2.0 ** -30, "pick another seed: a remainder sits at a tie"
                    msg = f"level {level} flags {flags} entry ({i}, {j})"
                    for c in range(2):
                        np.testing.assert_array_equal(h[c][i, j][:keep], _residues([res["out"][c]], q[:keep])[0],
                                                      err_msg=f"out{c} " + msg)
                    err = cm.decryption_error(q, level, res, s, s2, bool(flags))
                    bnd = cm.bound(q, p, alpha, level, N, bool(flags))
                    print(f"ctmat bits {bits} {msg}: error / bound = {err / bnd:.4f}")
                    assert err <= bnd and bnd < Ql // 4


# ---------------------------------------------------------------------------------------------------------------
# 6. graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After ctmat_reserve, ctmat allocates nothing and copies nothing to the device: it is captured into a graph on
    one stream (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed twice on changed inputs;
    each replay equals the eager call on those inputs."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, N = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    m, n, k, npoly, level, key_level, alpha, sp, nsp = 3, 2, 3, 2, 5, 5, 2, 5, 2
    flags = mfhe.CTMUL_RESCALE
    ctx.ctmat_reserve(m, n, npoly, level, key_level, alpha, sp, nsp, flags)
    rng = np.random.default_rng(9)
    rlk = mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, N).ravel())
    lead = [(m, k, npoly), (m, k, npoly), (k, n, npoly), (k, n, npoly)]
    ops = [mfhe.to_device_u64(_random_rows(rng, l, mod[:level], N).ravel()) for l in lead]
    words = m * n * npoly * level * N
    o0 = torch.zeros(words, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(words, dtype=torch.int64, device="cuda")

    def apply(x0, x1):
        ctx.ctmat(ops[0], ops[1], ops[2], ops[3], rlk, x0, x1, m, n, k, npoly, level, key_level, alpha, sp, nsp, flags)

    def kept(t):
        return mfhe.to_host_u64(t).reshape(m * n * npoly, level, N)[:, :level - 1].copy()

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        apply(o0, o1)
    first = None
    for _ in range(2):                                         # the captured inputs, then fresh ones
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
# 7. argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    mod, N = _moduli(4, (45, 49)), 16
    ctx = mfhe.Context(list(mod), 4, mfhe.CONV_PHANTOM)
    h = ctx.handle
    names = ("a0", "a1", "b0", "b1", "o0", "o1", "o2", "key")
    bufs = {name: _polys(mfhe, 1, 3 * 2 * 7, N) for name in names}
    pa0, pa1, pb0, pb1, p0, p1, p2, pk = (bufs[name].t.data_ptr() for name in names)
    E = mfhe.EINVAL
    L5 = 5 * N          # a polynomial at level 5
    EN = 2 * L5         # an entry: 2 polynomials
    LN = 2 * EN         # a line of 2 entries; every matrix here is 2 x 2, 4 EN = 640 of the buffers' 672 words

    def tensor(a0=pa0, a1=pa1, ar=LN, ac=EN, ap=L5, b0=pb0, b1=pb1, br=LN, bc=EN, bp=L5, m=2, n=2, k=2, d0=p0, d1=p1,
               dr=LN, dc=EN, dp=L5, d2=p2, d2r=LN, d2c=EN, d2p=L5, npoly=2, level=5):
        return lib.mfhe_ctmat_tensor(h, a0, a1, ar, ac, ap, b0, b1, br, bc, bp, m, n, k, d0, d1, dr, dc, dp, d2, d2r,
                                     d2c, d2p, npoly, level, None)

    def apply(a0=pa0, a1=pa1, ar=LN, ac=EN, ap=L5, b0=pb0, b1=pb1, br=LN, bc=EN, bp=L5, m=2, n=2, k=2, key=pk, o0=p0,
              o1=p1, ost=L5, npoly=2, level=5, kl=5, alpha=2, sp=5, nsp=2, flags=0):
        return lib.mfhe_ctmat_apply(h, a0, a1, ar, ac, ap, b0, b1, br, bc, bp, m, n, k, key, o0, o1, ost, npoly, level,
                                    kl, alpha, sp, nsp, flags, None)

    def reserve(m=2, n=2, npoly=2, level=5, kl=5, alpha=2, sp=5, nsp=2, flags=0):
        return lib.mfhe_ctmat_reserve(h, m, n, npoly, level, kl, alpha, sp, nsp, flags)

    cases = {
        "tensor null a0": lambda: tensor(a0=None),
        "tensor null a1": lambda: tensor(a1=None),
        "tensor null b0": lambda: tensor(b0=None),
        "tensor null b1": lambda: tensor(b1=None),
        "tensor null both b": lambda: tensor(b0=None, b1=None),
        "tensor null d0": lambda: tensor(d0=None),
        "tensor null d1": lambda: tensor(d1=None),
        "tensor null d2": lambda: tensor(d2=None),
        "tensor m 0": lambda: tensor(m=0),
        "tensor n 0": lambda: tensor(n=0),
        "tensor m -1": lambda: tensor(m=-1),
        "tensor k 0": lambda: tensor(k=0),
        "tensor k 65": lambda: tensor(k=65, npoly=0),
        "tensor level 0": lambda: tensor(level=0),
        "tensor level outside": lambda: tensor(level=8),
        "tensor a poly stride": lambda: tensor(ap=L5 - 1),
        "tensor b poly stride": lambda: tensor(bp=L5 - 1),
        "tensor d01 poly stride": lambda: tensor(dp=L5 - 1),
        "tensor d2 poly stride": lambda: tensor(d2p=L5 - 1),
        "tensor a col stride": lambda: tensor(ac=EN - 1),
        "tensor a row stride": lambda: tensor(ar=LN - 1),
        "tensor a transposed row stride": lambda: tensor(ar=EN - 1, ac=LN),
        "tensor a transposed col stride": lambda: tensor(ar=EN, ac=LN - 1),
        "tensor a equal strides": lambda: tensor(ar=EN, ac=EN),
        "tensor b col stride": lambda: tensor(bc=EN - 1),
        "tensor b row stride": lambda: tensor(br=LN - 1),
        "tensor b transposed col stride": lambda: tensor(br=EN, bc=LN - 1),
        "tensor d01 col stride": lambda: tensor(dc=EN - 1),
        "tensor d01 row stride": lambda: tensor(dr=LN - 1),
        "tensor d2 col stride": lambda: tensor(d2c=EN - 1),
        "tensor d2 row stride": lambda: tensor(d2r=LN - 1),
        "tensor d2 transposed row stride": lambda: tensor(d2r=EN - 1, d2c=LN),
        "tensor d0 is a0": lambda: tensor(d0=pa0),
        "tensor d1 overlaps a1": lambda: tensor(d1=pa1 + 8 * (2 * LN - 1)),
        "tensor d2 is b0": lambda: tensor(d2=pb0),
        "tensor d2 overlaps b1": lambda: tensor(d2=pb1 + 8 * N),
        "tensor d0 is d1": lambda: tensor(d1=p0),
        "tensor d2 overlaps d0": lambda: tensor(d2=p0 + 8 * (2 * LN - 1)),
        "apply null a0": lambda: apply(a0=None),
        "apply null b1": lambda: apply(b1=None),
        "apply null out0": lambda: apply(o0=None),
        "apply null out1": lambda: apply(o1=None),
        "apply null key": lambda: apply(key=None),
        "apply m 0": lambda: apply(m=0),
        "apply n 0": lambda: apply(n=0),
        "apply k 0": lambda: apply(k=0),
        "apply k 65": lambda: apply(k=65, npoly=0),
        "apply a poly stride": lambda: apply(ap=L5 - 1),
        "apply a col stride": lambda: apply(ac=EN - 1),
        "apply b row stride": lambda: apply(br=LN - 1),
        "apply out stride": lambda: apply(ost=L5 - 1),
        "apply out0 is a0": lambda: apply(o0=pa0),
        "apply out1 overlaps b1": lambda: apply(o1=pb1 + 8 * N),
        "apply out0 is out1": lambda: apply(o1=p0),
        "apply out1 overlaps out0": lambda: apply(o1=p0 + 8 * (2 * LN - 1)),
        "apply out1 is the key": lambda: apply(o1=pk),
        "apply unknown flag": lambda: apply(flags=2),
        "apply rescale at level 1": lambda: apply(level=1, ap=N, ac=2 * N, ar=4 * N, bp=N, bc=2 * N, br=4 * N, ost=N,
                                                  flags=1),
        "apply alpha < 1": lambda: apply(alpha=0),
        "apply nspecial < 1": lambda: apply(nsp=0),
        "apply level > key_level": lambda: apply(kl=4),
        "apply level < 1": lambda: apply(level=0),
        "apply special overlaps Q": lambda: apply(sp=4),
        "apply special outside": lambda: apply(sp=6),
        "reserve m 0": lambda: reserve(m=0),
        "reserve n 0": lambda: reserve(n=0),
        "reserve unknown flag": lambda: reserve(flags=2),
        "reserve rescale at level 1": lambda: reserve(level=1, flags=1),
        "reserve alpha < 1": lambda: reserve(alpha=0),
        "reserve nspecial < 1": lambda: reserve(nsp=0),
        "reserve level > key_level": lambda: reserve(kl=4),
        "reserve special outside": lambda: reserve(sp=6),
    }
    for name, call in cases.items():
        assert call() == E, name
        assert lib.mfhe_last_error(), name
    # no polynomials: nothing to do, and nothing is launched
    assert tensor(npoly=0) == mfhe.OK
    assert apply(npoly=0) == mfhe.OK
    # a context without the phantom tables
    plain = mfhe.Context(list(mod), 4, 0)
    hp = plain.handle
    R = mfhe.ENOTREADY
    assert lib.mfhe_ctmat_tensor(hp, pa0, pa1, LN, EN, L5, pb0, pb1, LN, EN, L5, 2, 2, 2, p0, p1, LN, EN, L5, p2, LN,
                                 EN, L5, 2, 5, None) == R
    assert lib.mfhe_ctmat_apply(hp, pa0, pa1, LN, EN, L5, pb0, pb1, LN, EN, L5, 2, 2, 2, pk, p0, p1, L5, 2, 5, 5, 2, 5,
                                2, 0, None) == R
    assert lib.mfhe_ctmat_reserve(hp, 2, 2, 2, 5, 5, 2, 5, 2, 0) == R
    torch.cuda.synchronize()
    for name, b in bufs.items():   # nothing ran: every word is still the canary
        assert b.all_canary(), name
