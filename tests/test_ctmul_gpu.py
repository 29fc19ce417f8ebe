"""GPU checks of ciphertext products (csrc/ctmul.hip; include/mfhe.h mfhe_ctmul_tensor, mfhe_ctmul_apply,
mfhe_ctmul_reserve and the Python layer's ctmul_tensor / ctmul / ctmul_reserve), bit-exact against Python integers:
the tensor formulas computed here, the composition of the public pieces, and the coefficient-domain model of
tests/ctmul_model.py.  Every comparison is exact equality: the arithmetic is integer (ModDown's one f64 sum only
selects the multiple of its modulus; tests/test_ctmul_cpu.py shows the model's seeded inputs stay 2^-30 of it away
from where it could flip, against the documented 2^-40)."""
import numpy as np
import pytest

import ctmul_model as cm
import ks_model as km
from primes import primes_of_size
from test_keyswitch_gpu import (CANARY, KS_CASES, LAYOUTS, _Blocks, _ctx, _device_key, _moduli, _polys, _random_rows,
                                _residues, _row_limbs, _u64)

pytestmark = pytest.mark.gpu

CLASSES = pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
LOGNS = pytest.mark.parametrize("log_n", [4, 10])
UNROLL = 6   # csrc/ctmul.hip kCtmulUnroll: term counts 1 .. 6 have their own instantiation
FOLD = 8     # csrc/ctmul.hip kCtmulFold: the chunked loop reduces its sums every 8 terms
TENSOR_TERMS = list(range(1, UNROLL + 2)) + [8, 9, 16, 17, 64]


def _operand(mfhe, x, npoly, ppad, tpad, off):
    """The first npoly polynomials of every term of x [T][P][level][n] on the device, polynomials level n + ppad and
    terms npoly (level n + ppad) + tpad words apart, `off` words into a canary-filled allocation."""
    nt, _, level, n = x.shape
    pst = level * n + ppad
    tst = npoly * pst + tpad
    src = np.ascontiguousarray(x[:, :npoly])
    b = _Blocks(mfhe, [t * tst + p * pst for t in range(nt) for p in range(npoly)], level * n, off, src)
    b.tst, b.pst, b.src = tst, pst, src
    return b


def _tensor_int(a0, a1, b0, b1, moduli, terms):
    """{T: (d0, d1, d2)} for every T in `terms`, each [P][level][n] uint64, in Python integers; b0 None: the square."""
    q = np.array([int(m) for m in moduli], dtype=object)[None, :, None]
    x0, x1 = a0.astype(object), a1.astype(object)
    y0, y1 = (x0, x1) if b0 is None else (b0.astype(object), b1.astype(object))
    s = [0, 0, 0]
    out = {}
    for t in range(max(terms)):
        s[0] = s[0] + x0[t] * y0[t]
        s[1] = s[1] + x0[t] * y1[t] + x1[t] * y0[t]
        s[2] = s[2] + x1[t] * y1[t]
        if t + 1 in terms:
            out[t + 1] = tuple((v % q).astype(np.uint64) for v in s)
    return out


def _run_tensor(mfhe, ctx, A0, A1, B0, B1, nterms, npoly, level, n, ppad, off):
    """One call on prepared operand blocks; returns the three output blocks (d0, d1 share a stride, d2 has its own)."""
    import torch
    o0 = _polys(mfhe, npoly, level, n, ppad, off)
    o1 = _polys(mfhe, npoly, level, n, ppad, off)
    o2 = _polys(mfhe, npoly, level, n, ppad + 2, off)
    ctx.ctmul_tensor(A0.t, A1.t, None if B0 is None else B0.t, None if B1 is None else B1.t, o0.t, o1.t, o2.t, npoly,
                     level, nterms, a_term_stride=A0.tst, a_poly_stride=A0.pst,
                     b_term_stride=None if B0 is None else B0.tst, b_poly_stride=None if B0 is None else B0.pst,
                     d01_stride=o0.stride, d2_stride=o2.stride)
    torch.cuda.synchronize()
    return o0, o1, o2


# ---------------------------------------------------------------------------------------------------------------
# 1. the tensor sum against Python integers
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_tensor_bit_exact(mfhe, log_n, bits):
    """Every term count with its own instantiation, the first of the chunked loop, both sides of its fold at 8 and 16
    and the largest, general and square, in the 16-byte form (dense, padded) and the scalar one (padded-odd,
    misaligned), A and B at different strides, 1 and 3 polynomials."""
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(40 + log_n)
    level, P, T = (3, 3, 64) if log_n == 4 else (2, 3, 64)
    a0, a1, b0, b1 = (_random_rows(rng, (T, P), mod[:level], n) for _ in range(4))
    want = {False: _tensor_int(a0, a1, b0, b1, mod[:level], TENSOR_TERMS),
            True: _tensor_int(a0, a1, None, None, mod[:level], TENSOR_TERMS)}
    for name, ppad, tpad, off in LAYOUTS:
        for npoly in ((1, 3) if name in ("dense", "misaligned") else (3,)):
            A0, A1 = (_operand(mfhe, x, npoly, ppad, tpad, off) for x in (a0, a1))
            B0, B1 = (_operand(mfhe, x, npoly, ppad + 2, tpad + 2, off) for x in (b0, b1))
            assert (A0.tst, A0.pst) != (B0.tst, B0.pst)
            for square in (False, True):
                for nt in TENSOR_TERMS:
                    outs = _run_tensor(mfhe, ctx, A0, A1, None if square else B0, None if square else B1, nt, npoly,
                                       level, n, ppad, off)
                    for k, o in enumerate(outs):
                        np.testing.assert_array_equal(
                            o.blocks((npoly, level, n)), want[square][nt][k][:npoly],
                            err_msg=f"d{k} {name} npoly {npoly} nterms {nt} square {square}")
                        o.check_pads()
            for blk in (A0, A1, B0, B1):                      # the inputs are untouched
                np.testing.assert_array_equal(blk.blocks(blk.src.shape), blk.src, err_msg=name)
                blk.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 2. the fold boundary at the worst case
# ---------------------------------------------------------------------------------------------------------------
def test_tensor_of_all_q_minus_1_with_62_bit_primes(mfhe):
    """Every operand q - 1 with 62-bit primes: each product is just below 2^124 and d1 takes two per term, so 8 terms
    are 16 maximal products in one u128 and the ninth overflows it unless the sums were reduced after 8; the square
    form doubles its 8.  (q - 1)^2 = 1 mod q: d0 = d2 = T, d1 = 2 T."""
    mod = primes_of_size(62, 32, 3)
    assert len(mod) == 3 and all(2 ** 61 < m < 2 ** 62 for m in mod)
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    n, level, npoly, T = 16, 3, 2, 64
    top = _u64(mod) - np.uint64(1)
    x = np.broadcast_to(top[None, None, :, None], (T, npoly, level, n)).copy()
    for name, ppad, tpad, off in (LAYOUTS[0], LAYOUTS[3]):   # the 16-byte and the scalar form
        A0, A1, B0, B1 = (_operand(mfhe, x, npoly, ppad, tpad, off) for _ in range(4))
        for square in (False, True):
            for nt in (FOLD, FOLD + 1, 2 * FOLD, 2 * FOLD + 1, 64):
                outs = _run_tensor(mfhe, ctx, A0, A1, None if square else B0, None if square else B1, nt, npoly,
                                   level, n, ppad, off)
                for k, o in enumerate(outs):
                    got = o.blocks((npoly, level, n))
                    assert (got == np.uint64(2 * nt if k == 1 else nt)).all(), f"d{k} {name} nterms {nt} square {square}"
                    o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 3. more polynomials than grid z holds
# ---------------------------------------------------------------------------------------------------------------
def test_tensor_folds_polynomials_over_grid_z(mfhe):
    """65538 polynomials of one 16-word row: grid z is 65535, so polynomials 0, 1 and 2 share their blocks with
    65535, 65536 and 65537."""
    import torch
    bits, log_n = (50, 61), 4
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 16
    npoly, level = 65538, 1
    rng = np.random.default_rng(43)
    a0, a1, b0, b1 = (_random_rows(rng, (1, npoly), mod[:level], n) for _ in range(4))
    dev = [mfhe.to_device_u64(x.ravel()) for x in (a0, a1, b0, b1)]
    for square in (False, True):
        want = _tensor_int(a0, a1, None if square else b0, None if square else b1, mod[:level], [1])[1]
        outs = [_polys(mfhe, npoly, level, n) for _ in range(3)]
        ctx.ctmul_tensor(dev[0], dev[1], None if square else dev[2], None if square else dev[3], outs[0].t, outs[1].t,
                         outs[2].t, npoly, level, 1)
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            bad = np.flatnonzero((o.blocks((npoly, level, n)) != want[k]).reshape(npoly, -1).any(axis=1))
            assert bad.size == 0, f"d{k} square {square}: {bad.size} wrong polynomials, the first {bad[:8].tolist()}"
            o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 4. the driver against the composition of the public calls
# ---------------------------------------------------------------------------------------------------------------
def _check_against_the_composition(mfhe, ctx, mod, rng, rlk, npoly, T, level, key_level, alpha, sp, k):
    """ctmul on fresh random operands of T terms against ctmul_tensor, keyswitch(KS_ADD) of d2 and, with CTMUL_RESCALE,
    ntt_moddown by limb level - 1 in place on each output: general and square, 1 and 3 terms, both flags, the outputs
    as two padded allocations and as the halves of one; the operands are untouched.  (tests/test_client_shapes_gpu.py
    runs it where the NTT plan changes.)"""
    import torch
    n = ctx.N
    lw = level * n
    a0, a1, b0, b1 = (_random_rows(rng, (T, npoly), mod[:level], n) for _ in range(4))
    A0, A1 = (_operand(mfhe, x, npoly, 2, 4, 0) for x in (a0, a1))
    B0, B1 = (_operand(mfhe, x, npoly, 0, 6, 0) for x in (b0, b1))
    for square in (False, True):
        tb0, tb1 = (None, None) if square else (B0.t, B1.t)
        strides = dict(a_term_stride=A0.tst, a_poly_stride=A0.pst, b_term_stride=B0.tst, b_poly_stride=B0.pst)
        for nt in (1, 3):
            d0, d1, d2 = (torch.zeros(npoly * lw, dtype=torch.int64, device="cuda") for _ in range(3))
            ctx.ctmul_tensor(A0.t, A1.t, tb0, tb1, d0, d1, d2, npoly, level, nt, **strides)
            ctx.keyswitch(d2, rlk, d0, d1, npoly, level, key_level, alpha, sp, k, mfhe.KS_ADD)
            torch.cuda.synchronize()
            want = {0: [mfhe.to_host_u64(d).reshape(npoly, level, n).copy() for d in (d0, d1)]}
            for d in (d0, d1):
                ctx.ntt_moddown(d, d, npoly, level - 1, level - 1, 1, in_stride=lw, out_stride=lw)
            torch.cuda.synchronize()
            want[mfhe.CTMUL_RESCALE] = [mfhe.to_host_u64(d).reshape(npoly, level, n)[:, :level - 1].copy()
                                        for d in (d0, d1)]
            for flags in (0, mfhe.CTMUL_RESCALE):
                keep = level - 1 if flags else level
                msg = f"alpha {alpha} K {k} level {level} nterms {nt} square {square} flags {flags}"
                o0, o1 = _polys(mfhe, npoly, level, n, 3), _polys(mfhe, npoly, level, n, 3)
                ctx.ctmul(A0.t, A1.t, tb0, tb1, rlk, o0.t, o1.t, npoly, level, key_level, alpha, sp, k, nt,
                          flags, out_stride=o0.stride, **strides)
                both = torch.full((2 * npoly * lw + 2,), CANARY - (1 << 64), dtype=torch.int64, device="cuda")
                ctx.ctmul(A0.t, A1.t, tb0, tb1, rlk, both[:npoly * lw], both[npoly * lw:], npoly, level,
                          key_level, alpha, sp, k, nt, flags, **strides)
                torch.cuda.synchronize()
                hb = mfhe.to_host_u64(both)
                assert (hb[-2:] == np.uint64(CANARY)).all(), msg
                for c, o in enumerate((o0, o1)):
                    np.testing.assert_array_equal(o.blocks((npoly, level, n))[:, :keep], want[flags][c],
                                                  err_msg=f"out{c} (two allocations) " + msg)
                    o.check_pads()
                    np.testing.assert_array_equal(
                        hb[c * npoly * lw:(c + 1) * npoly * lw].reshape(npoly, level, n)[:, :keep],
                        want[flags][c], err_msg=f"out{c} (one allocation) " + msg)
    for blk in (A0, A1, B0, B1):
        np.testing.assert_array_equal(blk.blocks(blk.src.shape), blk.src)
        blk.check_pads()


@CLASSES
@LOGNS
def test_ctmul_equals_the_composition(mfhe, log_n, bits):
    """ctmul = ctmul_tensor, keyswitch(KS_ADD) of d2 and, with CTMUL_RESCALE, ntt_moddown by limb level - 1 in place on
    each output (rows [0, level - 1) compared).  The outputs are once two padded allocations (the rescale runs per
    output) and once the halves of one dense allocation (it runs as one batch)."""
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(50 + log_n)
    npoly, T = 2, 3
    for key_level, alpha, sp, k, levels in KS_CASES:
        kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
        rlk = mfhe.to_device_u64(_random_rows(rng, (-(-key_level // alpha), 2), kmod, n).ravel())
        for level in levels:
            _check_against_the_composition(mfhe, ctx, mod, rng, rlk, npoly, T, level, key_level, alpha, sp, k)


# ---------------------------------------------------------------------------------------------------------------
# 5. the driver against the coefficient-domain model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("square", [False, True], ids=["general", "square"])
def test_ctmul_equals_the_model(mfhe, bits, square):
    """N = 16, the seeded ciphertexts of tests/test_ctmul_cpu.py (b = m - a s, sent through ntt_fwd): the product on
    the device, back through ntt_inv, equals the model residue for residue at levels 5, 3 and 2 with 1 and 3 terms,
    with and without rescale, and decrypts within the model's bound."""
    import torch
    cs = km.seeded_case(bits, "relin", True)
    q, p, n, alpha, s, s2 = cs["q"], cs["p"], cs["n"], cs["alpha"], cs["s_to"], cs["s_from"]
    ctx = mfhe.Context(q + p, 4, mfhe.CONV_PHANTOM)
    rlk = _device_key(mfhe, ctx, cs)
    for level in cm.LEVELS:
        Ql = km.prod(q[:level])
        for nt in (1, 3):
            _, cts_a, cts_b, _, _ = cm.seeded_inputs(bits, level, nt, square)

            def device(cts, comp):
                res = _residues([ct[comp] for ct in cts], q[:level])
                return ctx.ntt_fwd(mfhe.to_device_u64(res.ravel()), len(cts), 0, level)

            a0, a1 = device(cts_a, 0), device(cts_a, 1)
            b0, b1 = (None, None) if square else (device(cts_b, 0), device(cts_b, 1))
            for flags in (0, mfhe.CTMUL_RESCALE):
                res = cm.product(q, p, alpha, level, cts_a, cts_b, cs["key"], bool(flags))
                assert res["margin"] >= 2.0 ** -30, "pick another seed: a remainder sits at a tie"
                keep = level - 1 if flags else level
                o0 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
                o1 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
                ctx.ctmul(a0, a1, b0, b1, rlk, o0, o1, 1, level, 5, alpha, 5, 2, nt, flags)
                ctx.ntt_inv(o0, 1, 0, keep)
                ctx.ntt_inv(o1, 1, 0, keep)
                torch.cuda.synchronize()
                msg = f"level {level} nterms {nt} flags {flags}"
                for c, o in enumerate((o0, o1)):
                    np.testing.assert_array_equal(mfhe.to_host_u64(o).reshape(level, n)[:keep],
                                                  _residues([res["out"][c]], q[:keep])[0], err_msg=f"out{c} " + msg)
                err = cm.decryption_error(q, level, res, s, s2, bool(flags))
                bnd = cm.bound(q, p, alpha, level, n, bool(flags))
                print(f"ctmul bits {bits} {msg}: error / bound = {err / bnd:.4f}")
                assert err <= bnd and bnd < Ql // 4


# ---------------------------------------------------------------------------------------------------------------
# 6. graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After ctmul_reserve, ctmul allocates nothing and copies nothing to the device: it is captured into a graph on
    one stream (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed twice on changed inputs;
    each replay equals the eager call on those inputs."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, n = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    npoly, level, key_level, alpha, sp, k, nt = 2, 5, 5, 2, 5, 2, 3
    flags = mfhe.CTMUL_RESCALE
    ctx.ctmul_reserve(npoly, level, key_level, alpha, sp, k, flags)
    rng = np.random.default_rng(8)
    rlk = mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, n).ravel())
    ops = [mfhe.to_device_u64(_random_rows(rng, (nt, npoly), mod[:level], n).ravel()) for _ in range(4)]
    o0 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")

    def apply(x0, x1):
        ctx.ctmul(ops[0], ops[1], ops[2], ops[3], rlk, x0, x1, npoly, level, key_level, alpha, sp, k, nt, flags)

    def kept(t):
        return mfhe.to_host_u64(t).reshape(npoly, level, n)[:, :level - 1].copy()

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
        for t in ops:
            t.copy_(mfhe.to_device_u64(_random_rows(rng, (nt, npoly), mod[:level], n).ravel()))


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
    L5 = 5 * N

    def tensor(a0=pa0, a1=pa1, ats=2 * L5, aps=L5, b0=pb0, b1=pb1, bts=2 * L5, bps=L5, nt=2, d0=p0, d1=p1, ost=L5,
               d2=p2, o2st=L5, npoly=2, level=5):
        return lib.mfhe_ctmul_tensor(h, a0, a1, ats, aps, b0, b1, bts, bps, nt, d0, d1, ost, d2, o2st, npoly, level,
                                     None)

    def apply(a0=pa0, a1=pa1, ats=2 * L5, aps=L5, b0=pb0, b1=pb1, bts=2 * L5, bps=L5, nt=2, key=pk, o0=p0, o1=p1,
              ost=L5, npoly=2, level=5, kl=5, alpha=2, sp=5, k=2, flags=0):
        return lib.mfhe_ctmul_apply(h, a0, a1, ats, aps, b0, b1, bts, bps, nt, key, o0, o1, ost, npoly, level, kl,
                                    alpha, sp, k, flags, None)

    def reserve(npoly=2, level=5, kl=5, alpha=2, sp=5, k=2, flags=0):
        return lib.mfhe_ctmul_reserve(h, npoly, level, kl, alpha, sp, k, flags)

    cases = {
        "tensor null a0": lambda: tensor(a0=None),
        "tensor null a1": lambda: tensor(a1=None),
        "tensor null d0": lambda: tensor(d0=None),
        "tensor null d1": lambda: tensor(d1=None),
        "tensor null d2": lambda: tensor(d2=None),
        "tensor only b0": lambda: tensor(b1=None),
        "tensor only b1": lambda: tensor(b0=None),
        "tensor nterms 0": lambda: tensor(nt=0),
        "tensor nterms 65": lambda: tensor(nt=65, npoly=0),
        "tensor level 0": lambda: tensor(level=0),
        "tensor level outside": lambda: tensor(level=8),
        "tensor a poly stride": lambda: tensor(aps=L5 - 1),
        "tensor a term stride": lambda: tensor(ats=2 * L5 - 1),
        "tensor b poly stride": lambda: tensor(bps=L5 - 1),
        "tensor b term stride": lambda: tensor(bts=2 * L5 - 1),
        "tensor d01 stride": lambda: tensor(ost=L5 - 1),
        "tensor d2 stride": lambda: tensor(o2st=L5 - 1),
        "tensor d0 is a0": lambda: tensor(d0=pa0),
        "tensor d1 overlaps a1": lambda: tensor(d1=pa1 + 8 * (4 * L5 - 1)),
        "tensor d2 is b0": lambda: tensor(d2=pb0),
        "tensor d2 overlaps b1": lambda: tensor(d2=pb1 + 8 * N),
        "tensor d0 is d1": lambda: tensor(d1=p0),
        "tensor d2 overlaps d0": lambda: tensor(d2=p0 + 8 * (2 * L5 - 1)),
        "tensor square d1 is a1": lambda: tensor(b0=None, b1=None, d1=pa1),
        "apply null a0": lambda: apply(a0=None),
        "apply null a1": lambda: apply(a1=None),
        "apply null out0": lambda: apply(o0=None),
        "apply null out1": lambda: apply(o1=None),
        "apply null key": lambda: apply(key=None),
        "apply only b0": lambda: apply(b1=None),
        "apply nterms 0": lambda: apply(nt=0),
        "apply nterms 65": lambda: apply(nt=65, npoly=0),
        "apply a poly stride": lambda: apply(aps=L5 - 1),
        "apply b term stride": lambda: apply(bts=2 * L5 - 1),
        "apply out stride": lambda: apply(ost=L5 - 1),
        "apply out0 is a0": lambda: apply(o0=pa0),
        "apply out1 overlaps b1": lambda: apply(o1=pb1 + 8 * N),
        "apply out0 is out1": lambda: apply(o1=p0),
        "apply out1 is the key": lambda: apply(o1=pk),
        "apply unknown flag": lambda: apply(flags=2),
        "apply rescale at level 1": lambda: apply(level=1, aps=N, ats=2 * N, bps=N, bts=2 * N, ost=N, flags=1),
        "apply alpha < 1": lambda: apply(alpha=0),
        "apply nspecial < 1": lambda: apply(k=0),
        "apply level > key_level": lambda: apply(kl=4),
        "apply level < 1": lambda: apply(level=0),
        "apply special overlaps Q": lambda: apply(sp=4),
        "apply special outside": lambda: apply(sp=6),
        "reserve unknown flag": lambda: reserve(flags=2),
        "reserve rescale at level 1": lambda: reserve(level=1, flags=1),
        "reserve alpha < 1": lambda: reserve(alpha=0),
        "reserve nspecial < 1": lambda: reserve(k=0),
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
    assert lib.mfhe_ctmul_tensor(hp, pa0, pa1, 2 * L5, L5, pb0, pb1, 2 * L5, L5, 2, p0, p1, L5, p2, L5, 2, 5, None) == R
    assert lib.mfhe_ctmul_apply(hp, pa0, pa1, 2 * L5, L5, pb0, pb1, 2 * L5, L5, 2, pk, p0, p1, L5, 2, 5, 5, 2, 5, 2, 0,
                                None) == R
    assert lib.mfhe_ctmul_reserve(hp, 2, 5, 5, 2, 5, 2, 0) == R
    torch.cuda.synchronize()
    for name, b in bufs.items():   # nothing ran: every word is still the canary
        assert b.all_canary(), name
