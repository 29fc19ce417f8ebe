"""GPU checks of encrypted polynomial evaluation (csrc/lincomb.hip, csrc/poly.hip; include/mfhe.h mfhe_ct_lincomb,
mfhe_poly_plan_*, mfhe_poly_reserve, mfhe_poly_apply): the scalar sum bit for bit against Python integers (worst-case
words under 61-bit moduli among them) and against mfhe_lt_pt_mac on constant plaintexts, argument errors, graph
capture, the driver against its definition through the public calls, and three polynomials seen through the slots
under the bound of tests/poly_model.py."""
import ctypes
import functools

import numpy as np
import pytest

import ks_model as km
import poly_model as pm
import slot_model as sm
import test_slot_gpu as tsg
from primes import primes_of_size
from test_keyswitch_gpu import CANARY, CLASSES, LAYOUTS, LOGNS, _Blocks, _polys, _random_rows, _u64

pytestmark = pytest.mark.gpu

NQ, NSP = 8, 2                       # Q primes and special primes of the contexts here
UNROLL = 8                           # csrc/lincomb.hip kLincombUnroll: the last template-unrolled term count
NTERMS = (1, UNROLL, UNROLL + 1, 16, 17, 32, 33, 64)


@functools.lru_cache(maxsize=None)
def _moduli(log_n, bits):
    """8 Q primes and 2 special primes with q = 1 mod 2N."""
    m = primes_of_size(bits[0], 2 << log_n, NQ) + primes_of_size(bits[1], 2 << log_n, NSP)
    assert len(set(m)) == NQ + NSP
    return tuple(m)


@functools.lru_cache(maxsize=None)
def _ctx(log_n, bits):
    import mfhe
    return mfhe.Context(list(_moduli(log_n, bits)), log_n, mfhe.CONV_PHANTOM)


def _sources(mfhe, rng, nsrc, npoly, rows, n, mod, ppad, opad, base):
    """Both components of nsrc ciphertexts of npoly polynomials at `rows` rows: (blocks0, blocks1, data0, data1,
    source stride, poly stride)."""
    pst = rows * n + ppad
    sst = npoly * pst + opad
    offs = [s * sst + p * pst for s in range(nsrc) for p in range(npoly)]
    d0 = _random_rows(rng, (nsrc, npoly), mod[:rows], n)
    d1 = _random_rows(rng, (nsrc, npoly), mod[:rows], n)
    return _Blocks(mfhe, offs, rows * n, base, d0), _Blocks(mfhe, offs, rows * n, base, d1), d0, d1, sst, pst


def _lincomb_int(d0, d1, K, term_x, term_k, addend_k, mod, level):
    """(out0, out1) [npoly][level][n] uint64 in Python integers; d [nsrc][npoly][rows][n], K [nk][>= level] ints."""
    outs = []
    for c, d in enumerate((d0, d1)):
        out = np.zeros((d.shape[1], level, d.shape[3]), dtype=np.uint64)
        for r in range(level):
            q = int(mod[r])
            acc = np.zeros((d.shape[1], d.shape[3]), dtype=object)
            for tx, tk in zip(term_x, term_k):
                acc = acc + d[tx, :, r, :].astype(object) * int(K[tk][r])
            if c == 0 and addend_k >= 0:
                acc = acc + int(K[addend_k][r])
            out[:, r, :] = (acc % q).astype(np.uint64)
        outs.append(out)
    return outs


def _constants(rng, nk, mod, rows):
    """[nk][rows] canonical residues: row 0 is zero, row 1 is q - 1, the rest random."""
    K = (rng.integers(0, 2 ** 63, (nk, rows), dtype=np.uint64) % _u64(mod[:rows])[None, :])
    K[0, :] = 0
    K[1, :] = _u64(mod[:rows]) - np.uint64(1)
    return K


# ---------------------------------------------------------------------------------------------------------------
# 1. the scalar sum is exact
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@CLASSES
@LOGNS
def test_ct_lincomb_is_exact(mfhe, log_n, bits, layout):
    """Bit for bit against Python integers.  The eight term counts (1, the last unrolled one, the first looped one,
    16 / 17 and 32 / 33 around the folds, 64) cross levels 1 and 5 (sources allocated at 8 rows), with and without
    the addend and npoly 1 and 3 as a full factorial; term indices repeat; component 1 never receives the addend."""
    import torch
    name, ppad, opad, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(100 * log_n + bits[0])
    nsrc, nk, rows = 5, 7, 8
    K = _constants(rng, nk, mod, rows)
    kpad = 1 if ppad % 2 else 0
    kb = _Blocks(mfhe, [i * (rows + kpad) for i in range(nk)], rows, 0, K)
    src = {npoly: _sources(mfhe, rng, nsrc, npoly, rows, n, mod, ppad, opad, base) for npoly in (1, 3)}
    for idx, nt in enumerate(NTERMS):
        level, addend, npoly = (1, 5)[idx & 1], (idx >> 1) & 1, (1, 3)[(idx >> 2) & 1]
        b0, b1, d0, d1, sst, pst = src[npoly]
        term_x = [int(v) for v in rng.integers(0, nsrc, nt)]
        term_k = [int(v) for v in rng.integers(0, nk, nt)]
        if nt >= 2:
            term_x[1], term_k[1] = term_x[0], term_k[0]          # a repeated pair
        addend_k = int(rng.integers(1, nk)) if addend else -1
        o0 = _polys(mfhe, npoly, level, n, ppad, base)
        o1 = _polys(mfhe, npoly, level, n, ppad, base)
        ctx.ct_lincomb(b0.t, b1.t, kb.t, o0.t, o1.t, term_x, term_k, npoly, level, nsrc, nk, addend_k,
                       src_stride=sst, x_poly_stride=pst, k_stride=rows + kpad, out_stride=o0.stride)
        torch.cuda.synchronize()
        want = _lincomb_int(d0, d1, K, term_x, term_k, addend_k, mod, level)
        msg = f"{name} nterms {nt} level {level} addend {addend_k} npoly {npoly}"
        np.testing.assert_array_equal(o0.blocks((npoly, level, n)), want[0], err_msg="out0 " + msg)
        np.testing.assert_array_equal(o1.blocks((npoly, level, n)), want[1], err_msg="out1 " + msg)
        o0.check_pads()
        o1.check_pads()
    for b, d in ((src[1][0], src[1][2]), (src[3][1], src[3][3])):
        np.testing.assert_array_equal(b.blocks(d.shape), d, err_msg="a source was written")


@CLASSES
def test_ct_lincomb_walks_runs_of_pairs(mfhe, bits):
    """log_n 4, level 5, 2050 polynomials: one block column of 5 rows leaves 4096 // 5 = 819 runs for 4100 (polynomial,
    component) pairs, so a thread walks 6 pairs (the rule of tests/test_ks_shapes_gpu.py with the pairs as the batch)
    and the last of the 684 runs holds 2."""
    import torch
    from test_ks_shapes_gpu import _prun
    log_n, level, npoly, nsrc, nk = 4, 5, 2050, 2, 3
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    prun = _prun(2 * npoly, 1, level)
    assert prun == 6 and -(-2 * npoly // prun) == 684 and 2 * npoly - 683 * prun == 2
    rng = np.random.default_rng(9)
    K = _constants(rng, nk, mod, level)
    for name, ppad, opad, base in (LAYOUTS[0], LAYOUTS[2]):
        b0, b1, d0, d1, sst, pst = _sources(mfhe, rng, nsrc, npoly, level, n, mod, ppad, opad, base)
        o0, o1 = _polys(mfhe, npoly, level, n, ppad, base), _polys(mfhe, npoly, level, n, ppad, base)
        term_x, term_k = [1, 0, 1], [2, 1, 1]
        ctx.ct_lincomb(b0.t, b1.t, mfhe.to_device_u64(K.ravel()), o0.t, o1.t, term_x, term_k, npoly, level, nsrc, nk, 2,
                       src_stride=sst, x_poly_stride=pst, out_stride=o0.stride)
        torch.cuda.synchronize()
        want = _lincomb_int(d0, d1, K, term_x, term_k, 2, mod, level)
        for o, w in ((o0, want[0]), (o1, want[1])):
            bad = np.flatnonzero((o.blocks((npoly, level, n)) != w).reshape(npoly, -1).any(axis=1))
            assert bad.size == 0, (name, bad[:8])
            o.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 2. the fold bound is real
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [16, 17, 64])
def test_ct_lincomb_at_the_largest_words(mfhe, nt):
    """61-bit moduli, every source word and every constant q - 1, the addend q - 1 as well: 16 products of (q - 1)^2
    and a carried residue are the largest sum between two folds, and the result is exact."""
    import torch
    log_n, level, npoly = 4, 3, 2
    mod = primes_of_size(61, 2 << log_n, level)
    assert len(mod) == level and all(q.bit_length() == 61 for q in mod)
    ctx, n = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM), 1 << log_n
    top = _u64(mod) - np.uint64(1)
    d = np.broadcast_to(top[None, None, :, None], (1, npoly, level, n)).copy()
    K = top[None, :].copy()
    x0, x1 = mfhe.to_device_u64(d.ravel()), mfhe.to_device_u64(d.ravel())
    for base in (0, 1):                                             # the 16-byte and the 8-byte form
        o0, o1 = _polys(mfhe, npoly, level, n, 0, base), _polys(mfhe, npoly, level, n, 0, base)
        ctx.ct_lincomb(x0, x1, mfhe.to_device_u64(K.ravel()), o0.t, o1.t, [0] * nt, [0] * nt, npoly, level, 1, 1, 0)
        torch.cuda.synchronize()
        for r, q in enumerate(mod):
            assert (o0.blocks((npoly, level, n))[:, r] == np.uint64((nt * (q - 1) ** 2 + q - 1) % q)).all(), (nt, r)
            assert (o1.blocks((npoly, level, n))[:, r] == np.uint64((nt * (q - 1) ** 2) % q)).all(), (nt, r)


# ---------------------------------------------------------------------------------------------------------------
# 3. the same sum through mfhe_lt_pt_mac
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
def test_ct_lincomb_equals_pt_mac_on_constant_plaintexts(mfhe, bits):
    """log_n 10: u [nslots][npoly][2][level + K][N] is read by both; a plaintext filled with K[i][r] on row r is the
    constant i.  The Q rows of the accumulator equal the sum's outputs, word for word."""
    import torch
    log_n, level, sp, k, npoly, nslots, nk = 10, 5, NQ, NSP, 2, 4, 3
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rows = level + k
    rmod = list(mod[:level]) + list(mod[sp:sp + k])
    rng = np.random.default_rng(31)
    u = _random_rows(rng, (nslots, npoly, 2), rmod, n)                     # [nslots][npoly][2][rows][n]
    K = _constants(rng, nk, rmod, rows)
    pt = np.broadcast_to(K[:, :, None], (nk, rows, n)).copy()
    d_u = mfhe.to_device_u64(u.ravel())
    for nt in (2, UNROLL, 11):
        term_u = [int(v) for v in rng.integers(0, nslots, nt)]
        term_k = [int(v) for v in rng.integers(0, nk, nt)]
        acc = torch.zeros(npoly * 2 * rows * n, dtype=torch.int64, device="cuda")
        ctx.lt_pt_mac(d_u, mfhe.to_device_u64(pt.ravel()), acc, term_u, term_k, npoly, level, sp, k, nslots, nk)
        o0 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
        o1 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
        ctx.ct_lincomb(d_u, d_u[rows * n:], mfhe.to_device_u64(K.ravel()), o0, o1, term_u, term_k, npoly, level, nslots,
                       nk, src_stride=npoly * 2 * rows * n, x_poly_stride=2 * rows * n, k_stride=rows)
        torch.cuda.synchronize()
        a = mfhe.to_host_u64(acc).reshape(npoly, 2, rows, n)
        np.testing.assert_array_equal(mfhe.to_host_u64(o0).reshape(npoly, level, n), a[:, 0, :level], err_msg=str(nt))
        np.testing.assert_array_equal(mfhe.to_host_u64(o1).reshape(npoly, level, n), a[:, 1, :level], err_msg=str(nt))
        assert a.any()


# ---------------------------------------------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    log_n, bits = 4, (45, 49)
    mod, N = _moduli(log_n, bits), 16
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)
    h, E, L = ctx.handle, mfhe.EINVAL, len(mod)
    level, npoly, nsrc, nk = 3, 2, 2, 3
    lw = level * N
    rng = np.random.default_rng(4)
    x = _polys(mfhe, 2 * nsrc * npoly, level, N, 0, 0, _random_rows(rng, (2 * nsrc * npoly,), mod[:level], N))
    kt = _polys(mfhe, 1, nk * level, 1, 0, 0, _constants(rng, nk, mod, level))
    out = _polys(mfhe, 2 * npoly, level, N)
    px, pk, po = x.t.data_ptr(), kt.t.data_ptr(), out.t.data_ptr()
    px1, po1 = px + 8 * nsrc * npoly * lw, po + 8 * npoly * lw
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    tx, tk = ints(0, 1), ints(2, 0)

    def lc(x0=px, x1=px1, sst=npoly * lw, pst=lw, nsrc=nsrc, k=pk, kst=level, nk=nk, tx=tx, tk=tk, nt=2, add=-1, o0=po,
           o1=po1, ost=lw, npoly=npoly, level=level, ctx_h=h):
        return lib.mfhe_ct_lincomb(ctx_h, x0, x1, sst, pst, nsrc, k, kst, nk, tx, tk, nt, add, o0, o1, ost, npoly, level,
                                   None)

    bad = [
        lc(x0=None), lc(x1=None), lc(k=None), lc(o0=None), lc(o1=None), lc(tx=None), lc(tk=None), lc(ctx_h=None),
        lc(nt=0), lc(nt=65), lc(nt=-1),                                                   # nterms outside [1, 64]
        lc(tx=ints(0, nsrc)), lc(tx=ints(-1, 0)), lc(tk=ints(nk, 0)), lc(tk=ints(0, -1)), # term indices
        lc(nsrc=1), lc(nk=2),
        lc(add=-2), lc(add=nk),                                                           # the addend
        lc(level=0), lc(level=L + 1),                                                     # level outside the context
        lc(pst=lw - 1), lc(ost=lw - 1), lc(sst=npoly * lw - 1), lc(kst=level - 1),        # strides
        lc(o0=px + 8), lc(o1=px1 + 8 * (lw - 1)), lc(o0=pk), lc(o1=pk + 8 * (nk * level - 1)),   # an output on an input
        lc(o1=po + 8 * (npoly * lw - 1)), lc(o1=po),                                      # the outputs on each other
    ]
    assert bad == [E] * len(bad), bad
    torch.cuda.synchronize()
    assert out.all_canary(), "a rejected call wrote something"
    assert lc(npoly=0) == mfhe.OK
    torch.cuda.synchronize()
    assert out.all_canary(), "npoly == 0 launched something"
    noph = mfhe.Context(list(tsg._moduli(5, (45, 49))), 4, mfhe.CONV_GL)   # q = 1 mod 4N, no phantom tables
    assert lc(ctx_h=noph.handle) == mfhe.ENOTREADY

    # ---- plans ----
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    ph = ctypes.c_void_p()
    a7 = dbl(*([0.5] * 8))
    inf, nan = float("inf"), float("nan")

    def mk(coeffs=a7, degree=7, basis=mfhe.POLY_MONOMIAL, scale=2.0 ** 45, level=NQ, out=ctypes.byref(ph), ctx_h=h):
        return lib.mfhe_poly_plan_create(ctx_h, coeffs, degree, basis, scale, level, out)

    bad = [
        mk(coeffs=None), mk(out=None), mk(ctx_h=None),
        mk(degree=0), mk(degree=128), mk(degree=-1), mk(basis=2), mk(basis=-1),
        mk(coeffs=dbl(0.5, nan, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)), mk(coeffs=dbl(inf, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)),
        mk(scale=nan), mk(scale=inf), mk(scale=0.0), mk(scale=-2.0 ** 45),
        mk(level=0), mk(level=L + 1),
        mk(level=4), mk(level=4, basis=mfhe.POLY_CHEBYSHEV),             # degree 7 takes 4 levels: level - 1 = 3
        mk(coeffs=dbl(0.5, 0.5, 1e30, 0.5, 0.5, 0.5, 0.5, 0.5)),         # a constant beyond 2^126
        mk(coeffs=dbl(0.5, 0, 0, 0, 0, 0, 0, 0)),                        # nothing to evaluate
    ]
    assert bad == [E] * len(bad), bad
    assert ph.value is None
    assert mk(ctx_h=noph.handle) == mfhe.ENOTREADY
    assert mk(level=5) == mfhe.OK and ph.value
    assert lib.mfhe_poly_plan_destroy(ph) == mfhe.OK
    assert lib.mfhe_poly_plan_destroy(None) == mfhe.OK
    with pytest.raises(mfhe.MfheError):
        ctx.poly_plan([0.5] * 8, mfhe.POLY_MONOMIAL, 2.0 ** 45, 4)

    # ---- the driver ----
    plan = ctx.poly_plan([0.5] * 8, mfhe.POLY_MONOMIAL, 2.0 ** 45, NQ)
    info = plan.info()
    plv, olv = info.level, info.out_level
    assert (plv, olv) == (NQ, NQ - 4)
    other = mfhe.Context(list(_moduli(log_n, (50, 61))), log_n, mfhe.CONV_PHANTOM)
    alpha, sp, k = 3, NQ, NSP
    beta = -(-plv // alpha)
    pw, ow = plv * N, olv * N
    cin = _polys(mfhe, 2 * npoly, plv, N, 0, 0, _random_rows(rng, (2 * npoly,), mod[:plv], N))
    rlk = _polys(mfhe, 1, beta * 2 * (plv + k), N, 0, 0, _random_rows(rng, (beta * 2,), mod, N))
    res = _polys(mfhe, 2 * npoly, olv, N)
    pc, pr, pres = cin.t.data_ptr(), rlk.t.data_ptr(), res.t.data_ptr()
    pc1, pres1 = pc + 8 * npoly * pw, pres + 8 * npoly * ow

    def ap(plan_h=plan.handle, c0=pc, c1=pc1, ist=pw, key=pr, o0=pres, o1=pres1, ost=ow, npoly=npoly, key_level=plv,
           alpha=alpha, sp=sp, k=k, ctx_h=h):
        return lib.mfhe_poly_apply(ctx_h, plan_h, c0, c1, ist, key, o0, o1, ost, npoly, key_level, alpha, sp, k, None)

    def rs(plan_h=plan.handle, npoly=npoly, key_level=plv, alpha=alpha, sp=sp, k=k, ctx_h=h):
        return lib.mfhe_poly_reserve(ctx_h, plan_h, npoly, key_level, alpha, sp, k)

    bad = [
        ap(plan_h=None), ap(c0=None), ap(c1=None), ap(key=None), ap(o0=None), ap(o1=None), ap(ctx_h=None),
        ap(ctx_h=other.handle), rs(ctx_h=other.handle),                                   # a plan of other moduli
        ap(ist=pw - 1), ap(ost=ow - 1),                                                   # strides
        ap(o0=pc), ap(o1=pc1 + 8 * (npoly * pw - 1)), ap(o0=pr + 8), ap(o1=pres + 8 * (npoly * ow - 1)),   # overlaps
        ap(key_level=plv - 1), rs(key_level=plv - 1),                                     # a key made below the plan's level
        ap(alpha=0), ap(k=0), ap(sp=plv - 1), ap(sp=L), ap(key_level=L + 1),              # what the products reject
        rs(plan_h=None), rs(alpha=0), rs(k=0), rs(sp=L), rs(ctx_h=None),
    ]
    assert bad == [E] * len(bad), bad
    torch.cuda.synchronize()
    assert res.all_canary(), "a rejected call wrote something"
    assert ap(npoly=0) == mfhe.OK
    torch.cuda.synchronize()
    assert res.all_canary(), "npoly == 0 launched something"
    assert ap(ctx_h=noph.handle) == mfhe.ENOTREADY and rs(ctx_h=noph.handle) == mfhe.ENOTREADY
    plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 6 (used by 5 as well). the driver is its definition
# ---------------------------------------------------------------------------------------------------------------
def _seeded_coeffs(rng, degree):
    a = rng.uniform(-1, 1, degree + 1)
    if degree >= 3:
        a[rng.integers(0, degree)] = 0.0
    return [float(v) for v in a]


def _run_by_public_calls(mfhe, ctx, plan, c0, c1, rlk, npoly, key_level, alpha, sp, k):
    """The plan's nodes in order through ctmul (no rescale), ct_lincomb and ntt_moddown on both components; the
    registers are slots of two tensors of their own, t and y separate buffers.  Returns (out0, out1) host arrays
    [npoly][out_level][N]."""
    import torch
    info, N = plan.info(), ctx.N
    lv = info.level
    lw = lv * N
    slot = npoly * lw
    X0 = torch.zeros((info.nreg + 1) * slot, dtype=torch.int64, device="cuda")     # the registers, then t
    X1 = torch.zeros((info.nreg + 1) * slot, dtype=torch.int64, device="cuda")
    y0 = torch.zeros(slot, dtype=torch.int64, device="cuda")
    y1 = torch.zeros(slot, dtype=torch.int64, device="cuda")
    X0[:slot].copy_(c0)
    X1[:slot].copy_(c1)
    reg = lambda X, r: X[r * slot:(r + 1) * slot]
    tslot = info.nreg
    for nd in plan.nodes():
        l = nd["level"]
        term_x, term_k = [s for s, _, _ in nd["terms"]], [kk for _, kk, _ in nd["terms"]]
        if nd["mul_a"] >= 0:
            a, b = nd["mul_a"], nd["mul_b"]
            sq = a == b
            ctx.ctmul(reg(X0, a), reg(X1, a), None if sq else reg(X0, b), None if sq else reg(X1, b), rlk,
                      reg(X0, tslot), reg(X1, tslot), npoly, l, key_level, alpha, sp, k, 1, 0, a_poly_stride=lw,
                      b_poly_stride=lw, out_stride=lw)
            term_x, term_k = [tslot] + term_x, [nd["k_mul"]] + term_k
        ctx.ct_lincomb(X0, X1, plan, y0, y1, term_x, term_k, npoly, l, info.nreg + 1, None, nd["addend_k"],
                       src_stride=slot, x_poly_stride=lw, out_stride=lw)
        for y, X in ((y0, X0), (y1, X1)):
            ctx.ntt_moddown(y, reg(X, nd["dst"]), npoly, l - 1, l - 1, 1, in_stride=lw, out_stride=lw)
    torch.cuda.synchronize()
    ol = info.out_level
    return tuple(mfhe.to_host_u64(reg(X, info.out_reg)).reshape(npoly, lv, N)[:, :ol].copy() for X in (X0, X1))


@CLASSES
@LOGNS
def test_poly_apply_is_its_definition(mfhe, log_n, bits):
    """Both bases at degrees 1, 2, 3, 7 and 15 on two polynomials, the outputs at a padded stride: mfhe_poly_apply equals,
    bit for bit, its exported node list run through the public calls."""
    import torch
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    level, key_level, alpha, sp, k, npoly = NQ, NQ, 3, NQ, NSP, 2
    scale = 2.0 ** bits[0]
    rng = np.random.default_rng(7 * log_n + bits[0])
    beta = -(-key_level // alpha)
    rlk = mfhe.to_device_u64(_random_rows(rng, (beta, 2), mod, n).ravel())
    c0 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    c1 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    for basis in (mfhe.POLY_MONOMIAL, mfhe.POLY_CHEBYSHEV):
        for degree in (1, 2, 3, 7, 15):
            plan = ctx.poly_plan(_seeded_coeffs(rng, degree), basis, scale, level)
            info = plan.info()
            assert info.depth <= int(np.ceil(np.log2(degree + 1))) + 1 and info.nnodes >= 1
            want = _run_by_public_calls(mfhe, ctx, plan, c0, c1, rlk, npoly, key_level, alpha, sp, k)
            ol = info.out_level
            o0, o1 = _polys(mfhe, npoly, ol, n, 2), _polys(mfhe, npoly, ol, n, 2)
            ctx.poly_apply(plan, c0, c1, rlk, o0.t, o1.t, npoly, key_level, alpha, sp, k, out_stride=o0.stride)
            torch.cuda.synchronize()
            msg = f"basis {basis} degree {degree}"
            np.testing.assert_array_equal(o0.blocks((npoly, ol, n)), want[0], err_msg="out0 " + msg)
            np.testing.assert_array_equal(o1.blocks((npoly, ol, n)), want[1], err_msg="out1 " + msg)
            o0.check_pads()
            o1.check_pads()
            assert want[0].any() and want[1].any()
            plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After poly_reserve, poly_apply allocates nothing and copies nothing to the device: a degree-7 plan at log_n 10
    is captured on one stream (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed on the
    captured inputs and on fresh ones; each replay equals the eager call.  The same for ct_lincomb alone."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, n = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    level, key_level, alpha, sp, k, npoly = NQ, NQ, 3, NQ, NSP, 2
    rng = np.random.default_rng(12)
    plan = ctx.poly_plan(_seeded_coeffs(rng, 7), mfhe.POLY_CHEBYSHEV, 2.0 ** 45, level)
    ol = plan.info().out_level
    ctx.poly_reserve(plan, npoly, key_level, alpha, sp, k)
    fresh = lambda: mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    rlk = mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, n).ravel())
    c0, c1 = fresh(), fresh()
    K = mfhe.to_device_u64(_constants(rng, 3, mod, level).ravel())

    def zeros(rows):
        return torch.zeros(npoly * rows * n, dtype=torch.int64, device="cuda")

    def apply(o0, o1, s0, s1):
        ctx.poly_apply(plan, c0, c1, rlk, o0, o1, npoly, key_level, alpha, sp, k)
        ctx.ct_lincomb(c0, c1, K, s0, s1, [0, 0, 0], [1, 2, 0], npoly, level, 1, 3, 2)

    outs = [zeros(ol), zeros(ol), zeros(level), zeros(level)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        apply(*outs)
    first = None
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [mfhe.to_host_u64(t).copy() for t in outs]
        eager = [zeros(ol), zeros(ol), zeros(level), zeros(level)]
        apply(*eager)
        torch.cuda.synchronize()
        for g, e in zip(got, eager):
            np.testing.assert_array_equal(g, mfhe.to_host_u64(e))
            assert g.any()
        if first is not None:
            assert all((f != g).any() for f, g in zip(first, got))
        first = got
        c0.copy_(fresh())
        c1.copy_(fresh())
    plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. through the slots
# ---------------------------------------------------------------------------------------------------------------
class _Scheme(tsg._Scheme):
    """tests/test_slot_gpu.py's scheme (ternary secret, encryption and decryption pointwise on the host) at N = 2^10,
    level 8 + 2 special limbs (limbs 8, 9), alpha 2."""

    def __init__(self, mfhe, bits):
        self.km, self.mfhe = km, mfhe
        self.log_n, self.level, self.key_level, self.alpha, self.sp, self.k = 10, NQ, NQ, 2, NQ, NSP
        self.N = 1 << self.log_n
        self.mod = _moduli(self.log_n, bits)
        self.ctx = _ctx(self.log_n, bits)
        self.q, self.p = list(self.mod[:self.level]), list(self.mod[self.sp:self.sp + self.k])
        self.limbs = list(range(self.key_level)) + list(range(self.sp, self.sp + self.k))
        self.rng = np.random.default_rng(56)
        s = self.rng.integers(-1, 2, self.N)
        self.s_ev = self._eval_rows([int(v) for v in s])
        self.s_dev = mfhe.to_device_u64(self.s_ev.ravel())
        self.s2_dev = mfhe.to_device_u64(self._mul(self.s_ev, self.s_ev, self.limbs).ravel())

    def encode_real(self, x, scale):
        import torch
        out = torch.zeros(self.level * self.N, dtype=torch.int64, device="cuda")
        self.ctx.slot_encode(tsg._dev_f64(self.mfhe, x), out, 1, self.level, scale, flags=self.mfhe.SLOT_REAL)
        return self.mfhe.to_host_u64(out).reshape(self.level, self.N)


def _slot_cases(rng, n):
    cheb = np.polynomial.chebyshev
    nodes = np.cos(np.pi * (np.arange(64) + 0.5) / 64)
    f15 = lambda x: np.exp(x) * np.sin(3 * x)
    f31 = lambda x: np.tanh(4 * x) + 0.25 * np.cos(9 * x)
    return [
        ("A monomial degree 7", pm.MONOMIAL, [float(v) for v in rng.uniform(-1, 1, 8)],
         rng.random(n) + 1j * rng.random(n), False),
        ("B chebyshev degree 15", pm.CHEBYSHEV, [float(v) for v in cheb.chebfit(nodes, f15(nodes), 15)],
         rng.uniform(-1, 1, n), True),
        ("C chebyshev degree 31", pm.CHEBYSHEV, [float(v) for v in cheb.chebfit(nodes, f31(nodes), 31)],
         rng.uniform(-1, 1, n), True),
    ]


@CLASSES
def test_polynomials_seen_through_the_slots(mfhe, bits):
    """A monomial-basis degree-7 polynomial on complex slots of the unit square, and Chebyshev fits of degree 15 and 31
    (the last ends at level 2) on real slots of [-1, 1] encoded with SLOT_REAL, at scale 2^45 (45-bit class) or 2^50,
    each decoded and compared with p(z) from numpy.  The tolerance is poly_model.propagate's bound through the node
    list in the slot domain: the input's N (1/2 + B_E) / scale and the encoder's float term, N ks_model.error_bound per
    relinearisation, N (1 + N) / 2 per rescale, the constants' roundings, and the decoder's float term on the result.
    It is asserted on the CPU, before anything runs on the GPU, to be below 1/64 of the spread of the expected slots:
    a wrong coefficient, basis, scale or level shows as an error of the order of the spread.

    Measured on an MI355X (slot error / bound; DESIGN.md 3.15 has the table): 45-bit class A 2.6e-10 / 2.1e-7,
    B 1.2e-10 / 1.0e-7, C 1.4e-10 / 1.7e-7; 50-bit class A 6.8e-12 / 6.5e-9, B 4.0e-12 / 3.3e-9, C 4.1e-12 / 5.4e-9."""
    import torch
    log_n, level, key_level, alpha, sp, k = 10, NQ, NQ, 2, NQ, NSP
    N, n = 1 << log_n, 1 << (log_n - 1)
    mod = _moduli(log_n, bits)
    q, p = list(mod[:level]), list(mod[sp:sp + k])
    scale = 2.0 ** bits[0]
    rng = np.random.default_rng(77)
    B_E = km.B_E
    relin = {l: N * km.error_bound(q, p, alpha, l, N, B_E) for l in range(2, level + 1)}
    ctx = _ctx(log_n, bits)
    work = []
    for name, basis, coeffs, z, real in _slot_cases(rng, n):
        plan = ctx.poly_plan(coeffs, basis, scale, level)     # host arithmetic and one table upload; no kernel runs
        pd = pm.from_handle(plan, mod)
        want = pm.evaluate(coeffs, basis, z.astype(np.complex128))
        fp_in, _ = tsg._fp_terms(z, log_n, scale)
        e_in = N * (0.5 + B_E) / scale + fp_in
        intended, bound = pm.propagate(pd, z.astype(np.complex128), e_in, relin, N * (1 + N) / 2)
        bound += tsg._fp_terms(want, log_n, pd["out_scale"])[1] + pm.coefficient_arithmetic(coeffs, basis)
        bound += float(np.abs(intended - want).max())          # the intended value is p(z) up to float evaluation
        spread = max(np.ptp(want.real), np.ptp(want.imag))
        print(f"{name}: bound {bound:.3g}, spread {spread:.3g}, depth {pd['depth']}, products {pd['nmul']}, "
              f"out level {pd['out_level']}")
        assert bound < spread / 64, (name, bound, spread)
        two_limbs = int(q[0]) * int(q[1]) // 2
        assert (float(np.abs(want).max()) + bound) * pd["out_scale"] < two_limbs
        if "31" in name:
            assert pd["out_level"] == 2
        work.append((name, plan, pd, z, real, want, bound))
    # ---- everything above ran on the CPU; from here on the GPU ----
    sc = _Scheme(mfhe, bits)
    rlk = ctx.gen_switch_key(sc.s2_dev, sc.s_dev, key_level, alpha, sp, k)
    for name, plan, pd, z, real, want, bound in work:
        c0, c1 = sc.encrypt(sc.encode_real(z, scale) if real else sc.encode(z, scale))
        ol = pd["out_level"]
        o0 = torch.zeros(ol * N, dtype=torch.int64, device="cuda")
        o1 = torch.zeros(ol * N, dtype=torch.int64, device="cuda")
        ctx.poly_apply(plan, c0, c1, rlk, o0, o1, 1, key_level, alpha, sp, k)
        got = sc.decrypt_decode(o0, o1, ol, pd["out_scale"], stride_rows=ol)
        err = float(np.abs(got - want).max())
        tsg._report(name, err, bound)
        plan.close()
