"""GPU checks of key switching, rotations and the NTT-domain base conversion at the launch shapes the other files do
not reach (csrc/keyswitch.hip, csrc/galois.hip, csrc/bconv.hip through include/mfhe.h):

  1. the inner product with a thread's run of polynomials longer than kKsipMinRun, plain and gathered;
  2. the automorphism with (polynomial, row) folded over grid y and z;
  3. mfhe_ntt_modup, mfhe_ntt_moddown, mfhe_keyswitch, mfhe_keyswitch_raise, mfhe_galois_apply and
     mfhe_galois_apply_raised where the NTT they call on parts of the workspace runs the pipelined single pass (plan 4)
     or two passes (plan 2), and with the batch cut into chunks;
  4. one key switch at N = 2^14 checked by its decryption error, with the CPU oracle's transform and Python integers
     only.

Every comparison is exact equality against Python integers or against a composition of public calls that other tests
check against Python integers or the oracle; the one inequality is the proved noise bound of tests/ks_model.py."""
import random

import numpy as np
import pytest

import ks_model as km
from test_galois_gpu import LAYOUTS, _ctx3, _ctx7, _perm_np
from test_galois_gpu import _composition as _galois_composition
from test_keyswitch_gpu import (_Blocks, _composition, _inner_product_int, _moduli, _polys, _random_rows, _residues,
                                _row_limbs, _u64)

pytestmark = pytest.mark.gpu

U64_BITS, F64_BITS = (50, 61), (45, 49)


# ---------------------------------------------------------------------------------------------------------------
# 1. inner product: runs longer than kKsipMinRun
# ---------------------------------------------------------------------------------------------------------------
def _prun(npoly, bx, rows):
    """launch_ksk_inner_product's rule (ks_runs, csrc/ks_host.hpp): runs = max(1, 4096 / (bx rows)) workgroup columns,
    prun = ceil(npoly / runs), but never below kKsipMinRun = 4 (or the batch, when that is smaller)."""
    runs = max(1, 4096 // (bx * rows))
    prun = -(-npoly // runs)
    return prun if prun >= 4 else min(npoly, 4)


# 7 rows in one block column: runs = 585.  2340 = 4 * 585 is the last count with runs of 4, 2341 the first with runs
# of 5; 3001 gives runs of 6, 501 of them, the last holding one polynomial
KSIP_NPOLY = (2340, 2341, 3001)
KSIP_LAYOUTS = [l for l in LAYOUTS if l[0] in ("dense", "padded-odd", "misaligned")]


@pytest.mark.parametrize("npoly", KSIP_NPOLY)
@pytest.mark.parametrize("nd", [1, 3, 7])
@pytest.mark.parametrize("log_n,g", [(1, 1), (1, 3), (4, 1), (4, pow(5, 7, 32)), (4, 31)])
def test_inner_product_with_runs_longer_than_the_minimum(mfhe, log_n, g, nd, npoly):
    """Digit counts 1 and 3 (unrolled) and 7 (the generic loop); the gathered form for every g, and for g = 1 the
    plain form as well.  Every polynomial of the batch is compared, so a run that starts at the wrong polynomial, a
    short last run or a run beyond the batch shows as a wrong or an unwritten block."""
    import torch
    ctx, mod, n = _ctx7(log_n, U64_BITS), _moduli(log_n, U64_BITS), 1 << log_n
    level = key_level = sp = 5
    k, rows = 2, 7
    assert n // 2 <= 256, "one block per row (bx = 1) in the 16-byte and in the scalar form"
    prun = _prun(npoly, 1, rows)
    assert prun == {2340: 4, 2341: 5, 3001: 6}[npoly]
    if npoly == 3001:
        assert -(-npoly // prun) == 501 and npoly - 500 * prun == 1
    rng = np.random.default_rng(100 * log_n + 10 * g + nd)
    rmod = [mod[l] for l in _row_limbs(level, sp, k)]
    src = _random_rows(rng, (nd, npoly), rmod, n)                   # [nd][npoly][rows][n]
    top = _u64(rmod) - np.uint64(1)
    assert (src[0, 0, :, 0] == 0).all() and (src[0, 0, :, 1] == top).all() and (src[-1, -1, :, 0] == top).all()
    ksk = _random_rows(rng, (nd, 2), rmod, n)
    d_ksk = mfhe.to_device_u64(ksk.ravel())
    want = _inner_product_int(src[..., _perm_np(log_n, g)], ksk, mod, level, key_level, sp, k)
    calls = [("gathered", ctx.ksk_inner_product_galois, (g,))]
    if g == 1:
        calls.append(("plain", ctx.ksk_inner_product, ()))
    for name, ppad, dpad, off in KSIP_LAYOUTS:
        pst = rows * n + ppad
        dst = npoly * pst + dpad
        bi = _Blocks(mfhe, [j * dst + p * pst for j in range(nd) for p in range(npoly)], rows * n, off, src)
        for form, call, extra in calls:
            bo = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
            call(bi.t, d_ksk, bo.t, npoly, nd, level, key_level, sp, k, *extra, digit_stride=dst, poly_stride=pst,
                 acc_stride=bo.stride)
            torch.cuda.synchronize()
            bad = np.flatnonzero((bo.blocks((npoly, 2, rows, n)) != want).reshape(npoly, -1).any(axis=1))
            assert bad.size == 0, f"{name} {form}: {bad.size} wrong polynomials, the first {bad[:8].tolist()}"
            bo.check_pads()
        np.testing.assert_array_equal(bi.blocks((nd, npoly, rows, n)), src, err_msg=name)   # untouched
        bi.check_pads()
    np.testing.assert_array_equal(mfhe.to_host_u64(d_ksk), ksk.ravel())


# ---------------------------------------------------------------------------------------------------------------
# 2. automorphism: more than 65535 rows
# ---------------------------------------------------------------------------------------------------------------
# (rows, npoly): 65535 rows are the last that fit grid y alone (gz = 1); 65538 rows need a second z slab with three
# live rows and 65532 idle ones; 65543 polynomials of one row fold polynomials, not rows of one polynomial
AUTO_CASES = [(3, 21845), (3, 21846), (1, 65536 + 7)]


@pytest.mark.parametrize("rows,npoly", AUTO_CASES)
@pytest.mark.parametrize("log_n", [1, 4])
def test_automorphism_beyond_65535_rows(mfhe, log_n, rows, npoly):
    import torch
    (ctx, mod), n = _ctx3(log_n), 1 << log_n
    # launch_automorphism's fold (ks_fold, csrc/ks_host.hpp): gy = min(total, 65535), gz = ceil(total / gy)
    total = npoly * rows
    gy = min(total, 65535)
    assert -(-total // gy) == (1 if npoly == 21845 else 2)
    rng = np.random.default_rng(1000 * log_n + npoly)
    x = _random_rows(rng, (npoly,), mod[:rows], n)
    elts = (1, 3) if log_n == 1 else (5, pow(5, 7, 32), 31)
    for g in elts:
        pi = _perm_np(log_n, g)
        for name, ppad in (("dense", 0), ("padded-odd", 3)):    # the odd pad selects the scalar kernel
            bi = _polys(mfhe, npoly, rows, n, ppad, 0, x)
            bo = _polys(mfhe, npoly, rows, n, ppad + (2 if ppad % 2 == 0 else 4), 0)
            assert (bi.stride % 2, bo.stride % 2) == ((0, 0) if ppad == 0 else (1, 1))
            ctx.automorphism(bi.t, bo.t, npoly, rows, g, in_stride=bi.stride, out_stride=bo.stride)
            torch.cuda.synchronize()
            got = bo.blocks((npoly, rows, n))
            bad = np.flatnonzero((got != x[:, :, pi]).reshape(npoly, -1).any(axis=1))
            assert bad.size == 0, f"{name} g {g}: {bad.size} wrong polynomials, the first {bad[:8].tolist()}"
            bo.check_pads()
            np.testing.assert_array_equal(bi.blocks((npoly, rows, n)), x, err_msg=f"{name} g {g}")


# ---------------------------------------------------------------------------------------------------------------
# 3. the NTT-domain forms and the drivers where the NTT plan changes
# ---------------------------------------------------------------------------------------------------------------
# (log N, prime class, MFHE_OPT_NTT_PLAN_EFFECTIVE): the pipelined single pass (ntt_single14.hpp); two passes 7 + 7;
# two passes 8 + 8, whose column pass is the double-buffered one at the default MFHE_OPT_NTT_PREFETCH 2
PLANS = [pytest.param(14, F64_BITS, 4, id="2^14-f64-plan4"), pytest.param(14, U64_BITS, 2, id="2^14-u64-plan2"),
         pytest.param(16, U64_BITS, 2, id="2^16-u64-plan2"), pytest.param(16, F64_BITS, 2, id="2^16-f64-plan2")]
PLANS_GALOIS = PLANS[:3]


def _plan_ctx(mfhe, log_n, bits, plan):
    """The shared 5 + 2 limb context, after the assertions that make the test mean something: the plan the NTT calls
    will run, the arithmetic, the default prefetch and chunk size."""
    ctx = _ctx7(log_n, bits)
    assert ctx.info().arith == (mfhe.ARITH_F64 if bits == F64_BITS else mfhe.ARITH_U64)
    assert ctx.get_option(mfhe.OPT_NTT_PLAN) == 0 and ctx.get_option(mfhe.OPT_NTT_PREFETCH) == 2
    assert ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES) == 240 << 20
    assert ctx.get_option(mfhe.OPT_NTT_PLAN_EFFECTIVE) == plan
    return ctx, _moduli(log_n, bits), 1 << log_n


@pytest.mark.parametrize("log_n,bits,plan", PLANS)
def test_ntt_domain_forms_equal_the_composition_at_every_plan(mfhe, log_n, bits, plan):
    """mfhe_ntt_modup / mfhe_ntt_moddown against ntt_inv on dense copies of the rows, the rns_* call, ntt_fwd: the
    drivers transform parts of the workspace with start_limb != 0 and partial limb counts."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    batch = 3
    rng = np.random.default_rng(log_n + plan)
    ev = _random_rows(rng, (batch,), mod[:5], n)
    for ds, dc in ((0, 2), (2, 2), (4, 1)):
        bi = _polys(mfhe, batch, 5, n, 2, 0, ev)
        bo = _polys(mfhe, batch, 7, n, 4)
        ctx.ntt_modup(bi.t, bo.t, batch, 5, ds, dc, 5, 2, in_stride=bi.stride, out_stride=bo.stride)
        coef = mfhe.to_device_u64(ev.ravel())
        ctx.ntt_inv(coef, batch, 0, 5)
        comp = torch.zeros(batch * 7 * n, dtype=torch.int64, device="cuda")
        ctx.rns_modup(coef, comp, batch, n, 5, ds, dc, 5, 2)
        ctx.ntt_fwd(comp, batch, 0, 7)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks((batch, 7, n)), mfhe.to_host_u64(comp).reshape(batch, 7, n),
                                      err_msg=f"modup {ds}")
        bo.check_pads()
        np.testing.assert_array_equal(bi.blocks((batch, 5, n)), ev)
    ev7 = _random_rows(rng, (batch,), mod, n)
    for keep, drop in ((5, 2), (6, 1)):
        coef = mfhe.to_device_u64(ev7.ravel())
        ctx.ntt_inv(coef, batch, 0, 7)
        comp = torch.zeros(batch * keep * n, dtype=torch.int64, device="cuda")
        ctx.rns_moddown(coef, comp, batch, n, keep, keep, drop)
        ctx.ntt_fwd(comp, batch, 0, keep)
        torch.cuda.synchronize()
        want = mfhe.to_host_u64(comp).reshape(batch, keep, n)
        bi = _polys(mfhe, batch, 7, n, 2, 0, ev7)
        bo = _polys(mfhe, batch, keep, n, 4)
        ctx.ntt_moddown(bi.t, bo.t, batch, keep, keep, drop, in_stride=bi.stride, out_stride=bo.stride)
        ctx.ntt_moddown(bi.t, bi.t, batch, keep, keep, drop, in_stride=bi.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks((batch, keep, n)), want, err_msg=f"moddown keep {keep}")
        bo.check_pads()
        got = bi.blocks((batch, 7, n))
        np.testing.assert_array_equal(got[:, :keep], want, err_msg=f"moddown in place keep {keep}")
        np.testing.assert_array_equal(got[:, keep:], ev7[:, keep:])
        bi.check_pads()


# (key_level, alpha, special_start, nspecial, level): a partial last digit at levels 5 and 3; alpha 1 with one special
# limb that is not adjacent to the Q limbs
KS_SHAPES = [pytest.param(5, 2, 5, 2, 5, id="alpha2-level5"), pytest.param(5, 2, 5, 2, 3, id="alpha2-level3"),
             pytest.param(5, 1, 6, 1, 5, id="alpha1-K1")]


@pytest.mark.parametrize("key_level,alpha,sp,k,level", KS_SHAPES)
@pytest.mark.parametrize("log_n,bits,plan", PLANS)
def test_keyswitch_equals_the_composition_at_every_plan(mfhe, log_n, bits, plan, key_level, alpha, sp, k, level):
    """ntt_modup per digit, the inner product in Python integers, ntt_moddown per component, plus the addend."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    npoly = 2 if log_n == 14 else 1
    rng = np.random.default_rng(1000 * log_n + 100 * plan + 10 * alpha + level)
    kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
    ksk = _random_rows(rng, (-(-key_level // alpha), 2), kmod, n)
    d_ksk = mfhe.to_device_u64(ksk.ravel())
    x = _random_rows(rng, (npoly,), mod[:level], n)
    old = [_random_rows(rng, (npoly,), mod[:level], n) for _ in range(2)]
    plain = _composition(mfhe, ctx, mod, x, ksk, npoly, level, key_level, alpha, sp, k)
    q = np.array(mod[:level], dtype=object)[None, :, None]
    added = [((w.astype(object) + o.astype(object)) % q).astype(np.uint64) for w, o in zip(plain, old)]
    for flags, ipad, opad, want in ((0, 2, 4, plain), (mfhe.KS_ADD, 3, 5, added)):
        bi = _polys(mfhe, npoly, level, n, ipad, 0, x)
        b0 = _polys(mfhe, npoly, level, n, opad, 0, old[0])
        b1 = _polys(mfhe, npoly, level, n, opad, 0, old[1])
        ctx.keyswitch(bi.t, d_ksk, b0.t, b1.t, npoly, level, key_level, alpha, sp, k, flags, in_stride=bi.stride,
                      out_stride=b0.stride)
        torch.cuda.synchronize()
        msg = f"flags {flags} pads {ipad}, {opad}"
        np.testing.assert_array_equal(b0.blocks((npoly, level, n)), want[0], err_msg="out0 " + msg)
        np.testing.assert_array_equal(b1.blocks((npoly, level, n)), want[1], err_msg="out1 " + msg)
        b0.check_pads()
        b1.check_pads()
        np.testing.assert_array_equal(bi.blocks((npoly, level, n)), x, err_msg="input " + msg)
        bi.check_pads()
    np.testing.assert_array_equal(mfhe.to_host_u64(d_ksk), ksk.ravel())


@pytest.mark.parametrize("which", ["g=5", "g=2N-1"])
@pytest.mark.parametrize("log_n,bits,plan", PLANS_GALOIS)
def test_raise_and_galois_apply_equal_the_composition_at_every_plan(mfhe, log_n, bits, plan, which):
    """keyswitch_raise equals ntt_modup per digit; galois_apply_raised on those digits equals galois_apply and the
    composition: automorphism of c0, the gathered Python inner product, ntt_moddown per component, sigma_g(c0) added."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    g = 5 if which == "g=5" else 2 * n - 1
    npoly = 2 if log_n == 14 else 1
    level = key_level = sp = 5
    alpha, k = 2, 2
    rows, beta = level + k, 3
    rng = np.random.default_rng(2000 * log_n + 100 * plan + (g & 15))
    gk = _random_rows(rng, (beta, 2), mod, n)
    d_gk = mfhe.to_device_u64(gk.ravel())
    c0 = _random_rows(rng, (npoly,), mod[:level], n)
    c1 = _random_rows(rng, (npoly,), mod[:level], n)
    b0 = _polys(mfhe, npoly, level, n, 2, 0, c0)
    b1 = _polys(mfhe, npoly, level, n, 2, 0, c1)
    pst = rows * n + 2
    dst = npoly * pst + 2
    br = _Blocks(mfhe, [j * dst + p * pst for j in range(beta) for p in range(npoly)], rows * n)
    ctx.keyswitch_raise(b1.t, br.t, npoly, level, alpha, sp, k, in_stride=b1.stride, digit_stride=dst, poly_stride=pst)
    torch.cuda.synchronize()
    br.check_pads()
    raised = br.blocks((beta, npoly, rows, n)).copy()
    d_in = mfhe.to_device_u64(c1.ravel())
    for j, (ds, dc) in enumerate(km.digits(level, alpha)):
        up = torch.zeros(npoly * rows * n, dtype=torch.int64, device="cuda")
        ctx.ntt_modup(d_in, up, npoly, level, ds, dc, sp, k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(raised[j], mfhe.to_host_u64(up).reshape(npoly, rows, n), err_msg=f"digit {j}")
    o0, o1, h0, h1 = (_polys(mfhe, npoly, level, n, 4) for _ in range(4))
    ctx.galois_apply(b0.t, b1.t, d_gk, o0.t, o1.t, npoly, level, key_level, alpha, sp, k, g, in_stride=b0.stride,
                     out_stride=o0.stride)
    ctx.galois_apply_raised(b0.t, br.t, d_gk, h0.t, h1.t, npoly, level, key_level, alpha, sp, k, g, in_stride=b0.stride,
                            digit_stride=dst, poly_stride=pst, out_stride=h0.stride)
    torch.cuda.synchronize()
    want = _galois_composition(mfhe, ctx, mod, c0, c1, gk, npoly, level, key_level, alpha, sp, k, g)
    for got, hoisted, w, name in ((o0, h0, want[0], "out0"), (o1, h1, want[1], "out1")):
        np.testing.assert_array_equal(got.blocks((npoly, level, n)), w, err_msg=name)
        np.testing.assert_array_equal(hoisted.blocks((npoly, level, n)), w, err_msg="hoisted " + name)
        got.check_pads()
        hoisted.check_pads()
    np.testing.assert_array_equal(br.blocks((beta, npoly, rows, n)), raised, err_msg="raised digits are only read")
    br.check_pads()
    np.testing.assert_array_equal(b0.blocks((npoly, level, n)), c0)
    np.testing.assert_array_equal(b1.blocks((npoly, level, n)), c1)
    np.testing.assert_array_equal(mfhe.to_host_u64(d_gk), gk.ravel())


def test_drivers_return_the_same_bits_with_one_polynomial_per_chunk(mfhe):
    """N = 2^16, U64: with MFHE_OPT_NTT_CHUNK_BYTES = 8 N, one limb of one polynomial, every NTT call of the drivers
    (the narrowest transforms a single limb) walks its batch one polynomial at a time.  3 polynomials: ModUp batches
    of 3, the ModDown of both components a batch of 6."""
    import torch
    log_n = 16
    ctx, mod, n = _plan_ctx(mfhe, log_n, U64_BITS, 2)
    npoly, level, key_level, alpha, sp, k, g = 3, 5, 5, 2, 5, 2, 5
    rng = np.random.default_rng(16)
    d_key = mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, n).ravel())
    d0 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    d1 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())

    def run():
        outs = [torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda") for _ in range(4)]
        ctx.keyswitch(d1, d_key, outs[0], outs[1], npoly, level, key_level, alpha, sp, k)
        ctx.galois_apply(d0, d1, d_key, outs[2], outs[3], npoly, level, key_level, alpha, sp, k, g)
        torch.cuda.synchronize()
        return [mfhe.to_host_u64(o).copy() for o in outs]

    whole = run()
    default = ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES)
    assert default >= 2 * npoly * 7 * n * 8, "the default holds every batch of these calls in one chunk"
    try:
        ctx.set_option(mfhe.OPT_NTT_CHUNK_BYTES, 8 * n)
        chunked = run()
    finally:
        ctx.set_option(mfhe.OPT_NTT_CHUNK_BYTES, default)
    assert ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES) == default
    for name, a, b in zip(("keyswitch out0", "keyswitch out1", "galois out0", "galois out1"), whole, chunked):
        assert a.any(), name
        np.testing.assert_array_equal(a, b, err_msg=name)


# ---------------------------------------------------------------------------------------------------------------
# 4. a key switch at N = 2^14 checked by its decryption error, without the library's ModUp and ModDown
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [5, 3])
def test_keyswitch_decrypts_within_the_bound_at_n_2_to_14(mfhe, orc, level):
    """out0 + out1 s_to - c s_from, formed limb by limb in Python integers, brought to coefficients by the oracle's CPU
    transform and CRT-composed over the level limbs, is at most ks_model.error_bound with B = ceil(6 sigma) + 1, the
    clip of gen_switch_key; and it is not 0: the key carries noise."""
    import math
    import torch
    log_n, sigma = 14, 3.2
    ctx, mod, n = _plan_ctx(mfhe, log_n, F64_BITS, 4)
    q, p = list(mod[:5]), list(mod[5:])
    key_level, alpha, sp, k = 5, 2, 5, 2
    rnd = random.Random(14)
    s_from = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    s_to = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    sf = orc.phantom_fwd(_residues([s_from], mod).ravel(), 7, log_n, mod).reshape(7, n)
    st = orc.phantom_fwd(_residues([s_to], mod).ravel(), 7, log_n, mod).reshape(7, n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(14)
    ksk = ctx.gen_switch_key(mfhe.to_device_u64(sf.ravel()), mfhe.to_device_u64(st.ravel()), key_level, alpha, sp, k,
                             generator=gen, sigma=sigma)
    c = _random_rows(np.random.default_rng(level), (1,), mod[:level], n)
    o0 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
    ctx.keyswitch(mfhe.to_device_u64(c.ravel()), ksk, o0, o1, 1, level, key_level, alpha, sp, k)
    torch.cuda.synchronize()
    h0 = mfhe.to_host_u64(o0).reshape(level, n).astype(object)
    h1 = mfhe.to_host_u64(o1).reshape(level, n).astype(object)
    qcol = np.array(q[:level], dtype=object)[:, None]
    diff = ((h0 + h1 * st[:level].astype(object) - c[0].astype(object) * sf[:level].astype(object)) % qcol)
    coef = orc.phantom_inv(diff.astype(np.uint64).ravel(), level, log_n, q[:level]).reshape(level, n).astype(object)
    Ql = km.prod(q[:level])
    lift = [(Ql // qi) * pow(Ql // qi, -1, qi) for qi in q[:level]]
    tot = sum(coef[r] * lift[r] for r in range(level)) % Ql
    err = max(abs(km.centered(int(v), Ql)) for v in tot)
    bound = km.error_bound(q, p, alpha, level, n, math.ceil(6 * sigma) + 1)
    print(f"keyswitch N 2^14 level {level}: error {err}, bound {bound:.2f}")
    assert bound < Ql // 4, "the bound must mean something mod Q_level"
    assert err <= bound
    assert err > 0
