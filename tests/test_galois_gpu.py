"""GPU checks of Galois automorphisms and hoisted rotations (csrc/galois.hip, csrc/keyswitch.hip; include/mfhe.h
mfhe_ntt_automorphism, mfhe_ksk_inner_product_galois, mfhe_keyswitch_raise, mfhe_galois_apply_raised, mfhe_galois_apply,
mfhe_galois_reserve and the Python layer's gen_galois_key), bit-exact against Python integers: the gather of
tests/galois_model.py, the formulas computed here, the composition of the public pieces and the coefficient-domain
model.  Every comparison is exact equality: the arithmetic is integer (ModDown's one f64 sum only selects the multiple
of P; tests/test_galois_cpu.py shows the model's seeded inputs stay 2^-30 P away from where it could flip)."""
import functools
import random

import numpy as np
import pytest

import galois_model as gm
import ks_model as km
from primes import primes_of_size
from test_keyswitch_gpu import (_Blocks, _device_key, _inner_product_int, _moduli, _polys, _random_rows, _residues,
                                _row_limbs, _u64)

pytestmark = pytest.mark.gpu

# (name, poly pad, outer pad, base offset in words): even pads keep the 16-byte form, the odd pad and the one-word
# (8-byte) offset force the scalar variant
LAYOUTS = [("dense", 0, 0, 0), ("padded", 2, 4, 0), ("padded-odd", 3, 5, 0), ("misaligned", 0, 0, 1)]


def _perm_np(log_n, g):
    """galois_model.perm as a numpy index array."""
    def br(x):
        r = np.zeros_like(x)
        for b in range(log_n):
            r |= ((x >> b) & 1) << (log_n - 1 - b)
        return r
    i = np.arange(1 << log_n, dtype=np.int64)
    return br((((2 * br(i) + 1) * g) % (2 << log_n) - 1) // 2)


def _elts(log_n):
    m = 2 << log_n
    base = {1, 3 % m, 5 % m, pow(5, 7, m), pow(5, 1000, m), m - 1}
    return sorted(base | set(range(1, m, 2))) if log_n == 4 else sorted(base)


@functools.lru_cache(maxsize=None)
def _ctx3(log_n):
    import mfhe
    mod = primes_of_size(50, 2 << log_n, 3)
    return mfhe.Context(mod, log_n, mfhe.CONV_PHANTOM), tuple(mod)


@functools.lru_cache(maxsize=None)
def _ctx7(log_n, bits):
    import mfhe
    return mfhe.Context(list(_moduli(log_n, bits)), log_n, mfhe.CONV_PHANTOM)


# ---------------------------------------------------------------------------------------------------------------
# the automorphism
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 4, 8])
def test_automorphism_equals_the_gather(mfhe, log_n):
    import torch
    (ctx, mod), n, rows = _ctx3(log_n), 1 << log_n, 3
    rng = np.random.default_rng(log_n)
    x = _random_rows(rng, (5,), mod, n)
    for g in _elts(log_n):
        pi = _perm_np(log_n, g)
        assert pi.tolist() == gm.perm(log_n, g)
        for npoly in (1, 5):
            for name, ppad, _, off in (LAYOUTS if g in (1, 3 % (2 * n), 2 * n - 1) or log_n != 4 else LAYOUTS[:1]):
                src = np.ascontiguousarray(x[:npoly])
                bi = _polys(mfhe, npoly, rows, n, ppad, off, src)
                bo = _polys(mfhe, npoly, rows, n, ppad + (2 if ppad % 2 == 0 else 4), off)
                ctx.automorphism(bi.t, bo.t, npoly, rows, g, in_stride=bi.stride, out_stride=bo.stride)
                torch.cuda.synchronize()
                msg = f"{name} g {g} npoly {npoly}"
                np.testing.assert_array_equal(bo.blocks((npoly, rows, n)), src[:, :, pi], err_msg=msg)
                bo.check_pads()
                np.testing.assert_array_equal(bi.blocks((npoly, rows, n)), src, err_msg=msg)


def test_automorphism_at_n_2_to_17(mfhe):
    """One polynomial of one row at log N = 17, the largest the context takes: 32-bit index arithmetic suffices."""
    import torch
    log_n, n = 17, 1 << 17
    mod = primes_of_size(50, 2 << log_n, 1)
    ctx = mfhe.Context(mod, log_n, mfhe.CONV_PHANTOM)
    rng = np.random.default_rng(17)
    x = rng.integers(0, 2 ** 63, n, dtype=np.uint64) % np.uint64(mod[0])
    d_in = mfhe.to_device_u64(x)
    for g in (1, 3, 5, pow(5, 1000, 2 * n), 2 * n - 1):
        out = torch.zeros(n, dtype=torch.int64, device="cuda")
        ctx.automorphism(d_in, out, 1, 1, g)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(out), x[_perm_np(log_n, g)], err_msg=f"g {g}")


def test_automorphism_is_sigma_in_the_coefficient_domain_and_composes(mfhe):
    """N = 16: ntt_inv -> sigma_g in Python -> ntt_fwd equals the device gather; sigma_g sigma_h = sigma_(gh mod 2N);
    sigma_g then sigma_(g^-1) is the identity."""
    import torch
    (ctx, mod), n, rows = _ctx3(4), 16, 3
    rnd = random.Random(4)
    polys = [[rnd.randrange(-(1 << 40), 1 << 40) for _ in range(n)] for _ in range(2)]
    ev = ctx.ntt_fwd(mfhe.to_device_u64(_residues(polys, mod).ravel()), 2, 0, 3)

    def auto(t, g):
        out = torch.zeros(2 * rows * n, dtype=torch.int64, device="cuda")
        return ctx.automorphism(t, out, 2, rows, g)

    for g in range(1, 32, 2):
        want = ctx.ntt_fwd(mfhe.to_device_u64(_residues([gm.sigma(p, g) for p in polys], mod).ravel()), 2, 0, 3)
        got = auto(ev, g)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(got), mfhe.to_host_u64(want), err_msg=f"g {g}")
        back = auto(got, pow(g, -1, 32))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(back), mfhe.to_host_u64(ev), err_msg=f"g {g} inverse")
    for g in (3, 5, 25, 31):
        for h in (5, 13, 31):
            a, b = auto(auto(ev, h), g), auto(ev, g * h % 32)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(mfhe.to_host_u64(a), mfhe.to_host_u64(b), err_msg=f"g {g} h {h}")


# ---------------------------------------------------------------------------------------------------------------
# the gathered inner product
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 4, 8])
def test_gathered_inner_product_bit_exact(mfhe, log_n):
    """Digits 1 .. 7 (every unrolled count and the generic loop), 1, 5 and 9 polynomials (a thread's run of 4, a second
    run, a tail), the 16-byte and the scalar form; g = 1 equals ksk_inner_product bit for bit."""
    import torch
    bits = (50, 61)
    ctx, mod, n = _ctx7(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(30 + log_n)
    key_level, sp, k = 5, 5, 2
    m2 = 2 * n
    for level in (5, 3):
        rows = level + k
        rmod = [mod[l] for l in _row_limbs(level, sp, k)]
        kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
        raised = _random_rows(rng, (7, 9), rmod, n)            # [nd][npoly][rows][n]
        ksk = _random_rows(rng, (7, 2), kmod, n)               # [nd][2][key_rows][n]
        d_ksk = mfhe.to_device_u64(ksk.ravel())
        for nd in range(1, 8):
            if level == 3 and nd not in (3, 7):
                continue
            # every element at 1, 3 and 7 digits; the other unrolled counts with one rotation
            for g in (sorted({1, 3 % m2, pow(5, 7, m2), m2 - 1}) if nd in (1, 3, 7) else [pow(5, 7, m2)]):
                pi = _perm_np(log_n, g)
                want = _inner_product_int(raised[:nd][..., pi], ksk, mod, level, key_level, sp, k)
                for npoly in (1, 5, 9):
                    full = nd in (1, 3, 7) and g != 1
                    for name, ppad, dpad, off in (LAYOUTS if full else (LAYOUTS[0], LAYOUTS[3])):
                        pst = rows * n + ppad
                        dst = npoly * pst + dpad
                        src = np.ascontiguousarray(raised[:nd, :npoly])
                        bi = _Blocks(mfhe, [j * dst + p * pst for j in range(nd) for p in range(npoly)], rows * n, off,
                                     src)
                        bo = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
                        ctx.ksk_inner_product_galois(bi.t, d_ksk, bo.t, npoly, nd, level, key_level, sp, k, g,
                                                     digit_stride=dst, poly_stride=pst, acc_stride=bo.stride)
                        torch.cuda.synchronize()
                        msg = f"{name} level {level} nd {nd} g {g} npoly {npoly}"
                        got = bo.blocks((npoly, 2, rows, n))
                        np.testing.assert_array_equal(got, want[:npoly], err_msg=msg)
                        bo.check_pads()
                        np.testing.assert_array_equal(bi.blocks((nd, npoly, rows, n)), src, err_msg=msg)   # untouched
                        if g == 1:
                            bp = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
                            ctx.ksk_inner_product(bi.t, d_ksk, bp.t, npoly, nd, level, key_level, sp, k,
                                                  digit_stride=dst, poly_stride=pst, acc_stride=bp.stride)
                            torch.cuda.synchronize()
                            np.testing.assert_array_equal(got, bp.blocks((npoly, 2, rows, n)), err_msg=msg)
        np.testing.assert_array_equal(mfhe.to_host_u64(d_ksk), ksk.ravel())


def test_gathered_inner_product_18_digits_of_62_bit_operands(mfhe):
    """Every operand q - 1 with 62-bit primes: 18 products overflow a u128 unless the sum is reduced after 16 terms.
    18 (q - 1)^2 = 18 mod q, whatever the gather."""
    import torch
    mod = primes_of_size(62, 32, 3)
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    n, nd, level, k = 16, 18, 2, 1
    rows = level + k
    top = _u64(mod) - np.uint64(1)
    raised = np.broadcast_to(top[None, None, :, None], (nd, 3, rows, n)).copy()
    ksk = np.broadcast_to(top[None, None, :, None], (nd, 2, rows, n)).copy()
    d_ksk = mfhe.to_device_u64(ksk.ravel())
    for g in (3, 31):
        for npoly in (1, 3):
            for name, ppad, dpad, off in LAYOUTS:
                pst = rows * n + ppad
                dst = npoly * pst + dpad
                src = np.ascontiguousarray(raised[:, :npoly])
                bi = _Blocks(mfhe, [j * dst + p * pst for j in range(nd) for p in range(npoly)], rows * n, off, src)
                bo = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
                ctx.ksk_inner_product_galois(bi.t, d_ksk, bo.t, npoly, nd, level, level, level, k, g, digit_stride=dst,
                                             poly_stride=pst, acc_stride=bo.stride)
                torch.cuda.synchronize()
                assert (bo.blocks((npoly, 2, rows, n)) == np.uint64(18)).all(), f"{name} g {g} npoly {npoly}"
                bo.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# the drivers against the composition of the public pieces
# ---------------------------------------------------------------------------------------------------------------
def _composition(mfhe, ctx, mod, c0, c1, gk, npoly, level, key_level, alpha, sp, k, g):
    """ntt_modup per digit -> the Python gathered inner product -> ntt_moddown per component, automorphism(c0) added in
    Python: (out0, out1), each [npoly][level][N] uint64."""
    import torch
    n, rows, log_n = ctx.N, level + k, ctx.N.bit_length() - 1
    d_in = mfhe.to_device_u64(c1.ravel())
    raised = []
    for ds, dc in km.digits(level, alpha):
        up = torch.zeros(npoly * rows * n, dtype=torch.int64, device="cuda")
        ctx.ntt_modup(d_in, up, npoly, level, ds, dc, sp, k)
        torch.cuda.synchronize()
        raised.append(mfhe.to_host_u64(up).reshape(npoly, rows, n).copy())
    pi = _perm_np(log_n, g)
    acc = _inner_product_int(np.stack(raised)[..., pi], gk, mod, level, key_level, sp, k)
    outs = []
    for c in range(2):
        d_acc = mfhe.to_device_u64(np.ascontiguousarray(acc[:, c]).ravel())
        down = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
        ctx.ntt_moddown(d_acc, down, npoly, level, sp, k)
        torch.cuda.synchronize()
        outs.append(mfhe.to_host_u64(down).reshape(npoly, level, n).copy())
    rot = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    ctx.automorphism(mfhe.to_device_u64(c0.ravel()), rot, npoly, level, g)
    torch.cuda.synchronize()
    q = np.array(mod[:level], dtype=object)[None, :, None]
    s0 = mfhe.to_host_u64(rot).reshape(npoly, level, n)
    np.testing.assert_array_equal(s0, c0[:, :, pi])
    outs[0] = ((outs[0].astype(object) + s0.astype(object)) % q).astype(np.uint64)
    return outs


# (key_level, alpha, special_start, nspecial, levels), as tests/test_keyswitch_gpu.py
GA_CASES = [(5, 2, 5, 2, (5, 3, 2)), (5, 1, 6, 1, (5,)), (5, 5, 5, 2, (5,))]


@pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("log_n", [4, 8])
def test_galois_apply_equals_the_composition_and_hoists(mfhe, log_n, bits):
    """galois_apply equals the public pieces; one keyswitch_raise followed by galois_apply_raised for three elements
    equals galois_apply for each, and leaves the raised digits as they were."""
    import torch
    ctx, mod, n = _ctx7(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(40 + log_n)
    npoly, m2 = 2, 2 << log_n
    elts = (5 % m2, pow(5, 7, m2), m2 - 1)
    for key_level, alpha, sp, k, levels in GA_CASES:
        kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
        gk = _random_rows(rng, (-(-key_level // alpha), 2), kmod, n)
        d_gk = mfhe.to_device_u64(gk.ravel())
        for level in levels:
            rows, beta = level + k, -(-level // alpha)
            c0 = _random_rows(rng, (npoly,), mod[:level], n)
            c1 = _random_rows(rng, (npoly,), mod[:level], n)
            for ipad, opad, rpad in ((0, 0, 0), (2, 4, 2), (3, 5, 1)):
                b0 = _polys(mfhe, npoly, level, n, ipad, 0, c0)
                b1 = _polys(mfhe, npoly, level, n, ipad, 0, c1)
                pst = rows * n + rpad
                dst = npoly * pst + rpad
                br = _Blocks(mfhe, [j * dst + p * pst for j in range(beta) for p in range(npoly)], rows * n)
                ctx.keyswitch_raise(b1.t, br.t, npoly, level, alpha, sp, k, in_stride=b1.stride, digit_stride=dst,
                                    poly_stride=pst)
                torch.cuda.synchronize()
                br.check_pads()
                raised = br.blocks((beta, npoly, rows, n)).copy()
                for g in elts:
                    msg = f"alpha {alpha} K {k} level {level} g {g} pads {ipad}, {opad}, {rpad}"
                    o0 = _polys(mfhe, npoly, level, n, opad)
                    o1 = _polys(mfhe, npoly, level, n, opad)
                    ctx.galois_apply(b0.t, b1.t, d_gk, o0.t, o1.t, npoly, level, key_level, alpha, sp, k, g,
                                     in_stride=b0.stride, out_stride=o0.stride)
                    h0 = _polys(mfhe, npoly, level, n, opad)
                    h1 = _polys(mfhe, npoly, level, n, opad)
                    ctx.galois_apply_raised(b0.t, br.t, d_gk, h0.t, h1.t, npoly, level, key_level, alpha, sp, k, g,
                                            in_stride=b0.stride, digit_stride=dst, poly_stride=pst,
                                            out_stride=h0.stride)
                    torch.cuda.synchronize()
                    got = [o0.blocks((npoly, level, n)), o1.blocks((npoly, level, n))]
                    if ipad == 0 or g == elts[0]:
                        want = _composition(mfhe, ctx, mod, c0, c1, gk, npoly, level, key_level, alpha, sp, k, g)
                        np.testing.assert_array_equal(got[0], want[0], err_msg="out0 " + msg)
                        np.testing.assert_array_equal(got[1], want[1], err_msg="out1 " + msg)
                    np.testing.assert_array_equal(h0.blocks((npoly, level, n)), got[0], err_msg="hoisted out0 " + msg)
                    np.testing.assert_array_equal(h1.blocks((npoly, level, n)), got[1], err_msg="hoisted out1 " + msg)
                    for b in (o0, o1, h0, h1):
                        b.check_pads()
                    np.testing.assert_array_equal(br.blocks((beta, npoly, rows, n)), raised, err_msg="raised " + msg)
                    br.check_pads()
                np.testing.assert_array_equal(b0.blocks((npoly, level, n)), c0)
                np.testing.assert_array_equal(b1.blocks((npoly, level, n)), c1)
        np.testing.assert_array_equal(mfhe.to_host_u64(d_gk), gk.ravel())


# ---------------------------------------------------------------------------------------------------------------
# the driver against the coefficient-domain model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("g", gm.CASE_ELTS)
def test_galois_apply_equals_the_model(mfhe, bits, g):
    """N = 16, the seeded inputs of tests/test_galois_cpu.py: the Galois key assembled on the device from
    automorphism(s), the rotation back through ntt_inv equals the model's hoisted rotation on every limb."""
    import torch
    cs = gm.seeded_case(bits, g)
    q, p, n = cs["q"], cs["p"], cs["n"]
    mod = q + p
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    gk = _device_key(mfhe, ctx, cs)
    # s_from of the key is the device automorphism of s
    sv = ctx.ntt_fwd(mfhe.to_device_u64(_residues([cs["s"]], mod).ravel()), 1, 0, 7)
    sf = ctx.automorphism(sv, torch.zeros_like(sv), 1, 7, g)
    want_sf = ctx.ntt_fwd(mfhe.to_device_u64(_residues([cs["s_from"]], mod).ravel()), 1, 0, 7)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mfhe.to_host_u64(sf), mfhe.to_host_u64(want_sf))
    for level in km.CASE_LEVELS:
        c0, c1 = cs["ct"][level]
        w0, w1, margin = gm.rotate(q, p, cs["alpha"], level, c0, c1, cs["key"], g)
        assert margin >= 2.0 ** -30
        d = ctx.ntt_fwd(mfhe.to_device_u64(_residues([c0, c1], q[:level]).ravel()), 2, 0, level)
        o0 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        o1 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        ctx.galois_apply(d[:level * n], d[level * n:], gk, o0, o1, 1, level, 5, cs["alpha"], 5, 2, g)
        ctx.ntt_inv(o0, 1, 0, level)
        ctx.ntt_inv(o1, 1, 0, level)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(o0).reshape(1, level, n), _residues([w0], q[:level]),
                                      err_msg=f"out0 level {level}")
        np.testing.assert_array_equal(mfhe.to_host_u64(o1).reshape(1, level, n), _residues([w1], q[:level]),
                                      err_msg=f"out1 level {level}")


# ---------------------------------------------------------------------------------------------------------------
# end to end: encrypt, rotate, decrypt
# ---------------------------------------------------------------------------------------------------------------
def test_rotation_and_conjugation_decrypt_at_n_256(mfhe):
    """A Python RLWE encryption (c0, c1) = (m + e - a s, a) of a small message under a ternary s at N = 256; Galois keys
    from gen_galois_key for g = galois_elt(1) and the conjugation.  After galois_apply, out0 + out1 s is
    sigma_g(m + e) within ks_model.error_bound (|e_key| <= 6 sigma = 19 = B_E)."""
    import torch
    log_n, n, bits = 8, 256, (50, 61)
    ctx, mod = _ctx7(log_n, bits), list(_moduli(log_n, bits))
    q, p = mod[:5], mod[5:]
    level, key_level, alpha, sp, k = 5, 5, 2, 5, 2
    Ql = km.prod(q)
    rnd = random.Random(256)
    s = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    m = [rnd.randint(-1000, 1000) for _ in range(n)]
    e = [rnd.randint(-km.B_E, km.B_E) for _ in range(n)]
    a = [rnd.randrange(Ql) for _ in range(n)]
    c0 = [(mv + ev - v) % Ql for mv, ev, v in zip(m, e, km.negacyclic(a, s, Ql))]
    d = ctx.ntt_fwd(mfhe.to_device_u64(_residues([c0, a], q).ravel()), 2, 0, level)
    sv = ctx.ntt_fwd(mfhe.to_device_u64(_residues([s], mod).ravel()), 1, 0, 7)
    lift = [(Ql // qi) * pow(Ql // qi, -1, qi) for qi in q]
    bound = km.error_bound(q, p, alpha, level, n, km.B_E)
    assert bound < Ql // 4
    plain = [mv + ev for mv, ev in zip(m, e)]
    for g in (mfhe.galois_elt(1, log_n), mfhe.galois_conj(log_n)):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(g)
        gk = ctx.gen_galois_key(sv, g, key_level, alpha, sp, k, generator=gen)
        o0 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        o1 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        ctx.galois_apply(d[:level * n], d[level * n:], gk, o0, o1, 1, level, key_level, alpha, sp, k, g)
        ctx.ntt_inv(o0, 1, 0, level)
        ctx.ntt_inv(o1, 1, 0, level)
        torch.cuda.synchronize()
        outs = []
        for t in (o0, o1):
            h = mfhe.to_host_u64(t).reshape(level, n).astype(object)
            outs.append([int(v) for v in sum(h[r] * lift[r] for r in range(level)) % Ql])
        dec = [(x + y) % Ql for x, y in zip(outs[0], km.negacyclic(outs[1], s, Ql))]
        err = max(abs(km.centered(x - y, Ql)) for x, y in zip(dec, gm.sigma(plain, g)))
        print(f"rotation g {g}: error {err}, bound {bound:.2f}")
        assert err <= bound
        if g != 1:
            assert max(abs(km.centered(x - y, Ql)) for x, y in zip(dec, plain)) > bound, "the slots did move"


# ---------------------------------------------------------------------------------------------------------------
# graph capture, argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After galois_reserve, galois_apply allocates nothing and copies nothing to the device: it is captured into a
    graph (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed on fresh inputs; the replay
    equals the eager call on those inputs."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, n = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    npoly, level, key_level, alpha, sp, k, g = 2, 5, 5, 2, 5, 2, 25
    ctx.galois_reserve(npoly, level, key_level, alpha, sp, k)
    rng = np.random.default_rng(5)
    gk = mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, n).ravel())
    d0 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    d1 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    o0 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx.galois_apply(d0, d1, gk, o0, o1, npoly, level, key_level, alpha, sp, k, g)
    first = None
    for _ in range(2):                                         # the captured inputs, then fresh ones
        o0.zero_()
        o1.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = (mfhe.to_host_u64(o0).copy(), mfhe.to_host_u64(o1).copy())
        e0, e1 = torch.zeros_like(o0), torch.zeros_like(o1)
        ctx.galois_apply(d0, d1, gk, e0, e1, npoly, level, key_level, alpha, sp, k, g)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[0], mfhe.to_host_u64(e0))
        np.testing.assert_array_equal(got[1], mfhe.to_host_u64(e1))
        assert got[0].any() and got[1].any()
        if first is not None:
            assert (first[0] != got[0]).any() and (first[1] != got[1]).any()
        first = got
        d0.copy_(mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel()))
        d1.copy_(mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel()))


def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    mod, N = _moduli(4, (45, 49)), 16
    ctx = mfhe.Context(list(mod), 4, mfhe.CONV_PHANTOM)
    h = ctx.handle
    bufs = {name: _polys(mfhe, 1, 3 * 2 * 7, N) for name in ("c0", "c1", "gk", "o0", "o1", "rs")}
    p0, p1, pk, q0, q1, pr = (bufs[name].t.data_ptr() for name in ("c0", "c1", "gk", "o0", "o1", "rs"))
    E = mfhe.EINVAL
    L5, L7 = 5 * N, 7 * N

    def au(i=p0, ist=L5, o=q0, ost=L5, npoly=1, rows=5, g=3):
        return lib.mfhe_ntt_automorphism(h, i, ist, o, ost, npoly, rows, g, None)

    def ip(r=pr, dst=L7, pst=L7, key=pk, acc=q0, ast=2 * L7, npoly=1, nd=3, level=5, kl=5, sp=5, k=2, g=3):
        return lib.mfhe_ksk_inner_product_galois(h, r, dst, pst, key, acc, ast, npoly, nd, level, kl, sp, k, g, None)

    def rs(i=p1, ist=L5, r=pr, dst=L7, pst=L7, npoly=1, level=5, alpha=2, sp=5, k=2):
        return lib.mfhe_keyswitch_raise(h, i, ist, r, dst, pst, npoly, level, alpha, sp, k, None)

    def ar(c0=p0, ist=L5, r=pr, dst=L7, pst=L7, key=pk, o0=q0, o1=q1, ost=L5, npoly=1, level=5, kl=5, alpha=2, sp=5,
           k=2, g=3):
        return lib.mfhe_galois_apply_raised(h, c0, ist, r, dst, pst, key, o0, o1, ost, npoly, level, kl, alpha, sp, k,
                                            g, None)

    def ap(c0=p0, c1=p1, ist=L5, key=pk, o0=q0, o1=q1, ost=L5, npoly=1, level=5, kl=5, alpha=2, sp=5, k=2, g=3):
        return lib.mfhe_galois_apply(h, c0, c1, ist, key, o0, o1, ost, npoly, level, kl, alpha, sp, k, g, None)

    cases = {}
    for name, fn in (("automorphism", au), ("inner product", ip), ("apply_raised", ar), ("apply", ap)):
        cases[f"{name} even g"] = lambda fn=fn: fn(g=4)
        cases[f"{name} g < 1"] = lambda fn=fn: fn(g=0)
        cases[f"{name} g negative"] = lambda fn=fn: fn(g=-3)
        cases[f"{name} g >= 2N"] = lambda fn=fn: fn(g=33)
    cases.update({
        "automorphism null in": lambda: au(i=None),
        "automorphism null out": lambda: au(o=None),
        "automorphism in stride": lambda: au(ist=L5 - 1, npoly=2),
        "automorphism out stride": lambda: au(ost=L5 - 1, npoly=2),
        "automorphism rows < 0": lambda: au(rows=-1),
        "automorphism in place": lambda: au(o=p0),
        "automorphism overlap": lambda: au(o=p0 + 8 * N),
        "inner product null raised": lambda: ip(r=None),
        "inner product null key": lambda: ip(key=None),
        "inner product null acc": lambda: ip(acc=None),
        "inner product ndigits < 1": lambda: ip(nd=0),
        "inner product poly stride": lambda: ip(pst=L7 - 1),
        "inner product acc stride": lambda: ip(ast=2 * L7 - 1),
        "inner product digit stride": lambda: ip(dst=L7 - 1),
        "inner product level > key_level": lambda: ip(kl=4),
        "raise null in": lambda: rs(i=None),
        "raise null raised": lambda: rs(r=None),
        "raise alpha < 1": lambda: rs(alpha=0),
        "raise nspecial < 1": lambda: rs(k=0),
        "raise level < 1": lambda: rs(level=0),
        "raise special overlaps Q": lambda: rs(sp=4),
        "raise special outside": lambda: rs(sp=6),
        "raise in stride": lambda: rs(ist=L5 - 1, npoly=2),
        "raise poly stride": lambda: rs(pst=L7 - 1),
        "raise digit stride": lambda: rs(dst=L7 - 1),
        "raise in is raised": lambda: rs(r=p1),
        "apply_raised null c0": lambda: ar(c0=None),
        "apply_raised null raised": lambda: ar(r=None),
        "apply_raised null key": lambda: ar(key=None),
        "apply_raised null out0": lambda: ar(o0=None),
        "apply_raised null out1": lambda: ar(o1=None),
        "apply_raised alpha < 1": lambda: ar(alpha=0),
        "apply_raised level > key_level": lambda: ar(kl=4),
        "apply_raised special outside": lambda: ar(sp=6),
        "apply_raised in stride": lambda: ar(ist=L5 - 1, npoly=2),
        "apply_raised out stride": lambda: ar(ost=L5 - 1, npoly=2),
        "apply_raised poly stride": lambda: ar(pst=L7 - 1),
        "apply_raised digit stride": lambda: ar(dst=L7 - 1),
        "apply_raised c0 is out0": lambda: ar(o0=p0),
        "apply_raised c0 is out1": lambda: ar(o1=p0),
        "apply_raised raised overlaps out1": lambda: ar(o1=pr + 8 * N),
        "apply_raised outputs overlap": lambda: ar(o1=q0 + 8 * N),
        "apply null c0": lambda: ap(c0=None),
        "apply null c1": lambda: ap(c1=None),
        "apply null key": lambda: ap(key=None),
        "apply null out0": lambda: ap(o0=None),
        "apply null out1": lambda: ap(o1=None),
        "apply alpha < 1": lambda: ap(alpha=0),
        "apply nspecial < 1": lambda: ap(k=0),
        "apply level > key_level": lambda: ap(kl=4),
        "apply in stride": lambda: ap(ist=L5 - 1, npoly=2),
        "apply out stride": lambda: ap(ost=L5 - 1, npoly=2),
        "apply c0 is out0": lambda: ap(o0=p0),
        "apply c1 is out1": lambda: ap(o1=p1),
        "apply c1 overlaps out0": lambda: ap(o0=p1 + 8 * N),
        "apply outputs overlap": lambda: ap(o1=q0),
        "reserve alpha < 1": lambda: lib.mfhe_galois_reserve(h, 1, 5, 5, 0, 5, 2),
        "reserve nspecial < 1": lambda: lib.mfhe_galois_reserve(h, 1, 5, 5, 2, 5, 0),
        "reserve level > key_level": lambda: lib.mfhe_galois_reserve(h, 1, 5, 4, 2, 5, 2),
        "reserve special outside": lambda: lib.mfhe_galois_reserve(h, 1, 5, 5, 2, 6, 2),
    })
    for name, call in cases.items():
        assert call() == E, name
        assert lib.mfhe_last_error(), name
    # a context without the phantom tables
    plain = mfhe.Context(list(mod), 4, 0)
    hp = plain.handle
    R = mfhe.ENOTREADY
    assert lib.mfhe_ntt_automorphism(hp, p0, L5, q0, L5, 1, 5, 3, None) == R
    assert lib.mfhe_ksk_inner_product_galois(hp, pr, L7, L7, pk, q0, 2 * L7, 1, 3, 5, 5, 5, 2, 3, None) == R
    assert lib.mfhe_keyswitch_raise(hp, p1, L5, pr, L7, L7, 1, 5, 2, 5, 2, None) == R
    assert lib.mfhe_galois_apply_raised(hp, p0, L5, pr, L7, L7, pk, q0, q1, L5, 1, 5, 5, 2, 5, 2, 3, None) == R
    assert lib.mfhe_galois_apply(hp, p0, p1, L5, pk, q0, q1, L5, 1, 5, 5, 2, 5, 2, 3, None) == R
    assert lib.mfhe_galois_reserve(hp, 1, 5, 5, 2, 5, 2) == R
    torch.cuda.synchronize()
    for name, b in bufs.items():   # nothing ran: every word is still the canary
        assert b.all_canary(), name
