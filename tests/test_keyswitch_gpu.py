"""GPU checks of hybrid key switching (csrc/keyswitch.hip; include/mfhe.h mfhe_ksk_assemble, mfhe_ksk_inner_product,
mfhe_keyswitch, mfhe_keyswitch_reserve and the Python layer's relinearize / gen_switch_key), bit-exact against Python
integers: the formulas computed here, the composition of the public pieces, and the coefficient-domain model of
tests/ks_model.py.  Every comparison is exact equality: the arithmetic is integer (ModDown's one f64 sum only selects
the multiple of P; tests/test_keyswitch_cpu.py shows the model's seeded inputs stay 2^-30 P away from where it could
flip, against the documented 2^-40 P)."""
import functools
import random

import numpy as np
import pytest

import ks_model as km
from primes import primes_of_size

pytestmark = pytest.mark.gpu

CANARY = 0xDEADBEEFCAFEF00D
CLASSES = pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
LOGNS = pytest.mark.parametrize("log_n", [4, 10])
# (name, poly pad, outer pad, base offset in words): even pads keep the 16-byte form, the odd pad and the one-word
# offset force the scalar variant
LAYOUTS = [("dense", 0, 0, 0), ("padded", 2, 4, 0), ("padded-odd", 3, 5, 0), ("misaligned", 0, 0, 1)]


def _u64(a):
    return np.array(a, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _moduli(log_n, bits):
    """5 Q primes and 2 special primes with q = 1 mod 2N."""
    m = primes_of_size(bits[0], 2 << log_n, 5) + primes_of_size(bits[1], 2 << log_n, 2)
    assert len(set(m)) == 7
    return tuple(m)


@functools.lru_cache(maxsize=None)
def _ctx(log_n, bits):
    import mfhe
    return mfhe.Context(list(_moduli(log_n, bits)), log_n, mfhe.CONV_PHANTOM)


def _row_limbs(level, special_start, nspecial):
    return list(range(level)) + list(range(special_start, special_start + nspecial))


def _random_rows(rng, lead, moduli, n):
    """Canonical residues [*lead][len(moduli)][n]; the first coefficient of the first block is 0 and its second, and
    the first of the last block, q - 1 on every row."""
    q = _u64(moduli)
    x = rng.integers(0, 2 ** 63, tuple(lead) + (len(moduli), n), dtype=np.uint64) % q[:, None]
    flat = x.reshape(-1, len(moduli), n)
    flat[0, :, 0] = 0
    flat[0, :, 1] = q - np.uint64(1)
    flat[-1, :, 0] = q - np.uint64(1)
    return x


class _Blocks:
    """A device allocation filled with a canary, holding blocks of `words` words at the given word offsets (from
    `base` words into the allocation); check_pads() asserts that every word outside the blocks is still the canary."""

    def __init__(self, mfhe, offsets, words, base=0, data=None):
        self.mfhe, self.offsets, self.words, self.base = mfhe, list(offsets), words, base
        host = np.full(base + max(self.offsets) + words + 2, CANARY, dtype=np.uint64)
        if data is not None:
            flat = np.ascontiguousarray(data).reshape(len(self.offsets), words)
            for o, d in zip(self.offsets, flat):
                host[base + o: base + o + words] = d
        self.full = mfhe.to_device_u64(host)
        self.t = self.full[base:]

    def blocks(self, shape):
        h = self.mfhe.to_host_u64(self.full)
        return np.stack([h[self.base + o: self.base + o + self.words] for o in self.offsets]).reshape(shape)

    def check_pads(self):
        h = self.mfhe.to_host_u64(self.full).copy()
        for o in self.offsets:
            h[self.base + o: self.base + o + self.words] = CANARY
        assert (h == np.uint64(CANARY)).all(), "words outside the output rows were written"

    def all_canary(self):
        return bool((self.mfhe.to_host_u64(self.full) == np.uint64(CANARY)).all())


def _polys(mfhe, npoly, rows, n, pad=0, base=0, data=None):
    """npoly blocks of rows * n words, rows * n + pad apart."""
    b = _Blocks(mfhe, [p * (rows * n + pad) for p in range(npoly)], rows * n, base, data)
    b.stride = rows * n + pad
    return b


def _inner_product_int(raised, ksk, moduli, level, key_level, special_start, nspecial):
    """acc [npoly][2][rows][N] (uint64) from raised [nd][npoly][rows][N] and ksk [nd][2][key_rows][N], in Python
    integers."""
    nd, npoly, rows, n = raised.shape
    limbs = _row_limbs(level, special_start, nspecial)
    out = np.zeros((npoly, 2, rows, n), dtype=np.uint64)
    for r, limb in enumerate(limbs):
        kr = r if r < level else key_level + r - level
        q = int(moduli[limb])
        x = raised[:, :, r, :].astype(object)                 # [nd][npoly][n]
        for c in range(2):
            k = ksk[:nd, c, kr, :].astype(object)             # [nd][n]
            out[:, c, r, :] = ((x * k[:, None, :]).sum(axis=0) % q).astype(np.uint64)
    return out


# ---------------------------------------------------------------------------------------------------------------
# key assembly
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_ksk_assemble_equals_the_formula(mfhe, log_n, bits):
    """Component 1 = a_j; component 0 = e_j - a_j s_to + F s_from with F = P mod q_r on the rows of digit j and 0
    elsewhere, the special rows included.  (5, 2): a partial last digit; (4, 3): the special limbs not adjacent to the
    key's Q limbs; (5, 1) with one special limb."""
    import torch
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(log_n)
    for key_level, alpha, sp, k in ((5, 2, 5, 2), (4, 3, 5, 2), (5, 1, 6, 1)):
        limbs = _row_limbs(key_level, sp, k)
        rmod = [mod[l] for l in limbs]
        rows, beta = key_level + k, -(-key_level // alpha)
        P = km.prod(mod[sp:sp + k])
        sf, st = _random_rows(rng, (1,), rmod, n)[0], _random_rows(rng, (1,), rmod, n)[0]
        a, e = _random_rows(rng, (beta,), rmod, n), _random_rows(rng, (beta,), rmod, n)
        out = _polys(mfhe, 1, beta * 2 * rows, n)
        ctx.ksk_assemble(mfhe.to_device_u64(sf.ravel()), mfhe.to_device_u64(st.ravel()), mfhe.to_device_u64(a.ravel()),
                         mfhe.to_device_u64(e.ravel()), out.t, key_level, alpha, sp, k)
        torch.cuda.synchronize()
        got = out.blocks((beta, 2, rows, n))
        out.check_pads()
        np.testing.assert_array_equal(got[:, 1], a, err_msg="component 1 is a copy of a")
        for j in range(beta):
            for r, q in enumerate(rmod):
                in_digit = r < key_level and r // alpha == j
                F = P % q if in_digit else 0
                want = (e[j, r].astype(object) - a[j, r].astype(object) * st[r].astype(object)
                        + F * sf[r].astype(object)) % q
                np.testing.assert_array_equal(got[j, 0, r], want.astype(np.uint64),
                                              err_msg=f"key_level {key_level} alpha {alpha} digit {j} row {r}")
                if r >= key_level:   # F = 0 on the special rows: s_from does not enter
                    plain = (e[j, r].astype(object) - a[j, r].astype(object) * st[r].astype(object)) % q
                    np.testing.assert_array_equal(got[j, 0, r], plain.astype(np.uint64))


# ---------------------------------------------------------------------------------------------------------------
# inner product
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_ksk_inner_product_bit_exact(mfhe, log_n, bits):
    import torch
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(10 + log_n)
    key_level, sp, k = 5, 5, 2
    for level in (5, 3):
        rows = level + k
        rmod = [mod[l] for l in _row_limbs(level, sp, k)]
        kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
        raised = _random_rows(rng, (6, 6), rmod, n)            # [nd][npoly][rows][n]
        ksk = _random_rows(rng, (6, 2), kmod, n)               # [nd][2][key_rows][n]
        d_ksk = mfhe.to_device_u64(ksk.ravel())
        # every layout at 1 and 3 digits and 1 and 3 polynomials; every other digit count with its own kernel
        # instantiation (2, 4, 5, 6), and 6 polynomials (a thread's run of 4 and a tail of 2), dense and misaligned
        for nd in (1, 2, 3, 4, 5, 6):
            want = _inner_product_int(raised[:nd], ksk, mod, level, key_level, sp, k)
            for npoly in (1, 3, 6):
                full = nd in (1, 3) and npoly in (1, 3)
                for name, ppad, dpad, off in (LAYOUTS if full else (LAYOUTS[0], LAYOUTS[3])):
                    pst = rows * n + ppad
                    dst = npoly * pst + dpad
                    src = np.ascontiguousarray(raised[:nd, :npoly])
                    bi = _Blocks(mfhe, [j * dst + p * pst for j in range(nd) for p in range(npoly)], rows * n, off, src)
                    bo = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
                    ctx.ksk_inner_product(bi.t, d_ksk, bo.t, npoly, nd, level, key_level, sp, k, digit_stride=dst,
                                          poly_stride=pst, acc_stride=bo.stride)
                    torch.cuda.synchronize()
                    msg = f"{name} level {level} nd {nd} npoly {npoly}"
                    np.testing.assert_array_equal(bo.blocks((npoly, 2, rows, n)), want[:npoly], err_msg=msg)
                    bo.check_pads()
                    np.testing.assert_array_equal(bi.blocks((nd, npoly, rows, n)), src, err_msg=msg)   # untouched
                    bi.check_pads()
        np.testing.assert_array_equal(mfhe.to_host_u64(d_ksk), ksk.ravel())


def test_ksk_inner_product_18_digits_of_62_bit_operands(mfhe):
    """Every operand q - 1 with 62-bit primes: each product is just below 2^124 and 18 of them overflow a u128, so the
    sum is only right if it is reduced after 16 terms.  18 (q - 1)^2 = 18 mod q."""
    import torch
    mod = primes_of_size(62, 32, 3)
    assert len(mod) == 3 and all(m < 2 ** 62 for m in mod)
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    n, nd, level, k = 16, 18, 2, 1
    rows = level + k
    top = _u64(mod) - np.uint64(1)
    raised = np.broadcast_to(top[None, None, :, None], (nd, 3, rows, n)).copy()
    ksk = np.broadcast_to(top[None, None, :, None], (nd, 2, rows, n)).copy()
    want = _inner_product_int(raised, ksk, mod, level, level, level, k)
    assert (want == np.uint64(18)).all()
    d_ksk = mfhe.to_device_u64(ksk.ravel())
    for npoly in (1, 3):
        for name, ppad, dpad, off in LAYOUTS:
            pst = rows * n + ppad
            dst = npoly * pst + dpad
            src = np.ascontiguousarray(raised[:, :npoly])
            bi = _Blocks(mfhe, [j * dst + p * pst for j in range(nd) for p in range(npoly)], rows * n, off, src)
            bo = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
            ctx.ksk_inner_product(bi.t, d_ksk, bo.t, npoly, nd, level, level, level, k, digit_stride=dst,
                                  poly_stride=pst, acc_stride=bo.stride)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bo.blocks((npoly, 2, rows, n)), want[:npoly], err_msg=f"{name} {npoly}")
            bo.check_pads()
            np.testing.assert_array_equal(bi.blocks((nd, npoly, rows, n)), src)


# ---------------------------------------------------------------------------------------------------------------
# the driver against the composition of the public pieces
# ---------------------------------------------------------------------------------------------------------------
def _composition(mfhe, ctx, mod, x, ksk, npoly, level, key_level, alpha, sp, k, addend=None):
    """ntt_modup per digit -> the Python inner product -> ntt_moddown per component (+ addend mod q):
    (out0, out1), each [npoly][level][N] uint64."""
    import torch
    n, rows = ctx.N, level + k
    d_in = mfhe.to_device_u64(x.ravel())
    raised = []
    for ds, dc in km.digits(level, alpha):
        up = torch.zeros(npoly * rows * n, dtype=torch.int64, device="cuda")
        ctx.ntt_modup(d_in, up, npoly, level, ds, dc, sp, k)
        torch.cuda.synchronize()
        raised.append(mfhe.to_host_u64(up).reshape(npoly, rows, n).copy())
    acc = _inner_product_int(np.stack(raised), ksk, mod, level, key_level, sp, k)
    outs = []
    for c in range(2):
        d_acc = mfhe.to_device_u64(np.ascontiguousarray(acc[:, c]).ravel())
        down = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
        ctx.ntt_moddown(d_acc, down, npoly, level, sp, k)
        torch.cuda.synchronize()
        o = mfhe.to_host_u64(down).reshape(npoly, level, n).copy()
        if addend is not None:
            q = _u64(mod[:level])[None, :, None]
            o = ((o.astype(object) + addend[c].astype(object)) % q.astype(object)).astype(np.uint64)
        outs.append(o)
    return outs


# (key_level, alpha, special_start, nspecial, levels): alpha 2 with a partial last digit at levels 5 and 3 and a single
# digit at level 2; alpha 1 with one special limb (not adjacent to the Q limbs); alpha = level, one digit
KS_CASES = [(5, 2, 5, 2, (5, 3, 2)), (5, 1, 6, 1, (5,)), (5, 5, 5, 2, (5,))]


@CLASSES
@LOGNS
def test_keyswitch_equals_the_composition(mfhe, log_n, bits):
    import torch
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(20 + log_n)
    npoly = 2
    for key_level, alpha, sp, k, levels in KS_CASES:
        kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
        beta_key = -(-key_level // alpha)
        ksk = _random_rows(rng, (beta_key, 2), kmod, n)
        d_ksk = mfhe.to_device_u64(ksk.ravel())
        for level in levels:
            x = _random_rows(rng, (npoly,), mod[:level], n)
            old = [_random_rows(rng, (npoly,), mod[:level], n) for _ in range(2)]
            for flags, ipad, opad in ((0, 2, 4), (mfhe.KS_ADD, 0, 0), (mfhe.KS_ADD, 3, 5)):
                want = _composition(mfhe, ctx, mod, x, ksk, npoly, level, key_level, alpha, sp, k,
                                    old if flags else None)
                bi = _polys(mfhe, npoly, level, n, ipad, 0, x)
                b0 = _polys(mfhe, npoly, level, n, opad, 0, old[0])
                b1 = _polys(mfhe, npoly, level, n, opad, 0, old[1])
                ctx.keyswitch(bi.t, d_ksk, b0.t, b1.t, npoly, level, key_level, alpha, sp, k, flags,
                              in_stride=bi.stride, out_stride=b0.stride)
                torch.cuda.synchronize()
                msg = f"alpha {alpha} K {k} level {level} flags {flags} pads {ipad}, {opad}"
                np.testing.assert_array_equal(b0.blocks((npoly, level, n)), want[0], err_msg="out0 " + msg)
                np.testing.assert_array_equal(b1.blocks((npoly, level, n)), want[1], err_msg="out1 " + msg)
                b0.check_pads()
                b1.check_pads()
                np.testing.assert_array_equal(bi.blocks((npoly, level, n)), x, err_msg="input " + msg)
                bi.check_pads()
        np.testing.assert_array_equal(mfhe.to_host_u64(d_ksk), ksk.ravel())


# ---------------------------------------------------------------------------------------------------------------
# the driver against the coefficient-domain model
# ---------------------------------------------------------------------------------------------------------------
def _residues(polys, moduli):
    """[len(polys)][len(moduli)][N] uint64 residues of integer polynomials (negative coefficients allowed)."""
    return _u64([[[int(v) % int(m) for v in poly] for m in moduli] for poly in polys])


def _device_key(mfhe, ctx, cs):
    """The model case's switching key assembled on the device from residues sent through ntt_fwd."""
    mod = cs["q"] + cs["p"]
    beta = len(cs["a"])
    ev = {}
    for name, polys in (("s_from", [cs["s_from"]]), ("s_to", [cs["s_to"]]), ("a", cs["a"]), ("e", cs["e"])):
        ev[name] = ctx.ntt_fwd(mfhe.to_device_u64(_residues(polys, mod).ravel()), len(polys), 0, 7)
    import torch
    ksk = torch.zeros(beta * 2 * 7 * cs["n"], dtype=torch.int64, device="cuda")
    return ctx.ksk_assemble(ev["s_from"], ev["s_to"], ev["a"], ev["e"], ksk, 5, cs["alpha"], 5, 2)


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("kind", ["switch", "relin"])
def test_keyswitch_equals_the_model(mfhe, bits, kind):
    """N = 16, the seeded inputs of tests/test_keyswitch_cpu.py: the key assembled and switched on the device, back
    through ntt_inv, equals the model's key, k_0 and k_1 on every limb."""
    import torch
    cs = km.seeded_case(bits, kind, True)
    q, p, n = cs["q"], cs["p"], cs["n"]
    mod = q + p
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    ksk = _device_key(mfhe, ctx, cs)
    coef = ctx.ntt_inv(ksk.clone(), 6, 0, 7)
    torch.cuda.synchronize()
    want_key = _residues([comp for kj in cs["key"] for comp in kj], mod)
    np.testing.assert_array_equal(mfhe.to_host_u64(coef).reshape(6, 7, n), want_key)
    for level in km.CASE_LEVELS:
        k0, k1, margin = km.keyswitch(q, p, cs["alpha"], level, cs["c"][level], cs["key"])
        assert margin >= 2.0 ** -30
        d_in = ctx.ntt_fwd(mfhe.to_device_u64(_residues([cs["c"][level]], q[:level]).ravel()), 1, 0, level)
        o0 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        o1 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        ctx.keyswitch(d_in, ksk, o0, o1, 1, level, 5, cs["alpha"], 5, 2)
        ctx.ntt_inv(o0, 1, 0, level)
        ctx.ntt_inv(o1, 1, 0, level)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(o0).reshape(1, level, n), _residues([k0], q[:level]),
                                      err_msg=f"k0 level {level}")
        np.testing.assert_array_equal(mfhe.to_host_u64(o1).reshape(1, level, n), _residues([k1], q[:level]),
                                      err_msg=f"k1 level {level}")


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
def test_relinearize_a_product(mfhe, bits):
    """Two ciphertexts (b, a) with b = m - a s, as evaluation-domain pairs; their tensor product (d0, d1, d2) is made
    from those pairs limb by limb; relinearize(d2 -> d0, d1) equals the composition of the public pieces, equals the
    model's (d0 + k_0, d1 + k_1), and that value decrypts to the product within the CPU test's bound."""
    import torch
    cs = km.seeded_case(bits, "relin", True)
    q, p, n, alpha, s = cs["q"], cs["p"], cs["n"], cs["alpha"], cs["s_to"]
    mod = q + p
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    ksk = _device_key(mfhe, ctx, cs)
    ksk_host = mfhe.to_host_u64(ksk).reshape(3, 2, 7, n).copy()
    rnd = random.Random(f"relin-{bits}")
    for level in km.CASE_LEVELS:
        Ql = km.prod(q[:level])
        cts = []
        for _ in range(2):
            a = [rnd.randrange(Ql) for _ in range(n)]
            m = [rnd.randint(-1000, 1000) for _ in range(n)]
            b = [(mv - v) % Ql for mv, v in zip(m, km.negacyclic(a, s, Ql))]
            cts.append((b, a))
        flat = [cts[0][0], cts[0][1], cts[1][0], cts[1][1]]
        ev = mfhe.to_host_u64(ctx.ntt_fwd(mfhe.to_device_u64(_residues(flat, q[:level]).ravel()), 4, 0, level))
        torch.cuda.synchronize()
        b1, a1, b2, a2 = (ev.reshape(4, level, n)[i].astype(object) for i in range(4))
        qo = np.array(q[:level], dtype=object)[:, None]
        d0, d1, d2 = ((b1 * b2) % qo).astype(np.uint64), ((b1 * a2 + a1 * b2) % qo).astype(np.uint64), \
            ((a1 * a2) % qo).astype(np.uint64)
        want = _composition(mfhe, ctx, mod, d2[None], ksk_host, 1, level, 5, alpha, 5, 2, [d0[None], d1[None]])
        t0, t1, t2 = (mfhe.to_device_u64(d.ravel()) for d in (d0, d1, d2))
        ctx.relinearize(t2, ksk, t0, t1, 1, level, 5, alpha, 5, 2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(t0).reshape(1, level, n), want[0], err_msg=f"level {level}")
        np.testing.assert_array_equal(mfhe.to_host_u64(t1).reshape(1, level, n), want[1], err_msg=f"level {level}")
        np.testing.assert_array_equal(mfhe.to_host_u64(t2).reshape(level, n), d2)
        # the model: d2 = a1 a2 in the coefficient domain, switched from s^2 to s
        d0c = km.negacyclic(cts[0][0], cts[1][0], Ql)
        d1c = [(x + y) % Ql for x, y in zip(km.negacyclic(cts[0][0], cts[1][1], Ql),
                                            km.negacyclic(cts[0][1], cts[1][0], Ql))]
        d2c = km.negacyclic(cts[0][1], cts[1][1], Ql)
        k0, k1, margin = km.keyswitch(q, p, alpha, level, d2c, cs["key"])
        assert margin >= 2.0 ** -30, "pick another seed: a ModDown remainder sits at +-P/2"
        ctx.ntt_inv(t0, 1, 0, level)
        ctx.ntt_inv(t1, 1, 0, level)
        torch.cuda.synchronize()
        r0 = [(x + y) % Ql for x, y in zip(d0c, k0)]
        r1 = [(x + y) % Ql for x, y in zip(d1c, k1)]
        np.testing.assert_array_equal(mfhe.to_host_u64(t0).reshape(1, level, n), _residues([r0], q[:level]))
        np.testing.assert_array_equal(mfhe.to_host_u64(t1).reshape(1, level, n), _residues([r1], q[:level]))
        err = km.decryption_error(q, level, k0, k1, d2c, cs["s_from"], s)
        bound = km.error_bound(q, p, alpha, level, n, km.B_E)
        print(f"relinearize bits {bits} level {level}: error {err}, bound {bound:.2f}")
        assert err <= bound
        # and so the relinearised pair decrypts to the degree-2 decryption d0 + d1 s + d2 s^2 within that bound
        deg2 = [(x + y + z) % Ql for x, y, z in zip(d0c, km.negacyclic(d1c, s, Ql),
                                                    km.negacyclic(d2c, cs["s_from"], Ql))]
        deg1 = [(x + y) % Ql for x, y in zip(r0, km.negacyclic(r1, s, Ql))]
        assert max(abs(km.centered(x - y, Ql)) for x, y in zip(deg1, deg2)) <= bound


# ---------------------------------------------------------------------------------------------------------------
# gen_switch_key
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_gen_switch_key_is_deterministic_and_its_noise_small(mfhe, log_n, bits):
    import torch
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    key_level, alpha, sp, k, sigma = 5, 2, 5, 2, 3.2
    rnd = random.Random(log_n)
    s_from = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    s_to = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    sf = ctx.ntt_fwd(mfhe.to_device_u64(_residues([s_from], mod).ravel()), 1, 0, 7)
    st = ctx.ntt_fwd(mfhe.to_device_u64(_residues([s_to], mod).ravel()), 1, 0, 7)
    keys = []
    for _ in range(2):
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        keys.append(mfhe.to_host_u64(ctx.gen_switch_key(sf, st, key_level, alpha, sp, k, generator=g, sigma=sigma)).copy())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(keys[0], keys[1], err_msg="same seed, same key")
    g = torch.Generator(device="cuda")
    g.manual_seed(8)
    other = mfhe.to_host_u64(ctx.gen_switch_key(sf, st, key_level, alpha, sp, k, generator=g, sigma=sigma))
    assert (other != keys[0]).any()
    beta = 3
    key = keys[0].reshape(beta, 2, 7, n)
    qcol = _u64(mod)[None, :, None]
    assert (key[:, 1] < qcol).all() and (key[:, 0] < qcol).all(), "canonical"
    # e_j = ntt_inv(b_j + a_j s_to - F s_from), composed over all 7 limbs
    sfh, sth = mfhe.to_host_u64(sf).reshape(7, n).astype(object), mfhe.to_host_u64(st).reshape(7, n).astype(object)
    P = km.prod(mod[5:7])
    noise = np.zeros((beta, 7, n), dtype=np.uint64)
    for j in range(beta):
        for r, q in enumerate(mod):
            F = P % q if (r < key_level and r // alpha == j) else 0
            noise[j, r] = ((key[j, 0, r].astype(object) + key[j, 1, r].astype(object) * sth[r] - F * sfh[r]) % q
                           ).astype(np.uint64)
    coef = mfhe.to_host_u64(ctx.ntt_inv(mfhe.to_device_u64(noise.ravel()), beta, 0, 7)).reshape(beta, 7, n)
    torch.cuda.synchronize()
    M = km.prod(mod)
    lift = [(M // m) * pow(M // m, -1, m) for m in mod]
    worst = 0
    for j in range(beta):
        tot = sum(coef[j, r].astype(object) * lift[r] for r in range(7)) % M
        worst = max(worst, max(abs(km.centered(int(v), M)) for v in tot))
    print(f"gen_switch_key log_n {log_n}: largest |e| = {worst}")
    assert worst <= 6 * sigma + 1
    assert worst > 0, "the key carries noise"


# ---------------------------------------------------------------------------------------------------------------
# graph capture, argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After keyswitch_reserve the driver allocates nothing and copies nothing to the device: it is captured into a
    graph (a hipMalloc or a synchronous hipMemcpy would fail the capture), replayed twice, and both replays equal the
    eager result."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, n = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    npoly, level, key_level, alpha, sp, k = 2, 5, 5, 2, 5, 2
    ctx.keyswitch_reserve(npoly, level, key_level, alpha, sp, k)
    rng = np.random.default_rng(3)
    x = _random_rows(rng, (npoly,), mod[:level], n)
    ksk = _random_rows(rng, (3, 2), mod, n)
    d_in, d_ksk = mfhe.to_device_u64(x.ravel()), mfhe.to_device_u64(ksk.ravel())
    o0 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.keyswitch(d_in, d_ksk, o0, o1, npoly, level, key_level, alpha, sp, k)
    outs = []
    for _ in range(2):
        o0.zero_()
        o1.zero_()
        g.replay()
        torch.cuda.synchronize()
        outs.append((mfhe.to_host_u64(o0).copy(), mfhe.to_host_u64(o1).copy()))
    e0 = torch.zeros_like(o0)
    e1 = torch.zeros_like(o1)
    ctx.keyswitch(d_in, d_ksk, e0, e1, npoly, level, key_level, alpha, sp, k)
    torch.cuda.synchronize()
    for got in outs:
        np.testing.assert_array_equal(got[0], mfhe.to_host_u64(e0))
        np.testing.assert_array_equal(got[1], mfhe.to_host_u64(e1))
    assert outs[0][0].any() and outs[0][1].any()


def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    mod, N = _moduli(4, (45, 49)), 16
    ctx = mfhe.Context(list(mod), 4, mfhe.CONV_PHANTOM)
    h = ctx.handle
    bufs = {name: _polys(mfhe, 1, 3 * 2 * 7, N) for name in ("in", "ksk", "o0", "o1", "aux")}
    pi, pk, p0, p1, px = (bufs[name].t.data_ptr() for name in ("in", "ksk", "o0", "o1", "aux"))
    E = mfhe.EINVAL
    L5, L7 = 5 * N, 7 * N

    def ks(i=pi, ist=L5, key=pk, o0=p0, o1=p1, ost=L5, npoly=1, level=5, kl=5, alpha=2, sp=5, k=2, flags=0):
        return lib.mfhe_keyswitch(h, i, ist, key, o0, o1, ost, npoly, level, kl, alpha, sp, k, flags, None)

    def ip(r=pi, dst=L7, pst=L7, key=pk, acc=p0, ast=2 * L7, npoly=1, nd=3, level=5, kl=5, sp=5, k=2):
        return lib.mfhe_ksk_inner_product(h, r, dst, pst, key, acc, ast, npoly, nd, level, kl, sp, k, None)

    def asm(sf=pi, st=px, a=p0, e=p1, key=pk, kl=5, alpha=2, sp=5, k=2):
        return lib.mfhe_ksk_assemble(h, sf, st, a, e, key, kl, alpha, sp, k, None)

    cases = {
        "keyswitch null in": lambda: ks(i=None),
        "keyswitch null key": lambda: ks(key=None),
        "keyswitch null out0": lambda: ks(o0=None),
        "keyswitch null out1": lambda: ks(o1=None),
        "keyswitch alpha < 1": lambda: ks(alpha=0),
        "keyswitch nspecial < 1": lambda: ks(k=0),
        "keyswitch level > key_level": lambda: ks(level=5, kl=4),
        "keyswitch level < 1": lambda: ks(level=0),
        "keyswitch special overlaps Q": lambda: ks(sp=4),
        "keyswitch special outside": lambda: ks(sp=6),
        "keyswitch special negative": lambda: ks(kl=4, level=4, sp=-1),
        "keyswitch in stride": lambda: ks(ist=L5 - 1, npoly=2),
        "keyswitch out stride": lambda: ks(ost=L5 - 1, npoly=2),
        "keyswitch in is out0": lambda: ks(o0=pi),
        "keyswitch in is out1": lambda: ks(o1=pi),
        "keyswitch in overlaps out1": lambda: ks(o1=pi + 8 * N),
        "keyswitch flags": lambda: ks(flags=2),
        "inner product null raised": lambda: ip(r=None),
        "inner product null key": lambda: ip(key=None),
        "inner product null acc": lambda: ip(acc=None),
        "inner product ndigits < 1": lambda: ip(nd=0),
        "inner product nspecial < 1": lambda: ip(k=0),
        "inner product level > key_level": lambda: ip(kl=4),
        "inner product special overlaps Q": lambda: ip(sp=4),
        "inner product special outside": lambda: ip(sp=6),
        "inner product poly stride": lambda: ip(pst=L7 - 1),
        "inner product acc stride": lambda: ip(ast=2 * L7 - 1),
        "inner product digit stride": lambda: ip(dst=L7 - 1),
        "assemble null s_from": lambda: asm(sf=None),
        "assemble null s_to": lambda: asm(st=None),
        "assemble null a": lambda: asm(a=None),
        "assemble null e": lambda: asm(e=None),
        "assemble null ksk": lambda: asm(key=None),
        "assemble alpha < 1": lambda: asm(alpha=0),
        "assemble nspecial < 1": lambda: asm(k=0),
        "assemble key_level outside": lambda: asm(kl=8),
        "assemble special overlaps Q": lambda: asm(sp=4),
        "assemble special outside": lambda: asm(sp=6),
        "reserve alpha < 1": lambda: lib.mfhe_keyswitch_reserve(h, 1, 5, 5, 0, 5, 2),
        "reserve nspecial < 1": lambda: lib.mfhe_keyswitch_reserve(h, 1, 5, 5, 2, 5, 0),
        "reserve level > key_level": lambda: lib.mfhe_keyswitch_reserve(h, 1, 5, 4, 2, 5, 2),
        "reserve special outside": lambda: lib.mfhe_keyswitch_reserve(h, 1, 5, 5, 2, 6, 2),
    }
    for name, call in cases.items():
        assert call() == E, name
        assert lib.mfhe_last_error(), name
    # a context without the phantom tables
    plain = mfhe.Context(list(mod), 4, 0)
    hp = plain.handle
    R = mfhe.ENOTREADY
    assert lib.mfhe_keyswitch(hp, pi, L5, pk, p0, p1, L5, 1, 5, 5, 2, 5, 2, 0, None) == R
    assert lib.mfhe_ksk_inner_product(hp, pi, L7, L7, pk, p0, 2 * L7, 1, 3, 5, 5, 5, 2, None) == R
    assert lib.mfhe_ksk_assemble(hp, pi, px, p0, p1, pk, 5, 2, 5, 2, None) == R
    assert lib.mfhe_keyswitch_reserve(hp, 1, 5, 5, 2, 5, 2) == R
    torch.cuda.synchronize()
    for name, b in bufs.items():   # nothing ran: every word is still the canary
        assert b.all_canary(), name
