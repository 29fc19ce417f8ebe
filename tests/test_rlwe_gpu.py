"""GPU checks of the RLWE client side (csrc/rlwe.hip; include/mfhe.h mfhe_rlwe_*): the samplers bit for bit against
tests/rlwe_model.py, every fused call against its definition through the public calls and Python integers, the noise
of a public-key encryption and of a generated switching key under their bounds, graph capture after the reserve call,
argument errors, and one computation end to end -- keys, encode, encrypt, polynomial, decrypt, decode -- with no host
arithmetic between the encoder and the decoder.  Everything here runs at N <= 2^10 on at most 3 polynomials;
tests/test_client_shapes_gpu.py reaches the launch shapes beyond that: more than one workgroup per row, more than one
run of polynomials, the small kernel's fold over grid y and z, and N = 2^14 and 2^16 where the NTT plan changes."""
import ctypes
import functools

import numpy as np
import pytest

import galois_model as gm
import ks_model as km
import poly_model as pm
import rlwe_model as rm
import test_poly_gpu as tpg
import test_slot_gpu as tsg
from test_keyswitch_gpu import CLASSES, LAYOUTS, LOGNS, _polys, _random_rows, _u64
from test_poly_gpu import NQ, NSP, _ctx, _moduli

pytestmark = pytest.mark.gpu

KEY = bytes((37 * i + 11) & 0xFF for i in range(32))
KW = rm.seed_words(KEY)
FIRST_ID = (1 << 32) - 2            # a batch of three crosses the id's word boundary
SP = NQ                             # the special limbs are limbs 8 and 9
GEOMS = [(1, 0), (1, 2), (5, 0), (5, 2)]   # (level, special rows)
B_NOISE = rm.NOISE_BITS             # |e| <= 21
LAYOUT = pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])


def _limbs(level, k):
    return rm.row_limbs(level, SP, k)


@functools.lru_cache(maxsize=None)
def _small_ints(stream, pid, n):
    return rm.small_values(KW, stream, pid % (1 << 64), n)


def _small_model(stream, first_id, npoly, limbs, mod, n):
    vals = np.stack([_small_ints(stream, first_id + p, n) for p in range(npoly)])
    return rm.small_rows(vals, limbs, mod), vals


@functools.lru_cache(maxsize=None)
def _mask_row(limb, pid, n, q):
    return rm.mask_residues(KW, limb, pid % (1 << 64), n, q)


def _uniform_model(first_id, npoly, limbs, mod, n):
    return np.stack([np.stack([_mask_row(l, first_id + p, n, int(mod[l])) for l in limbs]) for p in range(npoly)])


def _ntt_rows(mfhe, ctx, x, level, k):
    """The forward transform of coefficient rows x [npoly][level + k][n] (uint64), through mfhe_ntt_fwd on dense blocks."""
    npoly, rows, n = x.shape
    out = np.empty_like(x)
    dq = ctx.ntt_fwd(mfhe.to_device_u64(np.ascontiguousarray(x[:, :level]).ravel()), npoly, 0, level)
    out[:, :level] = mfhe.to_host_u64(dq).reshape(npoly, level, n)
    if k:
        dp = ctx.ntt_fwd(mfhe.to_device_u64(np.ascontiguousarray(x[:, level:]).ravel()), npoly, SP, k)
        out[:, level:] = mfhe.to_host_u64(dp).reshape(npoly, k, n)
    return out


def _intt_rows(mfhe, ctx, x, level):
    npoly, rows, n = x.shape
    d = ctx.ntt_inv(mfhe.to_device_u64(np.ascontiguousarray(x[:, :level]).ravel()), npoly, 0, level)
    return mfhe.to_host_u64(d).reshape(npoly, level, n)


def _mulmod(a, b, limbs, mod):
    """a b mod q_row on [..][rows][n] arrays, in Python integers."""
    qo = np.array([int(mod[l]) for l in limbs], dtype=object)[:, None]
    return (a.astype(object) * b.astype(object)) % qo


def _qcol(limbs, mod):
    return np.array([int(mod[l]) for l in limbs], dtype=object)[:, None]


def _dev(mfhe, a):
    return mfhe.to_device_u64(np.ascontiguousarray(a).ravel())


def _secret(mfhe, ctx, pid, level, k, n, sp=SP):
    """(device tensor, host rows) of the ternary secret of id `pid` at level + k rows, evaluation domain."""
    import torch
    t = torch.zeros((level + k) * n, dtype=torch.int64, device="cuda")
    ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, pid, t, 1, level, sp, k)
    torch.cuda.synchronize()
    return t, mfhe.to_host_u64(t).reshape(level + k, n).copy()


# ---------------------------------------------------------------------------------------------------------------
# 1. the samplers against the model
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
@LAYOUT
def test_sample_uniform_equals_the_model(mfhe, log_n, bits, layout):
    import torch
    _, ppad, _, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    for npoly in (1, 3):
        for level, k in GEOMS:
            limbs = _limbs(level, k)
            out = _polys(mfhe, npoly, level + k, n, ppad, base)
            ctx.rlwe_sample_uniform(KEY, FIRST_ID, out.t, npoly, level, SP, k, out_stride=out.stride)
            torch.cuda.synchronize()
            want = _uniform_model(FIRST_ID, npoly, limbs, mod, n)
            np.testing.assert_array_equal(out.blocks((npoly, level + k, n)), want, err_msg=f"{npoly} {level} {k}")
            out.check_pads()
    # the last id of the 64-bit space, and the id wrapping past it
    out = _polys(mfhe, 2, 1, n, ppad, base)
    ctx.rlwe_sample_uniform(KEY, (1 << 64) - 1, out.t, 2, 1, 0, 0, out_stride=out.stride)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.blocks((2, 1, n)), _uniform_model((1 << 64) - 1, 2, [0], mod, n))


@CLASSES
@LOGNS
@LAYOUT
def test_sample_small_equals_the_model(mfhe, log_n, bits, layout):
    """Every stream, in the coefficient domain against the model (v or q + v on every row) and transformed against
    mfhe_ntt_fwd of the coefficient form."""
    import torch
    _, ppad, _, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    for stream in rm.SMALL_STREAMS:
        for npoly in (1, 3):
            for level, k in GEOMS:
                limbs = _limbs(level, k)
                want, vals = _small_model(stream, FIRST_ID, npoly, limbs, mod, n)
                lim = 1 if stream in rm.TERNARY_STREAMS else B_NOISE
                assert np.abs(vals).max() <= lim
                for flags, w in ((mfhe.RLWE_COEFF, want), (0, None)):
                    out = _polys(mfhe, npoly, level + k, n, ppad, base)
                    ctx.rlwe_sample_small(KEY, stream, FIRST_ID, out.t, npoly, level, SP, k, flags,
                                          out_stride=out.stride)
                    torch.cuda.synchronize()
                    if w is None:
                        w = _ntt_rows(mfhe, ctx, want, level, k)
                    np.testing.assert_array_equal(out.blocks((npoly, level + k, n)), w,
                                                  err_msg=f"stream {stream} npoly {npoly} level {level} K {k} flags {flags}")
                    out.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 2. the same tail fed from memory
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
@LAYOUT
def test_lift_small_of_the_sampled_integers_gives_the_same_rows(mfhe, log_n, bits, layout):
    import torch
    _, ppad, _, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    npoly, cst = 3, n + 3
    for stream, (level, k) in ((rm.SECRET, (5, 2)), (rm.NOISE, (1, 0)), (rm.NOISE1, (5, 0))):
        _, vals = _small_model(stream, FIRST_ID, npoly, _limbs(level, k), mod, n)
        host = np.full(npoly * cst, 12345, dtype=np.int32)
        for p in range(npoly):
            host[p * cst:p * cst + n] = vals[p]
        coeffs = torch.from_numpy(host).cuda()
        for flags in (mfhe.RLWE_COEFF, 0):
            want = _polys(mfhe, npoly, level + k, n)
            ctx.rlwe_sample_small(KEY, stream, FIRST_ID, want.t, npoly, level, SP, k, flags)
            out = _polys(mfhe, npoly, level + k, n, ppad, base)
            ctx.rlwe_lift_small(coeffs, out.t, npoly, level, SP, k, flags, coeff_stride=cst, out_stride=out.stride)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.blocks((npoly, level + k, n)), want.blocks((npoly, level + k, n)))
            out.check_pads()
    # any int32, the extremes among them: v mod q on every row
    rng = np.random.default_rng(log_n)
    v = rng.integers(-(1 << 31), 1 << 31, (2, n), dtype=np.int64)
    v[0, :4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    out = _polys(mfhe, 2, 7, n, ppad, base)
    ctx.rlwe_lift_small(torch.from_numpy(v.astype(np.int32).ravel()).cuda(), out.t, 2, 5, SP, 2, mfhe.RLWE_COEFF,
                        out_stride=out.stride)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.blocks((2, 7, n)), rm.small_rows(v, _limbs(5, 2), mod))
    out.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# 3. symmetric encryption
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
@LAYOUT
def test_encrypt_sk_is_its_definition(mfhe, log_n, bits, layout):
    """c1 == sample_uniform and c0 == m + sample_small(NOISE) - c1 s in Python integers, with a message and without."""
    import torch
    _, ppad, _, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(log_n + 100)
    for npoly in (1, 3):
        for level, k in ((1, 0), (5, 2)):
            limbs, rows = _limbs(level, k), level + k
            s_dev, s = _secret(mfhe, ctx, 7, level, k, n)
            e = _polys(mfhe, npoly, rows, n)
            ctx.rlwe_sample_small(KEY, mfhe.RLWE_NOISE, FIRST_ID, e.t, npoly, level, SP, k)
            torch.cuda.synchronize()
            e = e.blocks((npoly, rows, n))
            a = _uniform_model(FIRST_ID, npoly, limbs, mod, n)
            a_s = _mulmod(a, s[None], limbs, mod)
            m = _random_rows(rng, (npoly,), [mod[l] for l in limbs], n)
            for msg in (m, None):
                mb = _polys(mfhe, npoly, rows, n, ppad + 2, 0, msg) if msg is not None else None
                c0 = _polys(mfhe, npoly, rows, n, ppad, base)
                c1 = _polys(mfhe, npoly, rows, n, ppad, base)
                ctx.rlwe_encrypt_sk(KEY, FIRST_ID, s_dev, mb.t if mb else None, c0.t, c1.t, npoly, level, SP, k,
                                    m_stride=mb.stride if mb else None, out_stride=c0.stride)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(c1.blocks((npoly, rows, n)), a, err_msg="c1 is the mask")
                add = msg.astype(object) if msg is not None else 0
                want = ((add + e.astype(object) - a_s) % _qcol(limbs, mod)).astype(np.uint64)
                np.testing.assert_array_equal(c0.blocks((npoly, rows, n)), want,
                                              err_msg=f"c0 npoly {npoly} level {level} K {k} m {msg is not None}")
                c0.check_pads()
                c1.check_pads()
                if mb:
                    np.testing.assert_array_equal(mb.blocks((npoly, rows, n)), msg)


# ---------------------------------------------------------------------------------------------------------------
# 4. switching, relinearisation and Galois keys
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
def test_ksk_gen_equals_ksk_assemble_fed_the_samplers(mfhe, log_n, bits):
    """All three kinds at (key_level, alpha, special range) = (5, 2, [8, 10)) with a partial last digit, (4, 3, [8, 10))
    with the special limbs not adjacent to the key's, (8, 1, [9, 10)) with one special limb: bit for bit
    mfhe_ksk_assemble of sample_uniform, sample_small(NOISE) and an s_from made outside (s^2 from Python integers,
    sigma_g(s) from mfhe_ntt_automorphism)."""
    import torch
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    g = gm.galois_elt(3, log_n)
    for key_level, alpha, sp, k in ((5, 2, 8, 2), (4, 3, 8, 2), (8, 1, 9, 1)):
        limbs = rm.row_limbs(key_level, sp, k)
        rows, beta = key_level + k, -(-key_level // alpha)
        first = FIRST_ID + key_level
        zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
        s_to, s_other = zeros(rows * n), zeros(rows * n)
        ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, 1, s_to, 1, key_level, sp, k)
        ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, 2, s_other, 1, key_level, sp, k)
        a, e = zeros(beta * rows * n), zeros(beta * rows * n)
        ctx.rlwe_sample_uniform(KEY, first, a, beta, key_level, sp, k)
        ctx.rlwe_sample_small(KEY, mfhe.RLWE_NOISE, first, e, beta, key_level, sp, k)
        torch.cuda.synchronize()
        sh = mfhe.to_host_u64(s_to).reshape(rows, n)
        s2 = _dev(mfhe, _mulmod(sh, sh, limbs, mod).astype(np.uint64))
        sg = ctx.automorphism(s_to, zeros(rows * n), 1, rows, g)
        for kind, s_from, arg in ((mfhe.RLWE_KEY_SWITCH, s_other, s_other), (mfhe.RLWE_KEY_RELIN, s2, None),
                                  (mfhe.RLWE_KEY_GALOIS, sg, None)):
            want = ctx.ksk_assemble(s_from, s_to, a, e, zeros(beta * 2 * rows * n), key_level, alpha, sp, k)
            out = _polys(mfhe, 1, beta * 2 * rows, n)
            ctx.rlwe_ksk_gen(KEY, first, kind, s_to, out.t, key_level, alpha, sp, k, s_from=arg, galois_elt=g)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.blocks((beta * 2 * rows * n,)), mfhe.to_host_u64(want),
                                          err_msg=f"kind {kind} key_level {key_level} alpha {alpha}")
            out.check_pads()


def _crt(res, q):
    """Integers mod prod(q) from residues [len(q)][n]."""
    Q = km.prod(q)
    out = [0] * res.shape[1]
    for r, qi in enumerate(q):
        Mi = Q // qi
        c = Mi * pow(Mi, -1, qi)
        out = [(o + int(v) * c) % Q for o, v in zip(out, res[r])]
    return out


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("kind", ["switch", "relin", "galois"])
def test_keyswitch_with_a_generated_key_stays_within_the_bound(mfhe, bits, kind):
    """ks_model's N = 16 case (its moduli, secrets and ciphertexts; the key from mfhe_rlwe_ksk_gen): k_0 + k_1 s_to - c
    s_from is at most ks_model.error_bound(..., b_e = 21) at every level."""
    import torch
    cs = km.seeded_case(bits, "relin" if kind == "relin" else "switch", True)
    q, p, n, alpha, s_to = cs["q"], cs["p"], cs["n"], cs["alpha"], cs["s_to"]
    g = 5
    s_from = gm.sigma(s_to, g) if kind == "galois" else cs["s_from"]
    ctx = mfhe.Context(q + p, 4, mfhe.CONV_PHANTOM)
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    ints = torch.tensor([s_to, cs["s_from"] if kind != "galois" else s_to], dtype=torch.int32, device="cuda")
    sec = ctx.rlwe_lift_small(ints.ravel(), zeros(2 * 7 * n), 2, 5, 5, 2)
    d_to, d_from = sec[:7 * n], sec[7 * n:]
    code = {"switch": mfhe.RLWE_KEY_SWITCH, "relin": mfhe.RLWE_KEY_RELIN, "galois": mfhe.RLWE_KEY_GALOIS}[kind]
    ksk = ctx.rlwe_ksk_gen(KEY, 40, code, d_to, zeros(3 * 2 * 7 * n), 5, alpha, 5, 2,
                           s_from=d_from if kind == "switch" else None, galois_elt=g)
    for level in km.CASE_LEVELS:
        c = cs["c"][level]
        res = _u64([[int(v) % int(m) for v in c] for m in q[:level]])
        d_in = ctx.ntt_fwd(_dev(mfhe, res), 1, 0, level)
        o0, o1 = zeros(level * n), zeros(level * n)
        ctx.keyswitch(d_in, ksk, o0, o1, 1, level, 5, alpha, 5, 2)
        ctx.ntt_inv(o0, 1, 0, level)
        ctx.ntt_inv(o1, 1, 0, level)
        torch.cuda.synchronize()
        k0 = _crt(mfhe.to_host_u64(o0).reshape(level, n), q[:level])
        k1 = _crt(mfhe.to_host_u64(o1).reshape(level, n), q[:level])
        err = km.decryption_error(q, level, k0, k1, c, s_from, s_to)
        bound = km.error_bound(q, p, alpha, level, n, B_NOISE)
        print(f"{kind} bits {bits} level {level}: error {err}, bound {bound:.2f}")
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------
# 5. public-key encryption
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
@LAYOUT
def test_encrypt_pk_is_its_definition(mfhe, log_n, bits, layout):
    """c0 == pk0 u + e0 + m and c1 == pk1 u + e1 in Python integers with u, e0, e1 from sample_small; after
    mfhe_ntt_inv the centred coefficients of c0 + c1 s - m = e_pk u + e0 + e1 s are at most 21 (2 N + 1) (ternary u and
    s, every noise at most 21)."""
    import torch
    _, ppad, _, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(log_n + 200)
    for npoly, level in ((1, 1), (3, 5)):
        limbs = list(range(level))
        qc = _qcol(limbs, mod)
        s_dev, s = _secret(mfhe, ctx, 9, level, 0, n)
        pk0, pk1 = _polys(mfhe, 1, level, n), _polys(mfhe, 1, level, n)
        ctx.rlwe_encrypt_sk(KEY, 5, s_dev, None, pk0.t, pk1.t, 1, level)
        draws = []
        for stream in (mfhe.RLWE_EPHEMERAL, mfhe.RLWE_NOISE0, mfhe.RLWE_NOISE1):
            b = _polys(mfhe, npoly, level, n)
            ctx.rlwe_sample_small(KEY, stream, FIRST_ID, b.t, npoly, level)
            draws.append(b)
        torch.cuda.synchronize()
        u, e0, e1 = (b.blocks((npoly, level, n)).astype(object) for b in draws)
        p0, p1 = pk0.blocks((1, level, n)).astype(object), pk1.blocks((1, level, n)).astype(object)
        m = _random_rows(rng, (npoly,), [mod[l] for l in limbs], n)
        for msg in (m, None):
            mb = _polys(mfhe, npoly, level, n, ppad + 2, 0, msg) if msg is not None else None
            c0 = _polys(mfhe, npoly, level, n, ppad, base)
            c1 = _polys(mfhe, npoly, level, n, ppad, base)
            ctx.rlwe_encrypt_pk(KEY, FIRST_ID, pk0.t, pk1.t, mb.t if mb else None, c0.t, c1.t, npoly, level,
                                m_stride=mb.stride if mb else None, out_stride=c0.stride)
            torch.cuda.synchronize()
            add = msg.astype(object) if msg is not None else 0
            g0, g1 = c0.blocks((npoly, level, n)), c1.blocks((npoly, level, n))
            np.testing.assert_array_equal(g0, ((p0 * u + e0 + add) % qc).astype(np.uint64), err_msg="c0")
            np.testing.assert_array_equal(g1, ((p1 * u + e1) % qc).astype(np.uint64), err_msg="c1")
            c0.check_pads()
            c1.check_pads()
            d = ((g0.astype(object) + g1.astype(object) * s[None].astype(object) - add) % qc).astype(np.uint64)
            coef = _intt_rows(mfhe, ctx, d, level).astype(object)
            cen = np.where(coef > qc // 2, coef - qc, coef)
            worst = int(np.abs(cen).max())
            assert worst <= B_NOISE * (2 * n + 1), worst
            assert (cen == cen[:, :1]).all(), "the same small integer on every limb"
            assert worst > 0


# ---------------------------------------------------------------------------------------------------------------
# 6. decryption
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@LOGNS
@LAYOUT
def test_decrypt_equals_python_integers(mfhe, log_n, bits, layout):
    import torch
    _, ppad, _, base = layout
    ctx, mod, n = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(log_n + 300)
    for npoly in (1, 3):
        for rows in (1, 2, 5):
            rmod = list(mod[:rows])
            x0, x1 = _random_rows(rng, (npoly,), rmod, n), _random_rows(rng, (npoly,), rmod, n)
            s = _random_rows(rng, (1,), rmod, n)
            b0 = _polys(mfhe, npoly, rows, n, ppad, base, x0)
            b1 = _polys(mfhe, npoly, rows, n, ppad, base, x1)
            out = _polys(mfhe, npoly, rows, n, ppad + 2, base)
            ctx.rlwe_decrypt(b0.t, b1.t, _dev(mfhe, s), out.t, npoly, rows, in_stride=b0.stride, out_stride=out.stride)
            torch.cuda.synchronize()
            want = (x0.astype(object) + x1.astype(object) * s.astype(object)) % _qcol(range(rows), mod)
            np.testing.assert_array_equal(out.blocks((npoly, rows, n)), want.astype(np.uint64))
            out.check_pads()
            np.testing.assert_array_equal(b0.blocks((npoly, rows, n)), x0)
            np.testing.assert_array_equal(b1.blocks((npoly, rows, n)), x1)


# ---------------------------------------------------------------------------------------------------------------
# 7. graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_reserve(mfhe):
    """After rlwe_reserve, encrypt_pk and decrypt allocate nothing and copy nothing to the device: captured on one
    stream at N = 2^10 and replayed twice on changed messages, each replay equals the eager call."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, n = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: nothing cached, no workspace yet
    npoly, level = 2, 5
    ctx.rlwe_reserve(npoly, level)
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    s = ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, 0, zeros(level * n), 1, level)
    pk0, pk1 = ctx.rlwe_encrypt_sk(KEY, 1, s, None, zeros(level * n), zeros(level * n), 1, level)
    rng = np.random.default_rng(8)
    fresh = lambda: _dev(mfhe, _random_rows(rng, (npoly,), mod[:level], n))
    m = fresh()

    def run(c0, c1, dec):
        ctx.rlwe_encrypt_pk(KEY, 2, pk0, pk1, m, c0, c1, npoly, level)
        ctx.rlwe_decrypt(c0, c1, s, dec, npoly, level)

    outs = [zeros(npoly * level * n) for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(*outs)
    first = None
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [mfhe.to_host_u64(t).copy() for t in outs]
        eager = [zeros(npoly * level * n) for _ in range(3)]
        run(*eager)
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            np.testing.assert_array_equal(a, mfhe.to_host_u64(b))
            assert a.any()
        if first is not None:
            assert (first[0] != got[0]).any() and (first[2] != got[2]).any()
            np.testing.assert_array_equal(first[1], got[1])   # c1 does not depend on the message
        first = got
        m.copy_(fresh())


# ---------------------------------------------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
def test_end_to_end_with_no_host_arithmetic(mfhe, bits):
    """N = 2^10, level 8, alpha 2: secret and public key, a relinearisation key (RLWE_KEY_RELIN), slot_encode,
    encrypt_pk, poly_apply on the monomial degree-7 case of test_polynomials_seen_through_the_slots, decrypt,
    slot_decode; compared with p(z) from numpy.  Every step between the encoder and the decoder is a library call on
    device tensors.  The tolerance is poly_model.propagate's with the input error of a public-key encryption,
    N (1/2 + 21 (2 N + 1)) / scale plus the encoder's float term, and ks_model.error_bound(..., 21) per relinearisation;
    it is asserted below 1/64 of the spread of the expected slots before anything runs on the GPU.

    Measured on an MI355X (slot error / bound): 45-bit class 4.3e-9 / 4.8e-5 with e_in 1.25e-6,
    50-bit class 1.4e-10 / 1.5e-6 with e_in 3.9e-8; spread / 64 = 0.070."""
    import torch
    log_n, level, key_level, alpha, sp, k = 10, NQ, NQ, 2, NQ, NSP
    N, n = 1 << log_n, 1 << (log_n - 1)
    mod = _moduli(log_n, bits)
    q, p = list(mod[:level]), list(mod[sp:sp + k])
    scale = 2.0 ** bits[0]
    name, basis, coeffs, z, real = tpg._slot_cases(np.random.default_rng(77), n)[0]
    assert name.startswith("A monomial degree 7") and not real
    ctx = _ctx(log_n, bits)
    plan = ctx.poly_plan(coeffs, basis, scale, level)
    pd = pm.from_handle(plan, mod)
    want = pm.evaluate(coeffs, basis, z.astype(np.complex128))
    relin = {l: N * km.error_bound(q, p, alpha, l, N, B_NOISE) for l in range(2, level + 1)}
    fp_in, _ = tsg._fp_terms(z, log_n, scale)
    e_in = N * (0.5 + B_NOISE * (2 * N + 1)) / scale + fp_in
    intended, bound = pm.propagate(pd, z.astype(np.complex128), e_in, relin, N * (1 + N) / 2)
    bound += tsg._fp_terms(want, log_n, pd["out_scale"])[1] + pm.coefficient_arithmetic(coeffs, basis)
    bound += float(np.abs(intended - want).max())
    spread = max(np.ptp(want.real), np.ptp(want.imag))
    print(f"{name}: e_in {e_in:.3g}, bound {bound:.3g}, spread {spread:.3g}, out level {pd['out_level']}")
    assert bound < spread / 64, (bound, spread)
    ol = pd["out_level"]
    rows = min(ol, 2)
    assert (float(np.abs(want).max()) + bound) * pd["out_scale"] < int(q[0]) * int(q[1]) // 2
    # ---- everything above ran on the CPU; from here on the GPU, library calls alone ----
    seed = mfhe.Seed(KEY)
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    s = ctx.rlwe_sample_small(seed, mfhe.RLWE_SECRET, seed.take(), zeros((key_level + k) * N), 1, key_level, sp, k)
    pk0, pk1 = ctx.rlwe_encrypt_sk(seed, seed.take(), s, None, zeros(level * N), zeros(level * N), 1, level)
    beta = -(-key_level // alpha)
    rlk = ctx.rlwe_ksk_gen(seed, seed.take(beta), mfhe.RLWE_KEY_RELIN, s, zeros(beta * 2 * (key_level + k) * N),
                           key_level, alpha, sp, k)
    pt = ctx.slot_encode(torch.from_numpy(z.astype(np.complex128)).cuda(), zeros(level * N), 1, level, scale)
    c0, c1 = ctx.rlwe_encrypt_pk(seed, seed.take(), pk0, pk1, pt, zeros(level * N), zeros(level * N), 1, level)
    o0, o1 = zeros(ol * N), zeros(ol * N)
    ctx.poly_apply(plan, c0, c1, rlk, o0, o1, 1, key_level, alpha, sp, k)
    dec = ctx.rlwe_decrypt(o0, o1, s, zeros(rows * N), 1, rows, in_stride=ol * N)
    slots = ctx.slot_decode(dec, torch.zeros(n, dtype=torch.complex128, device="cuda"), 1, rows, pd["out_scale"])
    torch.cuda.synchronize()
    assert seed.next_id == 3 + beta
    err = float(np.abs(slots.cpu().numpy() - want).max())
    tsg._report(name + f" end to end ({bits[0]}-bit class)", err, bound)
    plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    log_n, bits = 4, (45, 49)
    mod, N = _moduli(log_n, bits), 16
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)
    h, E, L = ctx.handle, mfhe.EINVAL, len(mod)
    level, sp, k, alpha = 5, 8, 2, 2
    rows, beta = level + k, 3
    W = rows * N
    seed = mfhe.Seed(KEY).words
    a = _polys(mfhe, 2, rows, N)          # outputs
    b = _polys(mfhe, 2, rows, N)
    src = _polys(mfhe, 2, rows, N)        # inputs: never written
    key = _polys(mfhe, 1, beta * 2 * rows, N)
    ints = torch.zeros(2 * N, dtype=torch.int32, device="cuda")
    pa, pb, ps, pk_, pi = a.t.data_ptr(), b.t.data_ptr(), src.t.data_ptr(), key.t.data_ptr(), ints.data_ptr()

    def uni(seed=seed, out=pa, ost=W, npoly=2, level=level, sp=sp, k=k):
        return lib.mfhe_rlwe_sample_uniform(h, seed, 0, out, ost, npoly, level, sp, k, None)

    def small(seed=seed, stream=2, out=pa, ost=W, npoly=2, level=level, sp=sp, k=k, flags=0):
        return lib.mfhe_rlwe_sample_small(h, seed, stream, 0, out, ost, npoly, level, sp, k, flags, None)

    def lift(co=pi, cst=N, out=pa, ost=W, npoly=2, level=level, sp=sp, k=k, flags=0):
        return lib.mfhe_rlwe_lift_small(h, co, cst, out, ost, npoly, level, sp, k, flags, None)

    def esk(seed=seed, s=ps, m=ps + 8 * W, mst=W, c0=pa, c1=pb, ost=W, npoly=1, level=level, sp=sp, k=k):
        return lib.mfhe_rlwe_encrypt_sk(h, seed, 0, s, m, mst, c0, c1, ost, npoly, level, sp, k, None)

    def gen(seed=seed, kind=0, g=5, sf=ps, st=ps + 8 * W, ksk=pk_, key_level=level, alpha=alpha, sp=sp, k=k):
        return lib.mfhe_rlwe_ksk_gen(h, seed, 0, kind, g, sf, st, ksk, key_level, alpha, sp, k, None)

    def epk(seed=seed, p0=ps, p1=ps + 8 * W, m=None, mst=level * N, c0=pa, c1=pb, ost=level * N, npoly=2, level=level):
        return lib.mfhe_rlwe_encrypt_pk(h, seed, 0, p0, p1, m, mst, c0, c1, ost, npoly, level, None)

    def dec(c0=ps, c1=ps + 8 * W, ist=2 * N, s=pb, out=pa, ost=2 * N, npoly=1, rows=2):
        return lib.mfhe_rlwe_decrypt(h, c0, c1, ist, s, out, ost, npoly, rows, None)

    bad = [
        uni(seed=None), uni(out=None), small(seed=None), small(out=None), lift(co=None), lift(out=None),   # null pointers
        esk(seed=None), esk(s=None), esk(c0=None), esk(c1=None), gen(seed=None), gen(sf=None), gen(st=None),
        gen(ksk=None), gen(kind=1, st=None), epk(seed=None), epk(p0=None), epk(p1=None), epk(c0=None), epk(c1=None),
        dec(c0=None), dec(c1=None), dec(s=None), dec(out=None),
        small(stream=1), small(stream=0), small(stream=7), small(stream=-1),                               # streams
        gen(kind=3), gen(kind=-1),                                                                         # kinds
        small(flags=2), lift(flags=4),                                                                     # flags
        gen(kind=2, g=4), gen(kind=2, g=0), gen(kind=2, g=2 * N + 1), gen(kind=2, g=-3),                   # Galois element
        uni(ost=W - 1), small(ost=W - 1), lift(ost=W - 1), lift(cst=N - 1), esk(ost=W - 1), esk(mst=W - 1),  # strides
        epk(ost=level * N - 1), epk(m=ps, p0=pk_, p1=pk_ + 8 * W, mst=level * N - 1), dec(ist=2 * N - 1),
        dec(ost=2 * N - 1),
        esk(c1=pa + 8), esk(s=pa), esk(m=pb + 8 * (W - 1)), gen(st=pk_), gen(sf=pk_ + 8 * (beta * 2 * W - 1)),  # overlaps
        epk(c1=pa + 8 * (level * N - 1)), epk(p0=pa), epk(p1=pb), epk(m=pa, npoly=1), dec(out=ps), dec(s=pa),
        dec(out=ps + 8 * W + 8), lift(co=pa + 8, npoly=1),
        uni(level=0), uni(level=L + 1), small(level=0), lift(level=L + 1), esk(level=0), epk(level=0),      # level
        epk(level=L + 1), dec(rows=0), dec(rows=L + 1), gen(key_level=0), gen(alpha=0),
        uni(k=-1), uni(sp=4), small(sp=L), lift(sp=9, k=2), esk(sp=3), gen(sp=4), gen(k=0), gen(sp=9, k=2),   # special range
        lib.mfhe_rlwe_reserve(h, 2, 0, sp, k), lib.mfhe_rlwe_reserve(h, 2, level, 2, k),
        lib.mfhe_rlwe_reserve(None, 2, level, sp, k),
    ]
    assert bad == [E] * len(bad), [i for i, v in enumerate(bad) if v != E]
    torch.cuda.synchronize()
    assert all(x.all_canary() for x in (a, b, src, key)), "a rejected call wrote something"
    ok = [uni(npoly=0), small(npoly=0), lift(npoly=0), esk(npoly=0), epk(npoly=0), dec(npoly=0),
          uni(npoly=0, k=0, sp=99)]                    # special_start is ignored without special rows
    assert ok == [mfhe.OK] * len(ok), ok
    torch.cuda.synchronize()
    assert all(x.all_canary() for x in (a, b, src, key)), "npoly == 0 launched something"
    noph = mfhe.Context(list(_moduli(5, bits)), 4, mfhe.CONV_GL)   # q = 1 mod 4N, no phantom tables
    assert lib.mfhe_rlwe_sample_uniform(noph.handle, seed, 0, pa, W, 1, level, sp, k, None) == mfhe.ENOTREADY
    assert lib.mfhe_rlwe_decrypt(noph.handle, ps, ps + 8 * W, 2 * N, pb, pa, 2 * N, 1, 2, None) == mfhe.ENOTREADY
    assert lib.mfhe_rlwe_reserve(noph.handle, 1, level, sp, k) == mfhe.ENOTREADY
    tiny = mfhe.Context(list(_moduli(4, bits)), 2, mfhe.CONV_PHANTOM)
    assert lib.mfhe_rlwe_reserve(tiny.handle, 1, 1, 0, 0) == mfhe.EUNSUPPORTED
    with pytest.raises(ValueError):
        ctx.rlwe_sample_uniform(KEY, 0, torch.zeros(W - 1, dtype=torch.int64, device="cuda"), 1, level, sp, k)
    with pytest.raises(ValueError):
        ctx.rlwe_lift_small(torch.zeros(N, dtype=torch.int64, device="cuda"), a.t, 1, level, sp, k)
    with pytest.raises(ValueError):
        ctx.rlwe_sample_small(b"short", 2, 0, a.t, 1, level, sp, k)
