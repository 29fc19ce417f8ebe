"""GPU parity of the W-CRT GEMMs over every modulus size mfhe_ctx_create accepts for MFHE_CONV_WCRT.

The reference's W-CRT (init_wntt_tables + the wntt_forward/inverse_matrix kernels, /root/reference/src/core/HE.cu:
237-273, 716-781) uses an __int128 % per product. It takes any prime q = 1 mod 771. This build has three
W-CRT paths (csrc/wcrt_gemm.hip, csrc/ctx.cpp build_wcrt):
* i8 MFMA digit-split GEMMs, D = ceil(bits / 8) balanced base-256 digits, for 2^27 < q < 2^59:
  * D = 5 or 6 (q below ~2^46.99): factored (771 = 3 x 257) or dense;
  * D = 7 (up to ~2^54.99) and D = 8 (up to 2^59): dense only;
  * q >= 2^50: the U64 epilogue instead of the FP64 one.
* the u128 VALU kernel: the only path when some q <= 2^27.
* mfhe_ctx_create rejects W-CRT moduli >= 2^59 (MFHE_EUNSUPPORTED).
VERDICT r05 found the D = 7 / 8 instantiations and the q <= 2^27 fallback compiled but never run. Here every mode of
every size runs the three layouts: forward matrix -> poly, inverse poly -> matrix, forward vector. The checks, all
bit-exact:
* against the VALU kernel;
* against the oracle (orc_wntt_forward_matrix / inverse, a restatement of HE.cu:716-781);
* inverse(forward(x)) == x.
"""
import numpy as np
import pytest

from oracle import P, U64
from primes import primes_of_size

pytestmark = pytest.mark.gpu

CONV = 1 | 4            # PHANTOM | WCRT
M771 = 256 * 771        # q = 1 mod 771 (W-CRT) and mod 2N for the phantom tables (n <= 128)
# bits -> (expected digit count D, or 0 for the VALU-only path)
SIZES = {20: 0, 27: 0, 28: 5, 35: 5, 40: 6, 46: 6, 47: 7, 48: 7, 50: 7, 55: 8, 56: 8, 59: 8}
MODES = [(1, 0), (1, 2), (3, 0), (3, 1), (3, 2), (3, 3), (2, 0), (0, 0)]   # (OPT_WCRT_MFMA, OPT_WCRT_PIPE)


def _digits(q: int) -> int:
    """ctx.cpp wcrt_digits: the smallest d with q - 1 <= 127 (256^d - 1) / 255."""
    d, top = 1, 127
    while d < 9 and q - 1 > top:
        top = top * 256 + 127
        d += 1
    return d


def _oracle_tables(orc, moduli):
    """V and V^-T of every limb, [L][512][512] each (orc_wcrt_tables: what orc_he_create builds, for any L)."""
    t = [orc.wcrt_tables(q) for q in moduli]
    return np.concatenate([v for v, _ in t]), np.concatenate([vi for _, vi in t])


def _every_mode_matches_valu_and_oracle(mfhe, orc, ctx, moduli, n, seed, what):
    """Every (OPT_WCRT_MFMA, OPT_WCRT_PIPE) of MODES on ctx: forward matrix -> poly, inverse of the forward, inverse of
    arbitrary canonical residues, forward vector, each equal to the oracle's (the last mode is the VALU kernel)."""
    import torch
    L = len(moduli)
    rng = np.random.default_rng(seed)
    qv = np.array(moduli, np.uint64)
    x = (rng.integers(0, 2 ** 63, (512, L, n * n), dtype=np.uint64) % qv[None, :, None]).ravel()
    x[:L * n * n] = np.repeat(qv - np.uint64(1), n * n)   # the all-(q - 1) first lane: the largest digit sums
    v = (rng.integers(0, 2 ** 63, (512, L, n), dtype=np.uint64) % qv[None, :, None]).ravel()
    V, VinvT = _oracle_tables(orc, moduli)
    ref_f = np.zeros_like(x)
    orc.L.orc_wntt_forward_matrix(P(x), P(ref_f), n, L, 512, P(U64(moduli)), P(V))
    ref_b = np.zeros_like(x)
    orc.L.orc_wntt_inverse_matrix(P(ref_f), P(ref_b), n, L, 512, P(U64(moduli)), P(VinvT))
    np.testing.assert_array_equal(ref_b, x)
    ref_v = np.zeros_like(v)
    orc.L.orc_wntt_forward_vector(P(v), P(ref_v), n, L, 512, P(U64(moduli)), P(V))
    # the inverse of arbitrary canonical residues too, laid out poly-major [w n + y][limb][x] (its input layout), with
    # the all-(q - 1) lane w = 0
    xp = (rng.integers(0, 2 ** 63, (512 * n, L, n), dtype=np.uint64) % qv[None, :, None])
    xp[:n] = (qv - np.uint64(1))[None, :, None]
    xp = xp.ravel()
    ref_b2 = np.zeros_like(xp)
    orc.L.orc_wntt_inverse_matrix(P(xp), P(ref_b2), n, L, 512, P(U64(moduli)), P(VinvT))
    dx, dv, dxp = mfhe.to_device_u64(x), mfhe.to_device_u64(v), mfhe.to_device_u64(xp)
    for mf, pipe in MODES:
        ctx.set_option(mfhe.OPT_WCRT_MFMA, mf)
        ctx.set_option(mfhe.OPT_WCRT_PIPE, pipe)
        f = torch.empty_like(dx)
        ctx.wcrt_fwd(dx, f)
        b = torch.empty_like(dx)
        ctx.wcrt_inv(f, b)
        vo = torch.empty_like(dv)
        ctx.wcrt_fwd_vector(dv, vo)
        torch.cuda.synchronize()
        tag = f"{what} mode={mf} pipe={pipe}"
        np.testing.assert_array_equal(mfhe.to_host_u64(f), ref_f, err_msg="fwd " + tag)
        # the inverse of arbitrary residues too (not only of the forward's output)
        np.testing.assert_array_equal(mfhe.to_host_u64(b), x, err_msg="inv " + tag)
        b2 = torch.empty_like(dx)
        ctx.wcrt_inv(dxp, b2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(b2), ref_b2, err_msg="inv(random) " + tag)
        np.testing.assert_array_equal(mfhe.to_host_u64(vo), ref_v, err_msg="vector " + tag)
    ctx.set_option(mfhe.OPT_WCRT_MFMA, 1)
    ctx.set_option(mfhe.OPT_WCRT_PIPE, 0)


@pytest.mark.parametrize("bits", sorted(SIZES))
def test_wcrt_every_mode_every_size_matches_valu_and_oracle(mfhe, orc, bits):
    n, log_n = 8, 3
    moduli = primes_of_size(bits, M771, 2)   # two limbs where the size class holds two such primes (20 bits: one)
    L = len(moduli)
    assert L >= 1 and all(q.bit_length() == bits for q in moduli)
    want_d = SIZES[bits]
    if want_d:
        assert max(max(5, _digits(q)) for q in moduli) == want_d, [_digits(q) for q in moduli]
    ctx = mfhe.Context(moduli, log_n, CONV)
    _every_mode_matches_valu_and_oracle(mfhe, orc, ctx, moduli, n, bits, f"bits={bits}")
    ctx.close()


# Contexts of mixed limb sizes: name -> (n, bits per limb, digits the GEMM takes per limb).  The reference moduli give
# the suite's only other mixed context (digits 6, 5, 5, ...: one run boundary, bit 0 of d6 alone, plane stride 6).
MIXED = {
    # FP64 epilogue, D = 6, factored and ring56 paths; d6 = 0b101010; other pipes: for_digit_runs<5, 6> in six runs
    "d6_101010": (8, [35, 46, 35, 40, 28, 46], [5, 6, 5, 6, 5, 6]),
    # all below 2^50, D = 7, dense only: runs 5 | 7 | 6 | 7, 7 | 5 reading planes at stride 7
    "stride7": (8, [35, 48, 46, 48, 47, 28], [5, 7, 6, 7, 7, 5]),
    # a modulus >= 2^50: the U64 epilogue on every limb, D = 8: runs 5 | 8 | 5 | 7 | 8 | 6, 6 at stride 8
    "stride8_u64": (8, [35, 56, 35, 48, 59, 46, 46], [5, 8, 5, 7, 8, 6, 6]),
    # one limb at or below 2^27 sends every limb to the VALU kernel, whatever the options say
    "valu": (8, [40, 20, 46], [6, 5, 6]),
    # L = 65 at n = 4: ring56_all and the pair launch refuse (L > 64); for_digit_runs gives [0, 64) at 5 digits and
    # [64, 65) at 6 with l0 = 64; the digitize writes all D planes for limb 64 (PlaneCounts holds 64 limbs)
    "L65": (4, [28] * 64 + [46], [5] * 64 + [6]),
}


def _mixed_moduli(bits):
    """Limb i: the next unused prime of its size, primes_of_size(bits, M771, count)[k] for the size's k-th use."""
    used, out = {}, []
    for b in bits:
        k = used.get(b, 0)
        used[b] = k + 1
        out.append(primes_of_size(b, M771, bits.count(b))[k])
    assert len(set(out)) == len(bits) and all(q.bit_length() == b for q, b in zip(out, bits))
    return out


@pytest.mark.parametrize("name", sorted(MIXED))
def test_wcrt_mixed_limb_sizes_match_valu_and_oracle(mfhe, orc, name):
    """The checks, modes and layouts of the test above on contexts whose limbs need different digit counts: more than
    two digit runs, runs that start past limb 0, 5- / 6- / 7-digit kernels reading planes laid out at stride 7 or 8,
    the U64 epilogue on small limbs, d6 bits above bit 0, the all-VALU fallback, and L > 64.

    L65: sixty-four 35-bit primes and a 46-bit one would have the same digit runs, but mfhe_ctx_create refuses that
    set (its product, 2^2254, is above 2^2047, the 32-word limit of the wide CRT; asserted below), so the 64 five-digit
    limbs are 28-bit primes (product 2^1806, 29 words).  It also runs encode -> decode once under the reference's 1e-3
    bound, where the pair launches fall back at 2 L > 128, and prints the context's creation time."""
    import time
    import torch
    n, bits, digits = MIXED[name]
    moduli = _mixed_moduli(bits)
    L = len(moduli)
    assert [max(5, _digits(q)) for q in moduli] == digits
    if name == "d6_101010":
        assert sum(1 << l for l, d in enumerate(digits) if d == 6) == 0b101010
    if name in ("d6_101010", "stride7"):
        assert max(moduli) < 2 ** 50
    if name == "stride8_u64":
        assert max(moduli) >= 2 ** 50
    if name == "valu":
        assert min(moduli) <= 2 ** 27
    else:
        assert min(moduli) > 2 ** 27
    t0 = time.perf_counter()
    ctx = mfhe.Context(moduli, n.bit_length() - 1, CONV)
    t_create = time.perf_counter() - t0
    _every_mode_matches_valu_and_oracle(mfhe, orc, ctx, moduli, n, 1000 + L, name)
    if name == "L65":
        print(f"WCRT | L = 65 context (n = 4, {ctx.crt_words} CRT words): created in {t_create:.2f} s")
        wide = primes_of_size(35, M771, 64) + [moduli[-1]]
        assert len(set(wide)) == 65
        with pytest.raises(mfhe.MfheError) as e:
            mfhe.Context(wide, 2, CONV)
        assert e.value.code == mfhe.EUNSUPPORTED
        rng = np.random.default_rng(65)
        msg = 100.0 * (rng.standard_normal(512 * n * n) + 1j * rng.standard_normal(512 * n * n))
        mt = torch.from_numpy(msg.view(np.float64).copy()).cuda()
        words = 512 * L * n * n
        out = {}
        for streams in (3, 0):
            ctx.set_option(mfhe.OPT_HE_STREAMS, streams)
            re_ = torch.full((words,), -1, dtype=torch.int64, device="cuda")
            im_, pre, pim = torch.full_like(re_, -1), torch.full_like(re_, -1), torch.full_like(re_, -1)
            dec = torch.full_like(mt, float("nan"))
            ctx.encode(mt, re_, im_)
            ctx.matrix_to_poly(re_, pre)
            ctx.matrix_to_poly(im_, pim)
            ctx.decode(pre, pim, dec)
            torch.cuda.synchronize()
            out[streams] = (mfhe.to_host_u64(re_), mfhe.to_host_u64(im_), dec.cpu().numpy())
        for a, b in zip(out[3], out[0]):
            np.testing.assert_array_equal(a, b)
        err = float(np.max(np.abs(out[3][2].view(np.complex128) - msg)))
        print(f"WCRT | L = 65 round trip |decode(encode(m)) - m| = {err:.3e} (reference bound 1e-3)")
        assert err < 1e-3
    ctx.close()


def test_wcrt_rejects_moduli_from_2_59(mfhe):
    """The one size the W-CRT tables refuse: q >= 2^59 (512-term u128 accumulation, D <= 8)."""
    q = primes_of_size(60, M771, 1)
    with pytest.raises(mfhe.MfheError) as e:
        mfhe.Context(q, 3, CONV)
    assert e.value.code == mfhe.EUNSUPPORTED
