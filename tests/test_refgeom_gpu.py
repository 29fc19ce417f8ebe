"""The pipeline at the reference's own geometry (n = 64, 512 lanes, the 11 reference moduli, CONV_PHANTOM | CONV_WCRT,
delta 2^35) held to the oracle, bit for bit wherever integers are visible, and to the long-double model of
tests/cdft_model.py where only doubles are.

At this shape, and only here, the default options run enc_ring_kernel<6> / dec_ring_kernel<6>, the 64 x 128 tile of
mod_gemm_mfma_smallb_kernel<D, 2>, the direct-a GEMM output, the decrypt-fused digitize (mfma_digitize_ifold_dec_kernel,
its pair form, dec_colsum*), the 7-word compose and the 11-limb pair launches, with the 6-digit limb 0 beside ten
5-digit limbs at P = 4096 columns.  Elsewhere in the suite they are compared with other HIP paths only.

The oracle's products are computed once per process in tests/refgeom.py (tests/test_refgeom_cpu.py checks the
arguments they rest on); comparisons of whole [512][11][4096] arrays are made on the device and fall back to numpy
only to report a mismatch.  Tolerances: cdft_model.bound alone; everything else is equality."""
import contextlib

import numpy as np
import pytest

import cdft_model as cm
import refgeom as rg
from he_checks import encrypt_decrypt_vs_oracle

pytestmark = pytest.mark.gpu

CGEMM_MODES = (2, 3, 1, 0)      # MFHE_OPT_CGEMM_MFMA, as tests/test_cdft_gpu.py
STREAMS = (3, 2, 0)             # MFHE_OPT_HE_STREAMS: encode pairs + decode side stream (default), pairs, one stream
# (OPT_WCRT_MFMA, OPT_WCRT_PIPE), as test_he_gpu.py::test_wcrt_mfma_matches_valu_and_oracle
WCRT_MODES = [(1, 0), (1, 1), (1, 2), (1, 3), (3, 0), (3, 1), (3, 2), (3, 3), (2, 0), (0, 0)]


def _defaults(mfhe):
    return {mfhe.OPT_WCRT_MFMA: 1, mfhe.OPT_WCRT_PIPE: 0, mfhe.OPT_HE_FUSED: 1, mfhe.OPT_ENC_A_DIRECT: 1,
            mfhe.OPT_HE_STREAMS: 3, mfhe.OPT_ENC_E_SMALL: 1, mfhe.OPT_CGEMM_MFMA: 2}


@pytest.fixture(scope="module")
def geom(mfhe, orc):
    ctx = mfhe.Context(rg.RNS, rg.LOG_N, rg.CONV, rg.DELTA)
    yield ctx, rg.he(orc)
    ctx.close()
    rg.drop()


def _assert_geometry(mfhe, ctx):
    """What every test here relies on: the default kernels and the reference's sizes."""
    for opt, want in _defaults(mfhe).items():
        assert ctx.get_option(opt) == want, (opt, want)
    info = ctx.info()
    assert (info.num_limbs, info.log_n, info.phi, info.conventions, info.delta) == (11, 6, 512, rg.CONV, rg.DELTA)
    assert 512 * info.num_limbs * (1 << info.log_n) ** 2 == rg.WORDS == 23068672
    assert ctx.crt_words == info.crt_words == 7
    assert [rg.wcrt_digits(q) for q in rg.RNS] == [6] + [5] * 10


@contextlib.contextmanager
def _options(mfhe, ctx, **opts):
    """Set OPT_<name> = value for the block; every option is back at its default afterwards."""
    try:
        for name, v in opts.items():
            ctx.set_option(getattr(mfhe, "OPT_" + name), v)
        yield
    finally:
        for opt, v in _defaults(mfhe).items():
            ctx.set_option(opt, v)


def _same(mfhe, got, want_dev, what):
    """got == want_dev, both on the device; the numpy comparison only words the failure."""
    import torch
    if not torch.equal(got, want_dev):
        np.testing.assert_array_equal(mfhe.to_host_u64(got), mfhe.to_host_u64(want_dev), err_msg=what)
        raise AssertionError(what)


# ------------------------------------------------------------------ 1. W-CRT, every mode
def test_wcrt_every_mode_matches_oracle(mfhe, orc, geom):
    """wcrt_fwd == orc_wntt_forward_matrix, wcrt_inv(forward) == input, wcrt_inv(random poly-major residues) ==
    orc_wntt_inverse_matrix, wcrt_fwd_vector == orc_wntt_forward_vector, in each of the ten (MFMA mode, K pipeline)
    pairs; lane w = 0 of the input and the first n polynomials of the poly-major one are all q - 1."""
    import torch
    ctx, _ = geom
    _assert_geometry(mfhe, ctx)
    p = rg.wcrt_products(orc)
    assert all((p["x"].reshape(512, 11, 4096)[0, l] == q - 1).all() for l, q in enumerate(rg.RNS))
    dx, dxp, dv, rf, rb2, rv = (mfhe.to_device_u64(p[k]) for k in ("x", "xp", "v", "ref_f", "ref_b2", "ref_v"))
    rg.drop("wcrt")
    del p
    for mf, pipe in WCRT_MODES:
        with _options(mfhe, ctx, WCRT_MFMA=mf, WCRT_PIPE=pipe):
            f, b, b2, vo = torch.empty_like(dx), torch.empty_like(dx), torch.empty_like(dx), torch.empty_like(dv)
            ctx.wcrt_fwd(dx, f)
            ctx.wcrt_inv(f, b)
            ctx.wcrt_inv(dxp, b2)
            ctx.wcrt_fwd_vector(dv, vo)
            torch.cuda.synchronize()
        tag = f" mode={mf} pipe={pipe}"
        _same(mfhe, f, rf, "fwd" + tag)
        _same(mfhe, b, dx, "inv(fwd)" + tag)
        _same(mfhe, b2, rb2, "inv(random)" + tag)
        _same(mfhe, vo, rv, "vector" + tag)


# ------------------------------------------------------------------ 2. keygen, encrypt, decrypt
def test_encrypt_decrypt_every_word_vs_oracle(mfhe, orc, geom):
    """The n = 8 / n = 32 check of test_he_gpu.py (he_checks.encrypt_decrypt_vs_oracle) at n = 64, L = 11, then more:
    b equals the oracle's on every word.  The samplers are index-hashed, so the inputs are fixed; the noise draw
    nearest a llround tie is 2.2e-7 from it (test_refgeom_cpu.py) and device libm is within a few ulp of glibc, so no
    draw rounds differently.  Then encrypt_pair / decrypt_to_eval again, against the same oracle arrays, with the
    unfused ring kernels, the factored noise W-CRT, a through the poly-major buffer, one stream and the pair
    launches; and encrypt(m_re) == the oracle's ct_re."""
    import torch
    ctx, h = geom
    _assert_geometry(mfhe, ctx)
    r = encrypt_decrypt_vs_oracle(mfhe, orc, 64, ctx, h, rg.RNS)
    np.testing.assert_array_equal(r["gre"], r["ore"])
    np.testing.assert_array_equal(r["gim"], r["oim"])
    ore, oim, ev_ref = (mfhe.to_device_u64(r[k]) for k in ("ore", "oim", "ev_ref"))
    m_re, m_im = mfhe.to_device_u64(r["m_re"]), mfhe.to_device_u64(r["m_im"])
    sk = r["sk"]
    del r
    variants = [dict(), dict(HE_FUSED=0), dict(ENC_E_SMALL=0), dict(ENC_A_DIRECT=0), dict(HE_STREAMS=0),
                dict(HE_STREAMS=2)]
    for opts in variants:
        with _options(mfhe, ctx, **opts):
            cre = torch.full((2 * rg.WORDS,), -1, dtype=torch.int64, device="cuda")
            cim = torch.full_like(cre, -1)
            ctx.encrypt_pair(m_re, m_im, sk, cre, cim)
            ev = torch.full((rg.WORDS,), -1, dtype=torch.int64, device="cuda")
            ctx.decrypt_to_eval(ore, sk, ev)
            ct = torch.full_like(cre, -1)
            ctx.encrypt(m_re, sk, ct)
            torch.cuda.synchronize()
        _same(mfhe, cre, ore, f"encrypt_pair re {opts}")
        _same(mfhe, cim, oim, f"encrypt_pair im {opts}")
        _same(mfhe, ev, ev_ref, f"decrypt_to_eval {opts}")
        _same(mfhe, ct, ore, f"encrypt {opts}")


# ------------------------------------------------------------------ 3. decrypt_and_decode on planted integers
def _lanes_of(msg, lanes_dev):
    """The checked lanes of a device message [512][64][64] interleaved complex, on the host."""
    got = msg.view(512, 64 * 64 * 2)[lanes_dev].cpu().numpy()
    assert np.all(np.isfinite(got))
    return got.view(np.complex128).reshape(-1, 64, 64)


@pytest.mark.parametrize("bits", [20, 40])
def test_decrypt_and_decode_planted_integers(mfhe, orc, geom, bits):
    """decrypt_and_decode is the only route to the decrypt-fused digitize, and its integers are visible only through
    FP64.  The ciphertexts of refgeom.planted_ct decrypt to exactly the planted k, so the message is the model's
    decode_truth(k) and E_gpu <= cm.bound(E_ref, S) (4 E_ref + 8 * 2^-53 * S), E_ref the oracle's decode
    of the same words.  At |k| < 2^20 that bound is below 2^-36 (asserted before anything runs), while one
    coefficient off by one unit moves every output by 2^-35: a single wrong unit anywhere fails.  |k| < 2^40 is the
    range of the n = 8 / 16 cases of test_cdft_gpu.py.  Every CGEMM mode under HE_STREAMS 3, 2 and 0; and
    decrypt_to_eval(ct_re) == ev_re bit for bit."""
    import torch
    ctx, h = geom
    _assert_geometry(mfhe, ctx)
    p = rg.planted_ct(orc, bits)
    if bits == 20:
        assert cm.bound(p["e_ref"], p["scale"]) < 2.0 ** -36
    sk = torch.empty(512 * 11 * 64, dtype=torch.int64, device="cuda")
    ctx.keygen(sk)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mfhe.to_host_u64(sk), rg.sk_ref(orc))
    ct_re, ct_im, ev_re = (mfhe.to_device_u64(p[k]) for k in ("ct_re", "ct_im", "ev_re"))
    lanes_dev = torch.from_numpy(p["lanes"]).cuda()
    rep = cm.Report()
    for streams in STREAMS:
        for mode in CGEMM_MODES:
            with _options(mfhe, ctx, HE_STREAMS=streams, CGEMM_MFMA=mode):
                msg = torch.full((2 * 512 * 4096,), float("nan"), dtype=torch.float64, device="cuda")
                ctx.decrypt_and_decode(ct_re, ct_im, sk, msg)
                torch.cuda.synchronize()
            rep.line(f"dec+decode s{streams}", f"int{bits}", 64, mode, cm.err(_lanes_of(msg, lanes_dev), p["truth"]),
                     p["e_ref"], p["e_best"], p["scale"])
        with _options(mfhe, ctx, HE_STREAMS=streams):
            ev = torch.full((rg.WORDS,), -1, dtype=torch.int64, device="cuda")
            ctx.decrypt_to_eval(ct_re, sk, ev)
            torch.cuda.synchronize()
        _same(mfhe, ev, ev_re, f"decrypt_to_eval, streams {streams}")
    if bits == 20:
        rg.drop("planted_ct")        # the 2^40 arrays stay for the decode test below
    rep.check()


# ------------------------------------------------------------------ 4. decode's FP path, encode recovering integers
def test_decode_fp_path_vs_model(mfhe, orc, geom):
    """test_cdft_gpu.py::test_decode_fp_path_vs_model at n = 64, L = 11 (the 7-word compose, the 11-limb pair launch):
    ctx.decode of the W-CRT image of planted |k| < 2^40 (the oracle's forward, which wcrt_fwd equals bit for bit)
    against the model, E_ref the oracle's decode of the same words.  A fresh context whose first call is decode, as
    there; every CGEMM mode under HE_STREAMS 3, 2, 0."""
    import torch
    ctx0, h = geom
    _assert_geometry(mfhe, ctx0)
    p = rg.planted_ct(orc, 40)
    ctx = mfhe.Context(rg.RNS, rg.LOG_N, rg.CONV, rg.DELTA)
    _assert_geometry(mfhe, ctx)
    pre, pim = mfhe.to_device_u64(p["ev_re"]), mfhe.to_device_u64(p["ev_im"])
    lanes_dev = torch.from_numpy(p["lanes"]).cuda()
    rep = cm.Report()
    for streams in STREAMS:
        for mode in CGEMM_MODES:
            with _options(mfhe, ctx, HE_STREAMS=streams, CGEMM_MFMA=mode):
                out = torch.full((2 * 512 * 4096,), float("nan"), dtype=torch.float64, device="cuda")
                ctx.decode(pre, pim, out)
                torch.cuda.synchronize()
            rep.line(f"decode s{streams}", "int40", 64, mode, cm.err(_lanes_of(out, lanes_dev), p["truth"]), p["e_ref"],
                     p["e_best"], p["scale"])
    ctx.close()
    rg.drop("planted_ct")
    rep.check()


def test_encode_recovers_planted_integers(mfhe, orc, geom):
    """test_cdft_gpu.py::test_encode_recovers_planted_integers at n = 64, L = 11: the message of
    refgeom.planted_message (|k| < 2^30, f in [-0.4, 0.4] on 1058 fixed columns, exact zero elsewhere; the oracle's
    float64 stages land within 0.025 of k + f, asserted before anything runs) encodes to k: after matrix_to_poly and
    wcrt_inv every residue on every limb is k mod q_l, in every CGEMM mode under HE_STREAMS 3, 2, 0."""
    import torch
    ctx, h = geom
    _assert_geometry(mfhe, ctx)
    m = rg.planted_message(orc)
    print(f"CDFT | encode precondition n=64: |k| < 2^{m['k_bits']} on {m['cols'].size} columns, oracle max "
          f"|delta wc - (k + f)| = {m['pre_err']:.3e} (<= 0.025)")
    assert m["pre_err"] <= 0.025
    mt = torch.from_numpy(m["msg"].view(np.float64).reshape(-1).copy()).cuda()
    want = {"re": mfhe.to_device_u64(rg.residues(m["k_re"], rg.RNS)),
            "im": mfhe.to_device_u64(rg.residues(m["k_im"], rg.RNS))}
    rg.drop("planted_msg")
    bad = []
    for streams in STREAMS:
        for mode in CGEMM_MODES:
            with _options(mfhe, ctx, HE_STREAMS=streams, CGEMM_MFMA=mode):
                gre = torch.full((rg.WORDS,), -1, dtype=torch.int64, device="cuda")
                gim = torch.full_like(gre, -1)
                ctx.encode(mt, gre, gim)
                for g, part in ((gre, "re"), (gim, "im")):
                    poly, back = torch.empty_like(g), torch.empty_like(g)
                    ctx.matrix_to_poly(g, poly)
                    ctx.wcrt_inv(poly, back)
                    torch.cuda.synchronize()
                    wrong = int(torch.count_nonzero(back != want[part]))
                    print(f"CDFT | encode planted  | {part}      | n=64  | mode {mode} | streams {streams} | wrong "
                          f"residues {wrong} of {rg.WORDS}")
                    if wrong:
                        bad.append((streams, mode, part, wrong))
    assert not bad, bad
