"""keygen / encrypt_pair / decrypt_to_eval against the oracle on identical inputs: the one check that
tests/test_he_gpu.py (n = 8, 32) and tests/test_refgeom_gpu.py (n = 64) share."""
import numpy as np

from oracle import P, U64


def encrypt_decrypt_vs_oracle(mfhe, orc, n, ctx, h, moduli):
    """Returns what it computed, for callers that check more: the messages, the keys and both sides' ciphertexts."""
    import torch
    Lq = len(moduli)
    words = 512 * Lq * n * n
    rng = np.random.default_rng(3)
    qm = np.array(moduli, np.uint64)[None, :, None]
    m_re, m_im = ((rng.integers(0, 2 ** 63, (512, Lq, n * n), dtype=np.uint64) % qm).ravel() for _ in range(2))
    sk_ref = h.keygen()
    sk = torch.empty(512 * Lq * n, dtype=torch.int64, device="cuda")
    ctx.keygen(sk)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mfhe.to_host_u64(sk), sk_ref)
    cre = torch.empty(2 * words, dtype=torch.int64, device="cuda")
    cim = torch.empty_like(cre)
    ctx.encrypt_pair(mfhe.to_device_u64(m_re), mfhe.to_device_u64(m_im), sk, cre, cim)
    ore, oim = h.encrypt_pair(m_re, m_im, sk_ref)
    torch.cuda.synchronize()
    gre, gim = mfhe.to_host_u64(cre), mfhe.to_host_u64(cim)
    np.testing.assert_array_equal(gre[words:], ore[words:])           # a: uniform sampler + W-CRT, exact
    np.testing.assert_array_equal(gim[words:], oim[words:])
    # b contains the Box-Muller Gaussian (device libm vs glibc may differ in the last ulp of log/cos,
    # which can move llround at a .5 boundary): require >= 99.999 % exact agreement
    assert np.mean(gre[:words] != ore[:words]) < 1e-5
    assert np.mean(gim[:words] != oim[:words]) < 1e-5
    # ... and exactly: b differs from the oracle's only by the W-CRT image of a noise difference (b is linear in
    # e), so the oracle's inverse W-CRT of (b_dev - b_orc) must be a noise difference in {-1, 0, +1}, the same
    # integer in every limb, nonzero only where the unrounded Box-Muller sample sits on a .5 rounding boundary
    # (HE.cu:605-627: the only step where device libm and glibc may differ)
    n2 = n * n
    q3 = np.array(moduli, np.uint64)[None, :, None]
    noise = []
    for got, want in ((gre, ore), (gim, oim)):
        # (got - want) mod q on canonical residues, in u64 (Python integers would take gigabytes at n = 64)
        g3, w3 = got[:words].reshape(512, Lq, n2), want[:words].reshape(512, Lq, n2)
        d = np.where(g3 >= w3, g3 - w3, g3 + q3 - w3).ravel()
        poly, de = np.zeros_like(d), np.zeros_like(d)
        orc.L.orc_matrix_to_poly(P(d), P(poly), n, Lq, 512)
        orc.L.orc_wntt_inverse_matrix(P(poly), P(de), n, Lq, 512, P(U64(moduli)), orc.L.orc_he_VinvT(h.h))
        de = de.reshape(512, Lq, n2)
        sgn = np.where(de == 0, 0, np.where(de == 1, 1, np.where(de == q3 - 1, -1, 99)))
        assert (sgn != 99).all(), "ciphertexts differ by more than a +-1 noise step"
        assert (sgn == sgn[:, :1, :]).all(), "noise difference not the same integer in every limb"
        noise.append(sgn[:, 0, :])
    np.testing.assert_array_equal(noise[0], noise[1])   # re and im share e (HE.cu:605-608)
    for w, pos in zip(*np.nonzero(noise[0])):
        r1 = orc.L.orc_splitmix64(0xD6E8FEB86659FD93 ^ int(w * n2 + pos))
        r2 = orc.L.orc_splitmix64(r1)
        u1 = ((r1 >> 11) + 1.0) / 9007199254740992.0
        u2 = ((r2 >> 11) + 1.0) / 9007199254740992.0
        z = 3.2 * np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
        assert abs(abs(z) % 1.0 - 0.5) < 1e-9, (w, pos, z)
    # decrypt on identical inputs is exact
    ev = torch.empty(words, dtype=torch.int64, device="cuda")
    ctx.decrypt_to_eval(cre, sk, ev)
    torch.cuda.synchronize()
    ev_ref = h.decrypt_to_eval(gre, sk_ref)
    np.testing.assert_array_equal(mfhe.to_host_u64(ev), ev_ref)
    return dict(m_re=m_re, m_im=m_im, sk=sk, sk_ref=sk_ref, cre=cre, cim=cim, gre=gre, gim=gim, ore=ore, oim=oim,
                ev_ref=ev_ref)
