"""The long-double model of the FP64 matrix codec (tests/cdft_model.py) checked on its own, against mpmath, against
the oracle's tables, and used to measure the oracle's float64 error E_ref: the unit of every bound in
test_cdft_gpu.py.  No GPU.  Run with -s to see the figures.

Figures measured on the CPU (x86-64, glibc libm), max-abs:
  model           max |V V^-1 - I|: W axis 1.2e-18; XY 5.0e-20 ... 6.8e-20 at n = 4 ... 128 (bound 2^-58 = 3.5e-18)
  oracle tables   W chain table V 6.0e-13 per entry (a correctly rounded entry: 7.5e-17), its Gauss-Jordan V^-1
                  2.4e-15; XY chain tables 7.4e-16 (n = 4) ... 8.7e-14 (n = 128)
  E_ref           standard-normal input: W forward 2.6e-11 ... 3.0e-11 on outputs of size 1e2, W inverse 3.9e-14 ...
                  4.2e-14 (0.35); XY dft 6.5e-15 (n = 4) ... 5.0e-11 (n = 128), XY idft 2.3e-16 ... 1.7e-15; the rest
                  is printed by test_reference_error_table.  cond(V) = 32.0 on the W axis."""
import numpy as np

import cdft_model as cm
from cdft_model import LD, PHI

TWO58 = 2.0 ** -58
U = 2.0 ** -53
XY_N = (4, 8, 16, 32, 64, 128)
# one chain step of the reference's tables (HE.cu:282-290, encoder.cu:425-444): the root is cos / sin of a double
# angle 2 pi e / m formed with three roundings (error <= 3 u * 2 pi, then one more u from cos / sin), and each
# complex product adds at most 2 sqrt(2) u to an entry of modulus 1: entry r of a chain is off by at most r * CHAIN.
CHAIN = (6 * np.pi + 1 + 2 * np.sqrt(2.0)) * U


def test_model_inverse_accuracy():
    V, Vi = cm.w_table(), cm.w_inverse()
    e = V @ Vi
    e[np.arange(PHI), np.arange(PHI)] -= 1
    w_err = float(np.max(np.abs(e)))
    print(f"\nW axis   max |V V^-1 - I| = {w_err:.3e}  (2^-58 = {TWO58:.3e})")
    assert w_err <= TWO58
    for n in XY_N:
        e = cm.xy_table(n) @ cm.xy_inverse(n) - np.eye(n)
        x_err = float(np.max(np.abs(e)))
        print(f"XY n={n:<4d} max |V V^-1 - I| = {x_err:.3e}")
        assert x_err <= TWO58
    # the exponents are the 512 units of Z_771 / the n residues 1 mod 4 below 4n, each once
    assert sorted(cm.w_exponents()) == [e for e in range(771) if e % 3 and e % 257]
    for n in XY_N:
        assert sorted(cm.xy_exponents(n)) == list(range(1, 4 * n, 4))


def test_model_outputs_against_mpmath():
    """Eight forward and eight inverse W outputs, and eight XY outputs, recomputed at 200 bits.  The inverse does
    not reuse the model's construction: V^-1[r][w] is coefficient r of the Lagrange polynomial
    Phi_771(x) / ((x - x_w) Phi_771'(x_w)), i.e. (sum_(m > r) phi_m x_w^(m - r - 1)) / (sum_m m phi_m x_w^(m - 1)),
    with the sums of roots taken exactly in fixed-point integers."""
    import mpmath as mp
    mp.mp.prec = 200
    FX = 180
    roots = [mp.expjpi(mp.mpf(2 * e) / 771) for e in range(771)]
    fx = [(int(mp.nint(mp.ldexp(z.real, FX))), int(mp.nint(mp.ldexp(z.imag, FX)))) for z in roots]
    fx_re = np.array([a for a, _ in fx], dtype=object)
    fx_im = np.array([b for _, b in fx], dtype=object)

    def from_fx(re, im):
        return mp.mpc(mp.ldexp(mp.mpf(int(re)), -FX), mp.ldexp(mp.mpf(int(im)), -FX))

    def to_mp(z):   # a clongdouble or complex128 scalar, exactly
        parts = []
        for v in (z.real, z.imag):
            m, e = np.frexp(LD(v))
            hi = int(np.ldexp(m, 32))
            lo = int(np.ldexp(np.ldexp(m, 32) - LD(hi), 32))
            parts.append(mp.ldexp(mp.mpf(hi), int(e) - 32) + mp.ldexp(mp.mpf(lo), int(e) - 64))
        return mp.mpc(*parts)

    ew = cm.w_exponents()
    rng = np.random.default_rng(7)
    x = rng.standard_normal((PHI, 8)) + 1j * rng.standard_normal((PHI, 8))
    cols = np.arange(8)
    fwd, inv = cm.wdft_fwd(x, cols), cm.wdft_inv(x, cols)
    picks = [(0, 0), (1, 1), (255, 2), (256, 3), (300, 4), (417, 5), (510, 6), (511, 7)]
    worst = 0.0
    for w, p in picks:
        s = mp.mpc(0)
        for r in range(PHI):
            s += roots[int(ew[w]) * r % 771] * mp.mpc(x[r, p].real, x[r, p].imag)
        terms = float(np.abs(x[:, p]).sum())
        d = float(abs(to_mp(fwd[w, p]) - s))
        print(f"\nW fwd  out[{w}][{p}]  |model - mpmath| = {d:.2e}  bound {TWO58 * terms:.2e}", end="")
        worst = max(worst, d / (TWO58 * terms))
        assert d <= TWO58 * terms
    phi = cm.phi771()
    m_idx = np.array([m for m in range(513) if phi[m]])
    m_cf = np.array([phi[m] for m in m_idx], dtype=object)
    # Phi'(x_w) for every w
    e_d = (ew[:, None] * (m_idx[None, :] - 1)) % 771
    wgt = m_cf * m_idx.astype(object)
    dre, dim = (fx_re[e_d] * wgt).sum(axis=1), (fx_im[e_d] * wgt).sum(axis=1)
    dphi = [from_fx(a, b) for a, b in zip(dre, dim)]
    for r, p in picks:
        sel = m_idx > r
        e_q = (ew[:, None] * (m_idx[sel][None, :] - r - 1)) % 771
        qre, qim = (fx_re[e_q] * m_cf[sel]).sum(axis=1), (fx_im[e_q] * m_cf[sel]).sum(axis=1)
        s, terms = mp.mpc(0), mp.mpf(0)
        for w in range(PHI):
            vi = from_fx(qre[w], qim[w]) / dphi[w]
            y = mp.mpc(x[w, p].real, x[w, p].imag)
            s += vi * y
            terms += abs(vi) * abs(y)
        d = float(abs(to_mp(inv[r, p]) - s))
        print(f"\nW inv  out[{r}][{p}]  |model - mpmath| = {d:.2e}  bound {TWO58 * float(terms):.2e}", end="")
        worst = max(worst, d / (TWO58 * float(terms)))
        assert d <= TWO58 * float(terms)
    # XY at n = 32: four dft and four idft outputs of one lane
    n = 32
    M = cm.xy_input("normal", n, 1, 9)
    g = cm.xy_exponents(n)
    xi = [mp.expjpi(mp.mpf(2 * e) / (4 * n)) for e in range(4 * n)]
    outs = {False: cm.xy_dft(M, n, [0])[0], True: cm.xy_idft(M, n, [0])[0]}
    for inverse, (j, l) in [(False, (0, 0)), (False, (1, 31)), (False, (17, 5)), (False, (31, 30)),
                            (True, (0, 0)), (True, (31, 1)), (True, (5, 17)), (True, (30, 31))]:
        s = mp.mpc(0)
        for y in range(n):
            for xx in range(n):
                if inverse:   # V^-1[j][y] = conj(V[y][j]) / n
                    wgt_ = xi[(-int(g[y]) * j - int(g[xx]) * l) % (4 * n)] / (n * n)
                else:
                    wgt_ = xi[(int(g[j]) * y + int(g[l]) * xx) % (4 * n)]
                s += wgt_ * mp.mpc(M[0, y, xx].real, M[0, y, xx].imag)
        terms = float(np.abs(M[0]).sum()) / (n * n if inverse else 1)
        d = float(abs(to_mp(outs[inverse][j, l]) - s))
        print(f"\nXY {'idft' if inverse else 'dft '} n=32 out[{j}][{l}]  |model - mpmath| = {d:.2e}  bound "
              f"{TWO58 * terms:.2e}", end="")
        worst = max(worst, d / (TWO58 * terms))
        assert d <= TWO58 * terms
    print(f"\nworst |model - mpmath| / (2^-58 sum |terms|) = {worst:.3f}")


def test_model_definitions_against_oracle_tables(orc):
    """The oracle's tables (the reference's chain-of-products construction, in float64) are the model's tables up to
    the chain's drift: the same exponents, the same layout, the same conjugation and scaling."""
    from oracle import P
    V, ViT = np.zeros(PHI * PHI * 2), np.zeros(PHI * PHI * 2)
    assert orc.L.orc_wdft_tables(P(V), P(ViT)) == 0
    V = V.view(np.complex128).reshape(PHI, PHI)
    ViT = ViT.view(np.complex128).reshape(PHI, PHI)      # [w][r] = V^-1[r][w]
    mV, mVi = cm.w_table(), cm.w_inverse()
    dV = cm.err(V, mV)
    rounded = cm.err(mV.astype(np.complex128), mV)
    dVi = cm.err(ViT.T, mVi)
    print(f"\nW chain table V: max |oracle - model| = {dV:.3e} (bound {511 * CHAIN:.3e}); a correctly rounded entry "
          f"differs by {rounded:.3e}")
    assert dV <= 511 * CHAIN
    assert rounded <= 2 * U
    # the oracle's V^-1 inverts its own drifted V: to first order V^-1 dV V^-1, entrywise at most
    # ||V^-1||_inf ||V^-1||_1 max |dV|, and a float64 Gauss-Jordan on a matrix of condition 32 adds far less
    a = np.abs(mVi).astype(np.float64)
    vi_bound = a.sum(axis=1).max() * a.sum(axis=0).max() * 511 * CHAIN
    print(f"W Gauss-Jordan V^-1: max |oracle - model| = {dVi:.3e} (bound {vi_bound:.3e}); cond(V) = "
          f"{np.linalg.cond(mV.astype(np.complex128)):.1f}")
    assert dVi <= vi_bound
    for n in XY_N:
        t = [np.zeros(n * n * 2) for _ in range(4)]
        orc.L.orc_encoder_matrices(n, *[P(x) for x in t])
        eV, eVT, eVi, eViT = (x.view(np.complex128).reshape(n, n) for x in t)
        d = max(cm.err(eV, cm.xy_table(n)), cm.err(eVT.T, cm.xy_table(n)))
        di = max(cm.err(eVi, cm.xy_inverse(n)), cm.err(eViT.T, cm.xy_inverse(n))) * n
        print(f"XY n={n:<4d} chain tables: max |oracle - model| = {d:.3e} (V), {di:.3e} (n V^-1)  bound "
              f"{(n - 1) * CHAIN:.3e}")
        assert d <= (n - 1) * CHAIN and di <= (n - 1) * CHAIN + U


def test_reference_error_table(orc):
    """E_ref: the max-abs error of the oracle's float64 routines against the model, per transform and input class,
    with E_best (numpy complex128 on the model's tables rounded once) beside it."""
    print("\ntransform        class     E_ref      E_best     output scale")
    rows = []
    for n in (8, 64):
        P_ = n * n
        cols = cm.w_check_columns(P_)
        for kind in ("normal", "impulse", "range"):
            x = cm.w_input(kind, P_, 11)
            for inverse in (False, True):
                truth = (cm.wdft_inv if inverse else cm.wdft_fwd)(x, cols)
                e_ref = cm.w_eref(orc, x, cols, inverse, truth)
                e_best = cm.err((cm.wdft_inv_f64 if inverse else cm.wdft_fwd_f64)(x, cols), truth)
                name = f"W {'inv' if inverse else 'fwd'} P={P_}"
                rows.append((name, kind, e_ref, e_best, float(np.max(np.abs(truth)))))
    for n in XY_N:
        lanes = np.arange(5)
        for kind in ("normal", "impulse"):
            M = cm.xy_input(kind, n, 5, 12)
            for inverse in (False, True):
                truth = (cm.xy_idft if inverse else cm.xy_dft)(M, n, lanes)
                e_ref = cm.xy_eref(orc, M, n, lanes, inverse, truth)
                e_best = cm.err((cm.xy_idft_f64 if inverse else cm.xy_dft_f64)(M, n, lanes), truth)
                name = f"XY {'idft' if inverse else 'dft'} n={n}"
                rows.append((name, kind, e_ref, e_best, float(np.max(np.abs(truth)))))
    for name, kind, e_ref, e_best, scale in rows:
        print(f"{name:<16s} {kind:<9s} {e_ref:.2e}   {e_best:.2e}   {scale:.2e}")
        assert np.isfinite(e_ref) and e_best <= 8 * U * 512 * scale
    by = {(r[0], r[1]): r for r in rows}
    # the reference's dense tables drift along their chains, so it is far from the best float64 can do on random
    # input, and exact where an impulse at r = 0 meets only entries equal to 1
    assert by[("W fwd P=4096", "normal")][2] > 10 * by[("W fwd P=4096", "normal")][3]
    x0 = np.zeros((PHI, 1), dtype=np.complex128)
    x0[0, 0] = 1.0
    assert cm.w_eref(orc, x0, [0], False) == 0.0
