"""The FP64 matrix codec (csrc/cdft.hip, csrc/wtrans.hip, the tables of ensure_xy and build_wcrt in csrc/ctx.cpp) held
to the long-double model of tests/cdft_model.py, in every MFHE_OPT_CGEMM_MFMA mode (2: factored W-DFT with Rader
257-point DFTs, 64-point FFTs for XY at n = 64; 3: factored W-DFT on the GEMM, fused XY launch at n = 64; 1: dense
MFMA GEMM; 0: VALU).

The one bound.  E_gpu, the max-abs difference from the model over the checked outputs, must satisfy
    E_gpu <= 4 E_ref + 8 * 2^-53 * S.
E_ref is the error of the oracle's float64 routine (orc_wdft_forward, orc_w_idft, two orc_cmatmul, orc_he_decode) on
the same doubles against the same model, over the same outputs.  S is the largest sum of |table entry| |input|
feeding one checked output (the floor where the reference happens to be exact).  The 4 is a margin for two error
fields of the same size drawn in another summation order; it is not tuned from what the kernels do.

Every test prints E_gpu, E_ref, their ratio and E_gpu / E_best (numpy complex128 on the model's tables rounded once to
double; not asserted) before it asserts, one 'CDFT' line per transform, input class, n and mode."""
import numpy as np
import pytest

import cdft_model as cm
from cdft_model import PHI, Report
from refgeom import lift, residues

pytestmark = pytest.mark.gpu

RNS = [17592186435073, 17182765057, 17184541441]
CONV = 1 | 4   # PHANTOM | WCRT
DELTA = 2.0 ** 35
MODES = (2, 3, 1, 0)


@pytest.fixture(scope="module")
def wctx(mfhe):
    """One W-CRT context per n, two limbs (the FP64 transforms do not depend on the limbs)."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = mfhe.Context(RNS[:2], n.bit_length() - 1, CONV)
        return made[n]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def xctx(mfhe, wctx):
    """Contexts for the XY transforms: the W-CRT ones up to n = 64; n = 128 (n^2 = 2^14 words per lane, beyond the
    W axis geometry the suite builds) with CONV_PHANTOM alone and one 40-bit prime q = 1 mod 2n."""
    from primes import primes_of_size
    made = {}

    def get(n):
        if n <= 64:
            return wctx(n)
        if n not in made:
            made[n] = mfhe.Context(primes_of_size(40, 2 * n, 1), n.bit_length() - 1, mfhe.CONV_PHANTOM)
        return made[n]
    yield get
    for c in made.values():
        c.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.float64).reshape(-1).copy()).cuda()


def _host_c(t):
    return t.cpu().numpy().reshape(-1).view(np.complex128)


def _with_mode(mfhe, ctx, mode):
    ctx.set_option(mfhe.OPT_CGEMM_MFMA, mode)
    assert ctx.get_option(mfhe.OPT_CGEMM_MFMA) == mode


# ------------------------------------------------------------------ W-DFT forward and inverse
def _w_run(mfhe, ctx, x, cols, inverse, full=False):
    """The device transform of all columns of x in every mode; the checked columns (and the whole output)."""
    import torch
    xt = _dev(x)
    idx = torch.from_numpy(cols).cuda()
    got, whole = {}, {}
    for mode in MODES:
        _with_mode(mfhe, ctx, mode)
        o = torch.full_like(xt, float("nan"))
        (ctx.wdft_inv if inverse else ctx.wdft_fwd)(xt, o)
        torch.cuda.synchronize()
        got[mode] = _host_c(o.view(PHI, -1, 2)[:, idx].contiguous()).reshape(PHI, -1)
        if full:
            whole[mode] = o.cpu().numpy()
    _with_mode(mfhe, ctx, 2)
    return got, whole


@pytest.mark.parametrize("kind", ["normal", "impulse", "range"])
@pytest.mark.parametrize("n", [4, 8, 16, 32, 64])
def test_wdft_vs_model(mfhe, orc, wctx, n, kind):
    """W-DFT forward and inverse at P = n^2 = 16 ... 4096 (P = 16 is ragged for the 64-wide MFMA tile and for the
    interleaved columns 2p + a' of the factored forms).  The device transforms all columns; the model checks
    cm.w_check_columns(P).  Input classes: 'normal'; 'impulse' (column p holds a single 1 at row (p + s) mod 512, over
    the shifts s of cm.w_impulse_shifts, so the checked columns hit every row 0 ... 511 and the forward reads every
    column of V, the inverse every column of V^-1; the model's answer to an impulse is the table column itself);
    'range' (rows scaled by 2^(-40 r / 511)).  The inverse is judged against the model's V^-1 and by residual,
    |V_model x_gpu - y| against the same bound with E_ref replaced by the oracle's residual (for impulses at the first
    shift only; the direct form at every shift).  On 'normal' input the other columns keep the cross-mode check."""
    ctx = wctx(n)
    P_ = n * n
    cols = cm.w_check_columns(P_, n)
    rep = Report()
    shifts = cm.w_impulse_shifts(P_, cols) if kind == "impulse" else [0]
    acc = {(inv, m): [0.0, 0.0, 0.0, 0.0] for inv in (False, True) for m in MODES}   # E_gpu, E_ref, E_best, S
    for si, s in enumerate(shifts):
        x = cm.w_input(kind, P_, 100 + n, s)
        for inverse in (False, True):
            if kind == "impulse":
                rows = (cols + s) % PHI
                table = cm.w_inverse() if inverse else cm.w_table()
                truth = table[:, rows]
                scale = np.abs(truth).astype(np.float64)
            else:
                truth = (cm.wdft_inv if inverse else cm.wdft_fwd)(x, cols)
                scale = cm.w_inv_scale(x, cols) if inverse else cm.w_fwd_scale(x, cols)
            e_ref = cm.w_eref(orc, x, cols, inverse, truth)
            e_best = cm.err((cm.wdft_inv_f64 if inverse else cm.wdft_fwd_f64)(x, cols), truth)
            got, whole = _w_run(mfhe, ctx, x, cols, inverse, full=(kind == "normal"))
            for mode in MODES:
                a = acc[inverse, mode]
                a[0] = max(a[0], cm.err(got[mode], truth))
                a[1], a[2], a[3] = max(a[1], e_ref), max(a[2], e_best), max(a[3], float(np.max(scale)))
            if kind == "normal":
                for mode in (2, 3, 1):
                    assert np.max(np.abs(whole[mode] - whole[0])) <= 1e-12 * np.max(np.abs(whole[0])), (mode, inverse)
            if inverse and si == 0:
                V = cm.w_table()
                y = cm._cols(x, cols)
                res_ref = cm.err(V @ cm.orc_wdft(orc, x, cols, True).astype(cm.CLD), y)
                for mode in MODES:
                    xg = got[mode].astype(cm.CLD)
                    res = cm.err(V @ xg, y)
                    rep.line("W inv residual", kind, n, mode, res, res_ref, 0.0, np.abs(xg).sum(axis=0).astype(np.float64),
                             e_ref_name="R_ref")
    for (inverse, mode), (e_gpu, e_ref, e_best, scale) in acc.items():
        rep.line("W inverse" if inverse else "W forward", kind, n, mode, e_gpu, e_ref, e_best, scale)
    if kind == "impulse":
        print(f"CDFT | W impulse shifts at n={n}: {len(shifts)} calls, every row 0 ... 511 hit on a checked column")
    rep.check()


# ------------------------------------------------------------------ XY dft and idft
XY_CASES = [(n, lanes) for n in (4, 8, 16, 32, 64, 128) for lanes in (1, 5)] + [(8, 512), (64, 512)]


@pytest.mark.parametrize("kind", ["normal", "impulse"])
@pytest.mark.parametrize("n,lanes", XY_CASES)
def test_xy_vs_model(mfhe, orc, xctx, n, lanes, kind):
    """XY dft (V M V^T) and idft per lane at n = 4 ... 128 (n = 32 and n = 128 run nowhere else; at n = 128 the MFMA
    kernel has 2 x 2 tiles and 8 K-stages per product), lanes 1 and 5 everywhere and 512 at n = 8 and 64.  The model
    checks the first lane, the last lane and up to 6 random lanes.  'impulse': lane l holds ones at the positions
    p = l mod min(lanes, n^2) of its n x n matrix, so every (row, column) is hit over the lanes used: exactly once
    where lanes <= n^2 (one 1 per lane at 512 lanes and n = 8, eight per lane at n = 64, the whole matrix at 1 lane)."""
    import torch
    ctx = xctx(n)
    if kind == "impulse":
        stride = min(lanes, n * n)
        p = np.arange(n * n)
        M = (p[None, :] % stride == (np.arange(lanes) % stride)[:, None]).astype(np.complex128).reshape(lanes, n, n)
        assert (M.real.sum(axis=0) >= 1).all()
    else:
        M = cm.xy_input("normal", n, lanes, 200 + n)
    check = cm.xy_check_lanes(lanes, n)
    mt = _dev(M)
    rep = Report()
    for inverse in (False, True):
        truth = (cm.xy_idft if inverse else cm.xy_dft)(M, n, check)
        e_ref = cm.xy_eref(orc, M, n, check, inverse, truth)
        e_best = cm.err((cm.xy_idft_f64 if inverse else cm.xy_dft_f64)(M, n, check), truth)
        scale = cm.xy_scale(M, n, check, inverse)
        for mode in MODES:
            _with_mode(mfhe, ctx, mode)
            o = torch.full_like(mt, float("nan"))
            (ctx.xy_idft if inverse else ctx.xy_dft)(mt, o, lanes)
            torch.cuda.synchronize()
            got = _host_c(o).reshape(lanes, n, n)
            assert np.all(np.isfinite(got.view(np.float64)))
            rep.line(f"XY {'idft' if inverse else 'dft'} x{lanes}", kind, n, mode, cm.err(got[check], truth), e_ref, e_best,
                     scale)
    _with_mode(mfhe, ctx, 2)
    rep.check()


# ------------------------------------------------------------------ planar pair entry points
@pytest.mark.parametrize("n", [8, 32])
def test_wdft_pair_vs_model(mfhe, orc, wctx, n):
    """wdft_fwd_pair_i64 / wdft_inv_pair on integers below 2^52 in magnitude (the conversion to double is exact):
    planar equals interleaved bit for bit in the same mode, and both meet the bound against the model."""
    import torch
    ctx = wctx(n)
    P_ = n * n
    rng = np.random.default_rng(300 + n)
    re = rng.integers(-2 ** 52 + 1, 2 ** 52, (PHI, P_), dtype=np.int64)
    im = rng.integers(-2 ** 52 + 1, 2 ** 52, (PHI, P_), dtype=np.int64)
    z = re.astype(np.float64) + 1j * im.astype(np.float64)
    assert np.array_equal(z.real.astype(np.int64), re) and np.array_equal(z.imag.astype(np.int64), im)
    cols = cm.w_check_columns(P_, n)
    truth = cm.wdft_fwd(z, cols)
    e_ref = cm.w_eref(orc, z, cols, False, truth)
    e_best = cm.err(cm.wdft_fwd_f64(z, cols), truth)
    rt, it, zt = torch.from_numpy(re.ravel()).cuda(), torch.from_numpy(im.ravel()).cuda(), _dev(z)
    rep = Report()
    for mode in MODES:
        _with_mode(mfhe, ctx, mode)
        ore = torch.full((PHI * P_,), float("nan"), dtype=torch.float64, device="cuda")
        oim = torch.full_like(ore, float("nan"))
        ctx.wdft_fwd_pair_i64(rt, it, ore, oim)
        inter = torch.full_like(zt, float("nan"))
        ctx.wdft_fwd(zt, inter)
        torch.cuda.synchronize()
        f = _host_c(inter).reshape(PHI, P_)
        np.testing.assert_array_equal(ore.cpu().numpy().reshape(PHI, P_), f.real, err_msg=f"mode {mode}")
        np.testing.assert_array_equal(oim.cpu().numpy().reshape(PHI, P_), f.imag, err_msg=f"mode {mode}")
        rep.line("W fwd pair", "int52", n, mode, cm.err(f[:, cols], truth), e_ref, e_best, cm.w_fwd_scale(z, cols))
        # the inverse of the device's own forward doubles
        bre, bim = torch.full_like(ore, float("nan")), torch.full_like(ore, float("nan"))
        ctx.wdft_inv_pair(ore, oim, bre, bim)
        binter = torch.full_like(zt, float("nan"))
        ctx.wdft_inv(inter, binter)
        torch.cuda.synchronize()
        b = _host_c(binter).reshape(PHI, P_)
        np.testing.assert_array_equal(bre.cpu().numpy().reshape(PHI, P_), b.real, err_msg=f"mode {mode}")
        np.testing.assert_array_equal(bim.cpu().numpy().reshape(PHI, P_), b.imag, err_msg=f"mode {mode}")
        itruth = cm.wdft_inv(f, cols)
        rep.line("W inv pair", "int52", n, mode, cm.err(b[:, cols], itruth), cm.w_eref(orc, f, cols, True, itruth),
                 cm.err(cm.wdft_inv_f64(f, cols), itruth), cm.w_inv_scale(f, cols))
    _with_mode(mfhe, ctx, 2)
    rep.check()


# ------------------------------------------------------------------ the codec: decode, encode, round trip
@pytest.fixture(scope="module")
def codec(mfhe, orc):
    """(ctx, oracle HE) per n on two limbs (44 + 34 bits: every planted or encoded integer here is below 2^62)."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = (mfhe.Context(RNS[:2], n.bit_length() - 1, CONV, DELTA), orc.HE(n, RNS[:2], DELTA))
        return made[n]
    yield get
    for c, _ in made.values():
        c.close()


def _residues(k):
    """[512][n^2] int64 -> matrix-major [512][2][n^2] residues (refgeom.residues: any limb count)."""
    return residues(k, RNS[:2])


def _lift(res, n):
    """Matrix-major residues [512][2][n^2] -> the centred integers (int64), from limb 0 (44 bits), checked on limb 1."""
    return lift(res, n, RNS[:2])


def _decode_eref(orc, h, pre, pim, k_re, k_im, n, lanes):
    """Truth of decode on exact integers, the oracle's E_ref on the same words, E_best and S, over lanes."""
    truth = cm.decode_truth(k_re, k_im, n, DELTA, lanes)
    ref = h.decode(pre, pim).reshape(PHI, n, n)[lanes]
    kc = (k_re.astype(np.float64) + 1j * k_im.astype(np.float64)) / DELTA
    ev = cm._w_tables_f64()[0][lanes] @ kc
    V = cm.xy_table(n).astype(np.complex128)
    best = np.stack([V @ m.reshape(n, n) @ V.T for m in ev])
    return truth, cm.err(ref, truth), cm.err(best, truth), cm.decode_scale(k_re, k_im, DELTA)


@pytest.mark.parametrize("n", [8, 16])
def test_decode_fp_path_vs_model(mfhe, orc, codec, n):
    """Decode's FP path on planted integers: k[r][p] with real and imaginary parts uniform below 2^40, their residues
    formed on the host, ctx.wcrt_fwd (bit-exact elsewhere; its poly-major output is the layout ctx.decode takes), then
    ctx.decode.  Truth is xy_dft(wdft_fwd(k)) / delta from the model on the exact integers; E_ref is the oracle's
    decode of the same words.  The context is a fresh one and decode its first call that needs the pipeline workspace:
    decode_impl once took the workspace's address before allocating it."""
    import torch
    _, h = codec(n)
    ctx = mfhe.Context(RNS[:2], n.bit_length() - 1, CONV, DELTA)
    rng = np.random.default_rng(400 + n)
    k_re = rng.integers(-2 ** 40 + 1, 2 ** 40, (PHI, n * n), dtype=np.int64)
    k_im = rng.integers(-2 ** 40 + 1, 2 ** 40, (PHI, n * n), dtype=np.int64)
    pre = torch.empty(PHI * 2 * n * n, dtype=torch.int64, device="cuda")
    pim = torch.empty_like(pre)
    ctx.wcrt_fwd(mfhe.to_device_u64(_residues(k_re)), pre)
    ctx.wcrt_fwd(mfhe.to_device_u64(_residues(k_im)), pim)
    torch.cuda.synchronize()
    lanes = cm.xy_check_lanes(PHI, n)
    truth, e_ref, e_best, scale = _decode_eref(orc, h, mfhe.to_host_u64(pre), mfhe.to_host_u64(pim), k_re, k_im, n, lanes)
    rep = Report()
    for mode in MODES:
        _with_mode(mfhe, ctx, mode)
        out = torch.full((2 * PHI * n * n,), float("nan"), dtype=torch.float64, device="cuda")
        ctx.decode(pre, pim, out)
        torch.cuda.synchronize()
        got = _host_c(out).reshape(PHI, n, n)
        rep.line("decode", "int40", n, mode, cm.err(got[lanes], truth), e_ref, e_best, scale)
    ctx.close()
    rep.check()


def _planted_message(n, k_bits, seed):
    """c = (k + f) / delta with |k| < 2^k_bits and f in [-0.4, 0.4], and msg = xy_dft(wdft_fwd(c)) by the model over
    all 512 lanes, rounded to double."""
    rng = np.random.default_rng(seed)
    shape = (PHI, n * n)
    k_re, k_im = (rng.integers(-2 ** k_bits + 1, 2 ** k_bits, shape, dtype=np.int64) for _ in range(2))
    f_re, f_im = (rng.uniform(-0.4, 0.4, shape) for _ in range(2))
    c = ((k_re.astype(cm.LD) + f_re.astype(cm.LD)) + 1j * (k_im.astype(cm.LD) + f_im.astype(cm.LD))) / cm.LD(DELTA)
    ev = cm.w_table() @ c.astype(cm.CLD)
    V = cm.xy_table(n)
    msg = np.stack([V @ m.reshape(n, n) @ V.T for m in ev]).astype(np.complex128)
    return k_re, k_im, f_re, f_im, msg


@pytest.mark.parametrize("n", [8, 16])
def test_encode_recovers_planted_integers(mfhe, orc, codec, n):
    """msg = xy_dft(wdft_fwd((k + f) / delta)) by the model, |k| < 2^30, f uniform in [-0.4, 0.4]: ctx.encode rounds
    delta c back to k, so after matrix_to_poly and wcrt_inv every residue on every limb is k mod q_l, in every mode
    (mode 2 runs the planar Rader inverse, which only encode reaches).  CPU precondition, asserted before anything
    runs on the GPU: the oracle's float64 stages on that msg land within 0.025 of k + f, so a device error four times
    the reference's still leaves every value 0.1 - 4 * 0.025 >= 0 away from a tie.  It holds at the full range 2^30."""
    import torch
    ctx, h = codec(n)
    n2 = n * n
    k_bits = 30
    k_re, k_im, f_re, f_im, msg = _planted_message(n, k_bits, 500 + n)
    lanes_all = np.arange(PHI)
    xy = cm.orc_xy(orc, msg, n, lanes_all, True).reshape(PHI, n2)
    wc = cm.orc_wdft(orc, xy, np.arange(n2), True)
    pre_err = max(np.max(np.abs(DELTA * wc.real - (k_re + f_re))), np.max(np.abs(DELTA * wc.imag - (k_im + f_im))))
    print(f"CDFT | encode precondition n={n}: |k| < 2^{k_bits}, oracle max |delta wc - (k + f)| = {pre_err:.3e} (<= 0.025)")
    assert pre_err <= 0.025
    mt = _dev(msg)
    words = PHI * 2 * n2
    want_re, want_im = _residues(k_re), _residues(k_im)
    bad = []
    for mode in MODES:
        _with_mode(mfhe, ctx, mode)
        gre = torch.empty(words, dtype=torch.int64, device="cuda")
        gim = torch.empty_like(gre)
        ctx.encode(mt, gre, gim)
        for g, want, part in ((gre, want_re, "re"), (gim, want_im, "im")):
            poly, back = torch.empty_like(g), torch.empty_like(g)
            ctx.matrix_to_poly(g, poly)
            ctx.wcrt_inv(poly, back)
            torch.cuda.synchronize()
            wrong = int(np.count_nonzero(mfhe.to_host_u64(back) != want))
            print(f"CDFT | encode planted  | {part}      | n={n:<3d} | mode {mode} | wrong residues {wrong} of {words}")
            if wrong:
                bad.append((mode, part, wrong))
    _with_mode(mfhe, ctx, 2)
    assert not bad, bad


@pytest.mark.parametrize("n", [8, 16])
def test_round_trip_derived_bound(mfhe, orc, codec, n):
    """|decode(encode(msg)) - msg| <= 512 n^2 (sqrt(2) / 2) / delta + (4 E_ref + floor of decode on the encoded
    integers): each coefficient's two parts round by at most 1/2 and decode's weights have unit modulus; the rest is
    decode's own error on the integers encode produced (read back through wcrt_inv and lifted).  The round trip is
    taken over all outputs, decode's E_ref over the checked lanes.  The reference's own bound, 1e-3, is printed beside
    it."""
    import torch
    ctx, h = codec(n)
    n2 = n * n
    rng = np.random.default_rng(600 + n)
    msg = 100.0 * (rng.standard_normal(PHI * n2) + 1j * rng.standard_normal(PHI * n2))
    mt = _dev(msg)
    words = PHI * 2 * n2
    lanes = cm.xy_check_lanes(PHI, n)
    quant = PHI * n2 * (np.sqrt(2.0) / 2) / DELTA
    bad = []
    for mode in MODES:
        _with_mode(mfhe, ctx, mode)
        gre = torch.empty(words, dtype=torch.int64, device="cuda")
        gim, pre, pim, cre, cim = (torch.empty_like(gre) for _ in range(5))
        out = torch.full_like(mt, float("nan"))
        ctx.encode(mt, gre, gim)
        ctx.matrix_to_poly(gre, pre)
        ctx.matrix_to_poly(gim, pim)
        ctx.decode(pre, pim, out)
        ctx.wcrt_inv(pre, cre)
        ctx.wcrt_inv(pim, cim)
        torch.cuda.synchronize()
        k_re, k_im = _lift(mfhe.to_host_u64(cre), n), _lift(mfhe.to_host_u64(cim), n)
        truth, e_ref, e_best, scale = _decode_eref(orc, h, mfhe.to_host_u64(pre), mfhe.to_host_u64(pim), k_re, k_im, n,
                                                   lanes)
        got = _host_c(out)
        e_dec = cm.err(got.reshape(PHI, n, n)[lanes], truth)
        e_rt = float(np.max(np.abs(got - msg)))
        bnd = quant + cm.bound(e_ref, scale)
        print(f"CDFT | round trip     | normal  | n={n:<3d} | mode {mode} | |decode(encode(m)) - m| {e_rt:.3e} | bound "
              f"{bnd:.3e} (quantisation {quant:.3e} + decode {cm.bound(e_ref, scale):.3e}) | reference bound 1e-3 | "
              f"decode E_gpu {e_dec:.3e} E_ref {e_ref:.3e}")
        if not e_rt <= bnd:
            bad.append((mode, e_rt, bnd))
    _with_mode(mfhe, ctx, 2)
    assert not bad, bad
