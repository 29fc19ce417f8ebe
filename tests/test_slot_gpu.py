"""GPU checks of the CKKS slot encoder (csrc/slot.hip; include/mfhe.h mfhe_slot_reserve, mfhe_slot_encode,
mfhe_slot_decode and the Python layer's slot_reserve / slot_encode / slot_decode) against tests/slot_model.py.

Floating-point bounds are multiples of what plain float64 numpy gives on the same input, both measured from the
longdouble model: encode E_gpu <= 0.5 + 8 E_ref (the 0.5 is the rounding to an integer), decode D_gpu <= 8 D_ref.  The
8 is a margin over a textbook float64 FFT (2.7 to 3.0 times numpy's error at N = 2^10 .. 2^16); each test prints its
figures before it asserts.  Everything that is integer (row consistency, layouts, flags, batch index) is exact."""
import functools

import numpy as np
import pytest

import slot_model as sm
from test_keyswitch_gpu import CLASSES, LAYOUTS, _moduli, _polys

pytestmark = pytest.mark.gpu

LD = sm.LD
ALL_LOGN = list(range(2, 18))


@functools.lru_cache(maxsize=None)
def _ctx(log_n, bits):
    import mfhe
    return mfhe.Context(list(_moduli(log_n, bits)), log_n, mfhe.CONV_PHANTOM)


def _dev_f64(mfhe, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).view(np.float64)).cuda()


def _dev_c128(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda()


def _center_rows(rows, x_model, moduli):
    """rows [R][N] uint64, x_model [N] int64: the integer delta with row r == (x_model + delta) mod q_r on every row
    (asserted equal across the rows), as int64."""
    deltas = []
    for r, q in enumerate(moduli):
        q = int(q)
        want = (x_model.astype(object) % q).astype(np.uint64)
        d = (rows[r].astype(object) - want.astype(object)) % q
        d = np.where(d > (q - 1) // 2, d - q, d)
        deltas.append(np.array(d, dtype=object))
    for r in range(1, len(deltas)):
        assert (deltas[r] == deltas[0]).all(), f"row {r} holds another integer than row 0"
    assert (abs(deltas[0]) < 2 ** 40).all(), "the rows are far from the model"
    return deltas[0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def _encode_case(log_n, npoly=3):
    """z uniform in the unit square, the longdouble coefficients and numpy's float64 ones, unscaled."""
    rng = np.random.default_rng(1000 + log_n)
    n = 1 << (log_n - 1)
    z = rng.random((npoly, n)) + 1j * rng.random((npoly, n))
    c_ld = np.stack([sm.slots_to_coeffs(z[p], log_n) for p in range(npoly)])
    c_64 = np.stack([sm.slots_to_coeffs_f64(z[p], log_n) for p in range(npoly)])
    return z, c_ld, c_64


# ---------------------------------------------------------------------------------------------------------------
# 1. encode against the model
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@pytest.mark.parametrize("log_n", ALL_LOGN)
def test_encode_matches_the_model(mfhe, log_n, bits):
    """Level 2, coefficient form, 3 polynomials, scales 2^30, 2^40, 2^55: both rows hold the same integer x, and
    E_gpu = max |x_k - scale c_k| <= 0.5 + 8 E_ref, E_ref the same for numpy's unrounded float64 coefficients."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    z, c_ld, c_64 = _encode_case(log_n)
    npoly, level = z.shape[0], 2
    dz = _dev_c128(z)
    for e in (30, 40, 55):
        scale = 2.0 ** e
        out = torch.zeros(npoly * level * N, dtype=torch.int64, device="cuda")
        ctx.slot_encode(dz, out, npoly, level, scale, flags=mfhe.SLOT_COEFF)
        torch.cuda.synchronize()
        got = mfhe.to_host_u64(out).reshape(npoly, level, N)
        e_gpu = e_ref = 0.0
        for p in range(npoly):
            target = c_ld[p] * LD(scale)                     # exact: a power of two
            xm = np.rint(target).astype(np.int64)
            delta = _center_rows(got[p], xm, mod[:level])
            e_gpu = max(e_gpu, float(np.abs((xm.astype(LD) - target) + delta.astype(LD)).max()))
            e_ref = max(e_ref, float(np.abs(c_64[p].astype(LD) * LD(scale) - target).max()))
        print(f"encode log_n {log_n} bits {bits} scale 2^{e}: E_gpu - 0.5 = {e_gpu - 0.5:.4g}, E_ref = {e_ref:.4g}, "
              f"relative {max(e_gpu - 0.5, 0) / scale:.3g} vs {e_ref / scale:.3g}")
        assert e_gpu <= 0.5 + 8 * e_ref, (log_n, e, e_gpu, e_ref)


# ---------------------------------------------------------------------------------------------------------------
# 2. layouts and forms
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@pytest.mark.parametrize("log_n", [4, 10, 14])
def test_encode_layouts_flags_and_batch_index(mfhe, log_n, bits):
    """Level 3 + 2 special limbs from limb 5 (a gap above the level); log_n 4 and 10 are the one-workgroup form, 14 the
    two-pass form, whose last pass has its own addresses and its own 16-byte (dense, padded) and 8-byte (padded-odd,
    misaligned) stores.  The dense, padded, padded-odd and misaligned
    layouts give the same bits and write nothing outside their blocks; polynomial 2 repeats polynomial 0 and gets its
    bits, as does a batch of one; the evaluation form is the coefficient form followed by ntt_fwd of the same rows;
    SLOT_REAL is the complex form fed zeros."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    n, level, sp, k, npoly = N // 2, 3, 5, 2, 3
    rows, scale = level + k, 2.0 ** 40
    rng = np.random.default_rng(log_n)
    z = rng.random((npoly, n)) + 1j * rng.random((npoly, n))
    z[2] = z[0]
    ref = {}
    for name, pad, outer, base in LAYOUTS:
        for flags in (mfhe.SLOT_COEFF, 0):
            # slots: N doubles per polynomial, N + pad apart, `base` words into an allocation
            host = np.full(base + npoly * (N + pad) + 2, np.nan)
            for p in range(npoly):
                host[base + p * (N + pad): base + p * (N + pad) + N] = z[p].view(np.float64)
            dz = _dev_f64(mfhe, host)[base:]
            out = _polys(mfhe, npoly, rows, N, pad=pad + outer, base=base)
            ctx.slot_encode(dz, out.t, npoly, level, scale, sp, k, flags, slot_stride=N + pad, out_stride=out.stride)
            torch.cuda.synchronize()
            got = out.blocks((npoly, rows, N))
            out.check_pads()
            np.testing.assert_array_equal(got[2], got[0], err_msg="the bits depend on the batch index")
            if flags in ref:
                np.testing.assert_array_equal(got, ref[flags], err_msg=f"layout {name} changes the bits")
            ref.setdefault(flags, got)
    # rows are residues of one integer, on the limbs of KsGeom's row rule
    limbs = list(range(level)) + list(range(sp, sp + k))
    xm, _ = sm.encode_int(z[1], log_n, scale)
    _center_rows(ref[mfhe.SLOT_COEFF][1], np.array(xm, dtype=np.int64), [mod[l] for l in limbs])
    # a batch of one
    one = torch.zeros(rows * N, dtype=torch.int64, device="cuda")
    ctx.slot_encode(_dev_c128(z[1:2]), one, 1, level, scale, sp, k, mfhe.SLOT_COEFF)
    np.testing.assert_array_equal(mfhe.to_host_u64(one).reshape(rows, N), ref[mfhe.SLOT_COEFF][1])
    # evaluation form == coefficient form, then ntt_fwd of the Q rows and of the special rows
    co = ref[mfhe.SLOT_COEFF]
    dq = mfhe.to_device_u64(np.ascontiguousarray(co[:, :level]).ravel())
    ds = mfhe.to_device_u64(np.ascontiguousarray(co[:, level:]).ravel())
    ctx.ntt_fwd(dq, npoly, 0, level)
    ctx.ntt_fwd(ds, npoly, sp, k)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ref[0][:, :level], mfhe.to_host_u64(dq).reshape(npoly, level, N))
    np.testing.assert_array_equal(ref[0][:, level:], mfhe.to_host_u64(ds).reshape(npoly, k, N))
    # the dense evaluation form with no special rows takes the in-place path: the same bits again
    dn = torch.zeros(npoly * level * N, dtype=torch.int64, device="cuda")
    ctx.slot_encode(_dev_c128(z), dn, npoly, level, scale)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mfhe.to_host_u64(dn).reshape(npoly, level, N), ref[0][:, :level])
    # SLOT_REAL == the complex form with zero imaginary parts
    zr = np.ascontiguousarray(z.real)
    a = torch.zeros(npoly * rows * N, dtype=torch.int64, device="cuda")
    b = torch.zeros_like(a)
    ctx.slot_encode(_dev_f64(mfhe, zr), a, npoly, level, scale, sp, k, mfhe.SLOT_REAL)
    ctx.slot_encode(_dev_c128(zr.astype(np.complex128)), b, npoly, level, scale, sp, k)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mfhe.to_host_u64(a), mfhe.to_host_u64(b))
    assert mfhe.to_host_u64(a).any()


@CLASSES
@pytest.mark.parametrize("log_n", [4, 10, 14])
def test_decode_layouts_and_batch_index(mfhe, log_n, bits):
    """Decode of level-3 polynomials from every layout into canaried slot blocks: the same bits, nothing outside.  At
    log_n 14 pass A's residue loads and pass B's slot stores see the strided and misaligned layouts."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    level, npoly, scale = 3, 3, 2.0 ** 40
    rng = np.random.default_rng(log_n + 50)
    q = np.array(mod[:level], dtype=np.uint64)
    x = rng.integers(0, 2 ** 63, (npoly, level, N), dtype=np.uint64) % q[None, :, None]
    x[2] = x[0]
    ref = None
    for name, pad, outer, base in LAYOUTS:
        src = _polys(mfhe, npoly, level, N, pad=pad, base=base, data=x)
        dst = _polys(mfhe, npoly, 1, N, pad=pad + outer, base=base)
        ctx.slot_decode(src.t, dst.t.view(torch.float64), npoly, level, scale, mfhe.SLOT_COEFF, in_stride=src.stride,
                        slot_stride=dst.stride)
        torch.cuda.synchronize()
        got = dst.blocks((npoly, N))
        dst.check_pads()
        np.testing.assert_array_equal(got[2], got[0], err_msg="the bits depend on the batch index")
        if ref is not None:
            np.testing.assert_array_equal(got, ref, err_msg=f"layout {name} changes the bits")
        ref = got
    assert np.isfinite(ref.view(np.float64)).all() and ref.any()


# (log_n, npoly, log2 of the polynomials a workgroup holds): batches of 512 workgroups and more put 2^lcW polynomials
# into one tile (csrc/slot.hpp slot_geom; tests/test_slot_cpu.py checks these two values of lcW and that batches below
# 512 polynomials run one per workgroup); both end in a tile that is partly empty
BATCHED = [(4, 2050, 2), (6, 4100, 3)]


@CLASSES
@pytest.mark.parametrize("log_n,npoly,lcw", BATCHED)
def test_many_polynomials_per_workgroup(mfhe, log_n, npoly, lcw, bits):
    """The one-workgroup form with several polynomials per tile, the path of a large batch at a small N: encode (both
    domains; 16-byte stores on the dense layout, 8-byte ones on the misaligned one) and decode of the whole batch give
    the bits of the same polynomials done 500 at a time (one per workgroup) and one at a time, write nothing outside
    their blocks, and agree with the model."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    n, level, sp, k, scale = N // 2, 3, 5, 2, 2.0 ** 40
    rows = level + k
    assert npoly % (1 << lcw) and -(-npoly // (1 << lcw)) >= 512
    rng = np.random.default_rng(log_n + 900)
    z = rng.random((npoly, n)) + 1j * rng.random((npoly, n))
    singles = (0, 5, npoly - 1)
    coeff = None
    for flags in (mfhe.SLOT_COEFF, 0):
        ref = np.zeros((npoly, rows, N), dtype=np.uint64)
        for s0 in range(0, npoly, 500):
            m = min(500, npoly - s0)
            part = torch.zeros(m * rows * N, dtype=torch.int64, device="cuda")
            ctx.slot_encode(_dev_c128(z[s0:s0 + m]), part, m, level, scale, sp, k, flags)
            ref[s0:s0 + m] = mfhe.to_host_u64(part).reshape(m, rows, N)
        for p in singles:
            one = torch.zeros(rows * N, dtype=torch.int64, device="cuda")
            ctx.slot_encode(_dev_c128(z[p:p + 1]), one, 1, level, scale, sp, k, flags)
            np.testing.assert_array_equal(mfhe.to_host_u64(one).reshape(rows, N), ref[p])
        for base in (0, 1):          # base 1: rows 8 bytes off a 16-byte boundary
            out = _polys(mfhe, npoly, rows, N, base=base)
            ctx.slot_encode(_dev_c128(z), out.t, npoly, level, scale, sp, k, flags)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.blocks((npoly, rows, N)), ref,
                                          err_msg=f"flags {flags} base {base}: the bits depend on the batch size")
            out.check_pads()
        if flags:
            coeff = ref
    limbs = list(range(level)) + list(range(sp, sp + k))
    for p in singles:
        xm, _ = sm.encode_int(z[p], log_n, scale)
        _center_rows(coeff[p], np.array(xm, dtype=np.int64), [mod[l] for l in limbs])
    # decode of the coefficient rows: the whole batch against 500 at a time, one at a time and the model
    d_rows = mfhe.to_device_u64(coeff.ravel())
    ref = np.zeros((npoly, n), dtype=np.complex128)
    for s0 in range(0, npoly, 500):
        m = min(500, npoly - s0)
        part = torch.zeros(m * n, dtype=torch.complex128, device="cuda")
        ctx.slot_decode(d_rows[s0 * rows * N:], part, m, level, scale, mfhe.SLOT_COEFF, in_stride=rows * N)
        ref[s0:s0 + m] = part.cpu().numpy().reshape(m, n)
    for base in (0, 1):
        dst = _polys(mfhe, npoly, 1, N, base=base)
        ctx.slot_decode(d_rows, dst.t.view(torch.float64), npoly, level, scale, mfhe.SLOT_COEFF, in_stride=rows * N)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dst.blocks((npoly, N)), ref.view(np.uint64), err_msg=f"decode, base {base}")
        dst.check_pads()
    for p in singles:
        one = torch.zeros(n, dtype=torch.complex128, device="cuda")
        ctx.slot_decode(d_rows[p * rows * N:], one, 1, level, scale, mfhe.SLOT_COEFF, in_stride=rows * N)
        np.testing.assert_array_equal(one.cpu().numpy().view(np.uint64), ref[p].view(np.uint64))
        xm, _ = sm.encode_int(z[p], log_n, scale)
        truth = sm.coeffs_to_slots(xm, log_n) / LD(scale)
        d_ref = float(np.abs(sm.coeffs_to_slots_f64(np.array(xm, dtype=np.float64), log_n) / scale - truth).max())
        assert float(np.abs(ref[p].astype(sm.CLD) - truth).max()) <= 8 * d_ref


# ---------------------------------------------------------------------------------------------------------------
# 3. decode against the model on chosen integers
# ---------------------------------------------------------------------------------------------------------------
def _random_centred(rng, bound, count):
    """`count` Python integers uniform in (-bound, bound), as an object array."""
    hi = np.array(rng.integers(0, 2 ** 62, count), dtype=object)
    lo = np.array(rng.integers(0, 2 ** 62, count), dtype=object)
    mid = np.array(rng.integers(0, 2 ** 62, count), dtype=object)
    v = (hi << 124) | (mid << 62) | lo
    return v % (2 * bound - 1) - (bound - 1)


def _to_ld(x):
    """Object array of Python integers below 2^124 in magnitude to longdouble, one rounding."""
    s = np.where(x < 0, -1, 1).astype(LD)
    a = abs(x)
    hi = np.array(a >> 62, dtype=np.uint64).astype(LD)
    lo = np.array(a & ((1 << 62) - 1), dtype=np.uint64).astype(LD)
    return s * (hi * LD(2.0 ** 62) + lo)


def _decode_case(mfhe, ctx, mod, log_n, level, bounds, seed, scale=2.0 ** 40):
    """One polynomial per bound: centred coefficients uniform below it; returns (D_gpu, D_ref) per bound after the
    exact checks of the flags (the evaluation form and SLOT_REAL give the coefficient form's bits)."""
    import torch
    N, n, npoly = 1 << log_n, 1 << (log_n - 1), len(bounds)
    rng = np.random.default_rng(seed)
    xs = [_random_centred(rng, b, N) for b in bounds]
    rows = np.zeros((npoly, level, N), dtype=np.uint64)
    for p, x in enumerate(xs):
        for r in range(level):
            rows[p, r] = np.array(x % int(mod[r]) if r < 2 else rng.integers(0, int(mod[r]), N), dtype=np.uint64)
    d_rows = mfhe.to_device_u64(rows.ravel())
    out = torch.zeros(npoly * n, dtype=torch.complex128, device="cuda")
    ctx.slot_decode(d_rows, out, npoly, level, scale, mfhe.SLOT_COEFF)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(npoly, n)
    # evaluation form: the inverse NTT inside the call undoes ntt_fwd exactly
    d_ev = d_rows.clone()
    ctx.ntt_fwd(d_ev, npoly, 0, level)
    out_ev = torch.zeros_like(out)
    ctx.slot_decode(d_ev, out_ev, npoly, level, scale)
    out_re = torch.zeros(npoly * n, dtype=torch.float64, device="cuda")
    ctx.slot_decode(d_rows, out_re, npoly, level, scale, mfhe.SLOT_COEFF | mfhe.SLOT_REAL)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_ev.cpu().numpy().reshape(npoly, n).view(np.float64), got.view(np.float64))
    np.testing.assert_array_equal(out_re.cpu().numpy().reshape(npoly, n), got.real)
    figs = []
    for p, x in enumerate(xs):
        truth = sm.coeffs_to_slots(_to_ld(x), log_n) / LD(scale)
        ref = sm.coeffs_to_slots_f64(x.astype(np.float64), log_n) / scale
        d_gpu = float(np.abs(got[p].astype(sm.CLD) - truth).max())
        d_ref = float(np.abs(ref.astype(sm.CLD) - truth).max())
        figs.append((d_gpu, d_ref, float(np.abs(truth).max())))
    return figs


def _bounds(mod, level):
    if level == 1:
        q0 = int(mod[0])
        return [2 ** 20, q0 // 2 - (q0 // 2 >> 10)]
    Q = int(mod[0]) * int(mod[1])
    return [2 ** 20, 2 ** 58, Q // 2 - (Q // 2 >> 10)]


@CLASSES
@pytest.mark.parametrize("log_n", ALL_LOGN)
def test_decode_matches_the_model(mfhe, log_n, bits):
    """Level 2: centred coefficients uniform below 2^20, below 2^58 and below (1 - 2^-10) q_0 q_1 / 2.  D_gpu, the
    largest slot error against the longdouble model of the exact integers, is at most 8 D_ref, that of float64 numpy
    fed float(x)."""
    ctx, mod = _ctx(log_n, bits), _moduli(log_n, bits)
    for (d_gpu, d_ref, mag), b in zip(_decode_case(mfhe, ctx, mod, log_n, 2, _bounds(mod, 2), 2000 + log_n),
                                      ("2^20", "2^58", "Q/2")):
        print(f"decode log_n {log_n} bits {bits} |x| < {b}: D_gpu = {d_gpu:.4g}, D_ref = {d_ref:.4g}, "
              f"relative {d_gpu / mag:.3g} vs {d_ref / mag:.3g}")
        assert d_gpu <= 8 * d_ref, (log_n, b, d_gpu, d_ref)


@CLASSES
@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("log_n", [4, 10])
def test_decode_at_level_1_and_3(mfhe, log_n, level, bits):
    """Level 1 reads row 0 alone (coefficients below q_0 / 2); at level 3 the third row is present and ignored."""
    ctx, mod = _ctx(log_n, bits), _moduli(log_n, bits)
    for d_gpu, d_ref, mag in _decode_case(mfhe, ctx, mod, log_n, level, _bounds(mod, level), 3000 + log_n + level):
        print(f"decode log_n {log_n} level {level} bits {bits}: D_gpu = {d_gpu:.4g}, D_ref = {d_ref:.4g}")
        assert d_gpu <= 8 * d_ref, (log_n, level, d_gpu, d_ref)


@CLASSES
@pytest.mark.parametrize("log_n", [4, 10, 14])
def test_decode_of_a_constant_polynomial(mfhe, log_n, bits):
    """x_0 = +-(q_0 q_1 - 1) / 2, +-1 and 0 with every other coefficient 0: every slot is x_0 / scale, with the right
    sign, to within four ulp."""
    import torch
    ctx, mod, N = _ctx(log_n, bits), _moduli(log_n, bits), 1 << log_n
    q0, q1 = int(mod[0]), int(mod[1])
    half = (q0 * q1 - 1) // 2
    x0s = [half, -half, 1, -1, 0]
    rows = np.zeros((len(x0s), 2, N), dtype=np.uint64)
    for p, x0 in enumerate(x0s):
        rows[p, 0, 0], rows[p, 1, 0] = x0 % q0, x0 % q1
        assert sm.garner_lift(x0 % q0, x0 % q1, q0, q1) == x0
    scale = 2.0 ** 40
    out = torch.zeros(len(x0s) * N // 2, dtype=torch.complex128, device="cuda")
    ctx.slot_decode(mfhe.to_device_u64(rows.ravel()), out, len(x0s), 2, scale, mfhe.SLOT_COEFF)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(x0s), N // 2)
    for p, x0 in enumerate(x0s):
        want = float(x0) / scale
        assert np.abs(got[p].real - want).max() <= 4 * np.spacing(abs(want)), (x0, got[p][:2], want)
        assert np.abs(got[p].imag).max() <= 4 * np.spacing(abs(want)), (x0, got[p][:2])
        if x0:
            assert (np.sign(got[p].real) == np.sign(x0)).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. round trip
# ---------------------------------------------------------------------------------------------------------------
@CLASSES
@pytest.mark.parametrize("log_n", [4, 10, 16])
def test_round_trip(mfhe, log_n, bits):
    """decode(encode(z)) differs from z by at most N / (2 scale) (every coefficient off by a half) plus the two
    floating-point terms: 8 E_ref N / scale from the encoder's coefficients (test 1's bound, each coefficient error
    reaching a slot with weight at most 1) and 8 D_ref from the decoder (test 3's)."""
    import torch
    ctx, N = _ctx(log_n, bits), 1 << log_n
    z, c_ld, c_64 = _encode_case(log_n)
    npoly, level, scale = z.shape[0], 2, 2.0 ** 40
    rows = torch.zeros(npoly * level * N, dtype=torch.int64, device="cuda")
    back = torch.zeros(npoly * (N // 2), dtype=torch.complex128, device="cuda")
    ctx.slot_encode(_dev_c128(z), rows, npoly, level, scale)
    ctx.slot_decode(rows, back, npoly, level, scale)
    torch.cuda.synchronize()
    got = back.cpu().numpy().reshape(npoly, N // 2)
    for p in range(npoly):
        e_ref = float(np.abs((c_64[p].astype(LD) - c_ld[p]) * LD(scale)).max())
        xm = np.rint(c_ld[p] * LD(scale))
        truth = sm.coeffs_to_slots(xm, log_n) / LD(scale)
        d_ref = float(np.abs(sm.coeffs_to_slots_f64(xm.astype(np.float64), log_n) / scale - truth).max())
        bound = N / (2 * scale) + 8 * e_ref * N / scale + 8 * d_ref
        err = float(np.abs(got[p] - z[p]).max())
        print(f"round trip log_n {log_n} bits {bits}: error {err:.3g}, bound {bound:.3g}")
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------
# 6. capture
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [10, 14])
def test_graph_capture_after_reserve(mfhe, log_n):
    """After slot_reserve, encode then decode allocate nothing and copy nothing to the device: they are captured on
    one stream and replayed on changed inputs (log_n 14 is the two-pass form with its workspace)."""
    import torch
    bits = (45, 49)
    mod, N = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    npoly, level, sp, k, scale = 2, 3, 5, 2, 2.0 ** 40
    ctx.slot_reserve(npoly, level, sp, k)
    rng = np.random.default_rng(6)
    z = torch.zeros(npoly * N // 2, dtype=torch.complex128, device="cuda")
    rows = torch.zeros(npoly * (level + k) * N, dtype=torch.int64, device="cuda")
    back = torch.zeros_like(z)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.slot_encode(z, rows, npoly, level, scale, sp, k)
        ctx.slot_decode(rows, back, npoly, level, scale, in_stride=(level + k) * N)
    for _ in range(2):
        zh = rng.random(npoly * N // 2) + 1j * rng.random(npoly * N // 2)
        z.copy_(torch.from_numpy(zh))
        g.replay()
        torch.cuda.synchronize()
        replayed = (mfhe.to_host_u64(rows).copy(), back.cpu().numpy().copy())
        e_rows, e_back = torch.zeros_like(rows), torch.zeros_like(back)
        ctx.slot_encode(z, e_rows, npoly, level, scale, sp, k)
        ctx.slot_decode(e_rows, e_back, npoly, level, scale, in_stride=(level + k) * N)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(replayed[0], mfhe.to_host_u64(e_rows))
        np.testing.assert_array_equal(replayed[1].view(np.float64), e_back.cpu().numpy().view(np.float64))
        assert np.abs(replayed[1] - zh).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------
# 7. argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    mod, N = _moduli(4, (45, 49)), 16
    ctx = mfhe.Context(list(mod), 4, mfhe.CONV_PHANTOM)
    h, E = ctx.handle, mfhe.EINVAL
    L = len(mod)
    level, sp, k = 3, 5, 2
    rows = level + k
    res = _polys(mfhe, 2, rows, N)
    slots = _polys(mfhe, 2, 1, N)
    pr, ps = res.t.data_ptr(), slots.t.data_ptr()
    W = rows * N
    inf, nan = float("inf"), float("nan")

    def enc(slots_p=ps, sst=N, scale=2.0 ** 30, out_p=pr, ost=W, npoly=2, level=level, sp=sp, k=k, flags=0):
        return lib.mfhe_slot_encode(h, slots_p, sst, scale, out_p, ost, npoly, level, sp, k, flags, None)

    def dec(in_p=pr, ist=W, scale=2.0 ** 30, slots_p=ps, sst=N, npoly=2, level=level, flags=0):
        return lib.mfhe_slot_decode(h, in_p, ist, scale, slots_p, sst, npoly, level, flags, None)

    bad = [
        enc(slots_p=None), enc(out_p=None), dec(in_p=None), dec(slots_p=None),            # null pointers
        enc(level=0), enc(level=L + 1), dec(level=0), dec(level=L + 1),                   # level outside the context
        enc(k=-1), enc(sp=2), enc(sp=L), enc(sp=6, k=2),                                  # special range
        enc(ost=W - 1), enc(sst=N - 1), dec(ist=2 * N - 1), dec(sst=N - 1),               # strides
        enc(sst=N // 2 - 1, flags=mfhe.SLOT_REAL), dec(sst=N // 2 - 1, flags=mfhe.SLOT_REAL),
        enc(slots_p=pr + 8 * N, ost=W), dec(slots_p=pr + 8, sst=N),                       # input overlapping output
        enc(flags=4), dec(flags=8),                                                       # unknown flags
        enc(scale=0.0), enc(scale=-1.0), enc(scale=inf), enc(scale=nan),                  # scale
        dec(scale=0.0), dec(scale=-2.0), dec(scale=inf), dec(scale=nan),
        lib.mfhe_slot_reserve(h, 2, 0, sp, k), lib.mfhe_slot_reserve(h, 2, level, 2, k),
        lib.mfhe_slot_reserve(None, 2, level, sp, k),
    ]
    assert bad == [E] * len(bad), bad
    torch.cuda.synchronize()
    assert res.all_canary() and slots.all_canary(), "a rejected call wrote something"
    assert enc(npoly=0) == mfhe.OK and dec(npoly=0) == mfhe.OK
    assert enc(npoly=0, k=0, sp=99) == mfhe.OK       # special_start is ignored without special rows
    torch.cuda.synchronize()
    assert res.all_canary() and slots.all_canary(), "npoly == 0 launched something"
    noph = mfhe.Context(list(_moduli(5, (45, 49))), 4, mfhe.CONV_GL)   # q = 1 mod 4N, no phantom tables
    assert lib.mfhe_slot_encode(noph.handle, ps, N, 2.0 ** 30, pr, W, 2, level, sp, k, 0, None) == mfhe.ENOTREADY
    assert lib.mfhe_slot_decode(noph.handle, pr, W, 2.0 ** 30, ps, N, 2, level, 0, None) == mfhe.ENOTREADY
    assert lib.mfhe_slot_reserve(noph.handle, 2, level, sp, k) == mfhe.ENOTREADY
    tiny = mfhe.Context(list(_moduli(4, (45, 49))), 1, mfhe.CONV_PHANTOM)
    assert lib.mfhe_slot_reserve(tiny.handle, 1, 1, 0, 0) == mfhe.EUNSUPPORTED
    with pytest.raises(ValueError):
        ctx.slot_encode(torch.zeros(N, dtype=torch.float32, device="cuda"), res.t, 1, level, 2.0 ** 30)
    with pytest.raises(ValueError):
        ctx.slot_encode(torch.zeros(N // 2 - 1, dtype=torch.complex128, device="cuda"), res.t, 1, level, 2.0 ** 30)
    with pytest.raises(ValueError):
        ctx.slot_decode(res.t, torch.zeros(N // 2, dtype=torch.complex128, device="cuda"), 1, level, 2.0 ** 30,
                        mfhe.SLOT_REAL)


# ---------------------------------------------------------------------------------------------------------------
# 5. the evaluator seen through the slots
# ---------------------------------------------------------------------------------------------------------------
def _fp_terms(z, log_n, scale):
    """What the encoder's and the decoder's floating-point error may add to a slot of the vector z at `scale`, from
    the bounds tests 1 and 3 assert: (N 8 E_ref / scale, 8 D_ref).  E_ref is numpy's float64 coefficient error on z (a
    coefficient error reaches a slot with weight at most 1, N coefficients), D_ref numpy's float64 decode error on the
    rounded coefficients.  Computed on the CPU from the models alone."""
    N = 1 << log_n
    c_ld = sm.slots_to_coeffs(z, log_n)
    e_ref = float(np.abs(sm.slots_to_coeffs_f64(z, log_n).astype(LD) - c_ld).max())        # in units of the scale
    xm = np.rint(c_ld * LD(scale))
    truth = sm.coeffs_to_slots(xm, log_n) / LD(scale)
    d_ref = float(np.abs(sm.coeffs_to_slots_f64(xm.astype(np.float64), log_n) / scale - truth).max())
    return 8 * N * e_ref, 8 * d_ref


class _Scheme:
    """N = 2^10, level 3 + 2 special limbs (limbs 5, 6), alpha 2: a ternary secret, encryption and decryption done
    pointwise in the evaluation domain on the host, keys from the Python layer's generators (|e| <= km.B_E)."""

    def __init__(self, mfhe, bits):
        import ks_model as km
        self.km, self.mfhe = km, mfhe
        self.log_n, self.level, self.key_level, self.alpha, self.sp, self.k = 10, 3, 3, 2, 5, 2
        self.N = 1 << self.log_n
        self.mod = _moduli(self.log_n, bits)
        self.ctx = _ctx(self.log_n, bits)
        self.q, self.p = list(self.mod[:self.level]), list(self.mod[self.sp:self.sp + self.k])
        self.limbs = list(range(self.key_level)) + list(range(self.sp, self.sp + self.k))
        self.rng = np.random.default_rng(55)
        s = self.rng.integers(-1, 2, self.N)
        self.s_ev = self._eval_rows([int(v) for v in s])                  # [5][N] uint64, evaluation domain
        self.s_dev = mfhe.to_device_u64(self.s_ev.ravel())
        self.s2_dev = mfhe.to_device_u64(self._mul(self.s_ev, self.s_ev, self.limbs).ravel())
        self.ks_bound = km.error_bound(self.q, self.p, self.alpha, self.level, self.N, km.B_E)

    def _eval_rows(self, ints):
        """Residues of an integer polynomial on the five key rows, forward-transformed."""
        mfhe, ctx, N = self.mfhe, self.ctx, self.N
        rows = np.array([[v % int(self.mod[l]) for v in ints] for l in self.limbs], dtype=np.uint64)
        dq = ctx.ntt_fwd(mfhe.to_device_u64(rows[:self.key_level].ravel()), 1, 0, self.key_level)
        dp = ctx.ntt_fwd(mfhe.to_device_u64(rows[self.key_level:].ravel()), 1, self.sp, self.k)
        return np.concatenate([mfhe.to_host_u64(dq).reshape(-1, N), mfhe.to_host_u64(dp).reshape(-1, N)])

    def _mul(self, a, b, limbs):
        return np.stack([(a[r].astype(object) * b[r].astype(object) % int(self.mod[l])).astype(np.uint64)
                         for r, l in enumerate(limbs)])

    def encode(self, z, scale):
        import torch
        out = torch.zeros(self.level * self.N, dtype=torch.int64, device="cuda")
        self.ctx.slot_encode(_dev_c128(z), out, 1, self.level, scale)
        return self.mfhe.to_host_u64(out).reshape(self.level, self.N)

    def encrypt(self, pt):
        """(c0, c1) device tensors [level][N] with c0 + c1 s = pt + e, |e| <= B_E, c1 uniform."""
        lv, N, km = self.level, self.N, self.km
        e = self._eval_rows([int(v) for v in self.rng.integers(-km.B_E, km.B_E + 1, N)])[:lv]
        c1 = np.stack([self.rng.integers(0, int(self.mod[r]), N, dtype=np.uint64) for r in range(lv)])
        c1s = self._mul(c1, self.s_ev[:lv], range(lv))
        c0 = np.stack([((pt[r].astype(object) + e[r].astype(object) - c1s[r].astype(object)) % int(self.mod[r]))
                       .astype(np.uint64) for r in range(lv)])
        return self.mfhe.to_device_u64(c0.ravel()), self.mfhe.to_device_u64(c1.ravel())

    def decrypt_decode(self, o0, o1, level, scale, stride_rows=None):
        """Slots of (o0 + o1 s) / scale on rows [0, level) of the outputs ([stride_rows][N] each)."""
        import torch
        mfhe, N = self.mfhe, self.N
        sr = self.level if stride_rows is None else stride_rows
        a, b = mfhe.to_host_u64(o0).reshape(sr, N)[:level], mfhe.to_host_u64(o1).reshape(sr, N)[:level]
        bs = self._mul(b, self.s_ev[:level], range(level))
        m = np.stack([((a[r].astype(object) + bs[r].astype(object)) % int(self.mod[r])).astype(np.uint64)
                      for r in range(level)])
        out = torch.zeros(N // 2, dtype=torch.complex128, device="cuda")
        self.ctx.slot_decode(mfhe.to_device_u64(m.ravel()), out, 1, level, scale)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def galois_key(self, g):
        return self.ctx.gen_galois_key(self.s_dev, g, self.key_level, self.alpha, self.sp, self.k)

    def geom(self):
        return self.level, self.key_level, self.alpha, self.sp, self.k


def _report(what, err, bound):
    print(f"{what}: slot error {err:.3g}, bound {bound:.3g}, ratio {err / bound:.3g}")
    assert err <= bound, (what, err, bound)


@CLASSES
def test_the_evaluator_seen_through_the_slots(mfhe, bits):
    """Rotations, conjugation, a rescaled product and a banded matrix-vector product, each checked on the decoded
    slots.  Every tolerance is N |coefficient error|_inf / scale_out with the coefficient bounds the tree proves
    (ks_model.error_bound, ctmul_model.bound, lt_model.error_bound), the fresh noise B_E and 1/2 per rounded encoding,
    worked out below from the encoded integers' magnitudes, plus the floating-point terms of _fp_terms (each encoding's
    weighted by the largest slot of what it is multiplied with, and the decoder's on the expected result); each is
    asserted below 2^-10 on the CPU before anything runs on the GPU.  A wrong slot order, scale or row mapping gives errors of order 1."""
    import torch
    import ctmul_model as cm
    import ks_model as km
    import lt_model as lm
    log_n, level, key_level, alpha, sp, k = 10, 3, 3, 2, 5, 2          # _Scheme's geometry
    N, n = 1 << log_n, 1 << (log_n - 1)
    mod = _moduli(log_n, bits)
    q, p = list(mod[:level]), list(mod[sp:sp + k])
    ks_bound = km.error_bound(q, p, alpha, level, N, km.B_E)
    rng = np.random.default_rng(5)
    B_E = km.B_E

    def mag(z, scale):   # the largest encoded coefficient, from the model
        return max(abs(v) for v in sm.encode_int(z, log_n, scale)[0])

    # ---- rotations and conjugation: sigma_g(X + e) against sigma_g(C): 1/2 + B_E, plus the key switch ----
    s_rot = 2.0 ** 45
    z = rng.random(n) + 1j * rng.random(n)
    fp_fresh = sum(_fp_terms(z, log_n, s_rot))
    b_rot = N * (0.5 + B_E + ks_bound) / s_rot + fp_fresh
    # ---- product: (X1 + e1)(X2 + e2) against C1 C2, then relinearise and rescale by q_2 ----
    s_mul = 2.0 ** 45
    z1, z2 = rng.random(n) + 1j * rng.random(n), rng.random(n) + 1j * rng.random(n)
    B1, B2 = mag(z1, s_mul), mag(z2, s_mul)
    q2 = q[level - 1]
    msg = N * (B1 * B_E + B2 * B_E + B_E * B_E + (B1 + 0.5) / 2 + (B2 + 0.5) / 2 + 0.25)
    coef_mul = (msg + cm.bound(q, p, alpha, level, N, True)) / q2      # cm.bound is multiplied through by q_2
    s_out = s_mul * s_mul / q2
    fp_mul = (_fp_terms(z1, log_n, s_mul)[0] * np.abs(z2).max() + _fp_terms(z2, log_n, s_mul)[0] * np.abs(z1).max()
              + _fp_terms(z1 * z2, log_n, s_out)[1])
    b_mul = N * coef_mul / s_out + fp_mul
    # ---- banded matrix times vector: sum_t X_t sigma(X_v + e) against sum_t C_t sigma(C_v), then lt_model's bound ----
    s_v, s_pt, n1 = 2.0 ** 45, 2.0 ** 40, 4
    plan = mfhe.bsgs_plan(list(range(8)), n1, log_n)
    diags = rng.uniform(-0.125, 0.125, (8, n))
    v = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    pts_z = np.stack([np.roll(diags[kk], plan["giant_steps"][plan["term_giant"][t]])
                      for t, kk in enumerate(plan["term_step"])])
    B_v, B_pt = mag(v, s_v), max(mag(d, s_pt) for d in pts_z)
    T = len(plan["term_step"])
    msg_lt = T * N * (0.5 * (B_v + B_E) + (B_pt + 0.5) * (0.5 + B_E))
    coef_lt = msg_lt + lm.error_bound(q, p, alpha, level, N, B_E, B_pt, plan)
    j = np.arange(n)
    want_lt = sum(diags[kk] * v[(j + kk) % n] for kk in range(8))
    fp_lt = (_fp_terms(v, log_n, s_v)[0] * np.abs(diags).max(axis=1).sum()
             + sum(_fp_terms(d, log_n, s_pt)[0] for d in pts_z) * np.abs(v).max()
             + _fp_terms(want_lt, log_n, s_v * s_pt)[1])
    b_lt = N * coef_lt / (s_v * s_pt) + fp_lt
    print(f"floating-point terms: fresh {fp_fresh:.3g}, product {fp_mul:.3g}, transform {fp_lt:.3g}")
    for name, b in (("rotation", b_rot), ("product", b_mul), ("transform", b_lt)):
        print(f"bound of the {name}: {b:.3g}")
        assert b < 2.0 ** -10, (name, b)
    # what is decoded fits two limbs: a coefficient is at most the largest slot in magnitude (c_k is a mean of n
    # unit-modulus multiples of the slots, times 2 / N), here with the error bounds on top
    two_limbs = int(q[0]) * int(q[1]) // 2
    assert (np.abs(want_lt).max() + 1) * s_v * s_pt < two_limbs and 3 * s_mul * s_mul < km.prod(q) // 2
    assert 3 * s_out < two_limbs and 3 * s_rot < two_limbs
    # ---- everything above ran on the CPU; from here on the GPU ----
    sc = _Scheme(mfhe, bits)
    ctx = sc.ctx
    assert (sc.log_n, *sc.geom()) == (log_n, level, key_level, alpha, sp, k) and sc.ks_bound == ks_bound

    def fresh():
        return (torch.zeros(level * N, dtype=torch.int64, device="cuda"),
                torch.zeros(level * N, dtype=torch.int64, device="cuda"))

    # rotations and conjugation
    c0, c1 = sc.encrypt(sc.encode(z, s_rot))
    _report("fresh", float(np.abs(sc.decrypt_decode(c0, c1, level, s_rot) - z).max()), N * (0.5 + B_E) / s_rot + fp_fresh)
    for step in (1, 5, n - 1):
        g = mfhe.galois_elt(step, log_n)
        o0, o1 = fresh()
        ctx.galois_apply(c0, c1, sc.galois_key(g), o0, o1, 1, level, key_level, alpha, sp, k, g)
        got = sc.decrypt_decode(o0, o1, level, s_rot)
        _report(f"rotation by {step}", float(np.abs(got - np.roll(z, -step)).max()), b_rot)
    g = mfhe.galois_conj(log_n)
    o0, o1 = fresh()
    ctx.galois_apply(c0, c1, sc.galois_key(g), o0, o1, 1, level, key_level, alpha, sp, k, g)
    _report("conjugation", float(np.abs(sc.decrypt_decode(o0, o1, level, s_rot) - np.conj(z)).max()), b_rot)
    # the rescaled product
    rlk = ctx.gen_switch_key(sc.s2_dev, sc.s_dev, key_level, alpha, sp, k)
    a0, a1 = sc.encrypt(sc.encode(z1, s_mul))
    e0, e1 = sc.encrypt(sc.encode(z2, s_mul))
    o0, o1 = fresh()
    ctx.ctmul(a0, a1, e0, e1, rlk, o0, o1, 1, level, key_level, alpha, sp, k, 1, mfhe.CTMUL_RESCALE)
    got = sc.decrypt_decode(o0, o1, level - 1, s_out)
    _report("rescaled product", float(np.abs(got - z1 * z2).max()), b_mul)
    # the transform: plaintext diagonals encoded straight onto [pt_level + K][N] rows
    rows = level + k
    pt = torch.zeros(T * rows * N, dtype=torch.int64, device="cuda")
    ctx.slot_encode(_dev_f64(mfhe, pts_z), pt, T, level, s_pt, sp, k, mfhe.SLOT_REAL)
    keys = {st: sc.galois_key(mfhe.galois_elt(st, log_n)) for st in plan["key_steps"]}
    keys_b = [None] + [keys[st] for st in plan["baby_steps"][1:]]
    keys_g = [None] + [keys[st] for st in plan["giant_steps"][1:]]
    c0, c1 = sc.encrypt(sc.encode(v, s_v))
    o0, o1 = fresh()
    ctx.lt_apply(c0, c1, pt, o0, o1, 1, level, key_level, alpha, sp, k, plan["baby_elt"], plan["giant_elt"], keys_b,
                 keys_g, plan["term_giant"], plan["term_baby"])
    got = sc.decrypt_decode(o0, o1, level, s_v * s_pt)
    _report("banded matrix times vector", float(np.abs(got - want_lt).max()), b_lt)
    assert np.abs(want_lt).max() > 0.1
