"""GPU checks of the RLWE client side (csrc/rlwe.hip) and of the evaluator drivers (mfhe_ctmul, mfhe_ctmat_apply,
mfhe_lt_apply, mfhe_poly_apply) at the launch shapes their own files do not reach:

  1. the client's kernels beyond one workgroup (N = 2^12): a ChaCha block counter above 255;
  2. the mask, public-key and decryption kernels with more than one run of polynomials (grid z > 0), a short last run
     and runs longer than kRlweMinRun;
  3. the small kernel's (set, polynomial) pairs folded over grid y and z, in the one-set and in the three-set form;
  4. the client where the NTT it calls on dense blocks of the workspace runs the pipelined single pass (plan 4) or two
     passes (plan 2), and with the batch cut into chunks;
  5. the evaluator drivers at those plans and chunked.

Every test asserts, before its first GPU call, the geometry that gives it its meaning (ks_row_grid, ks_runs and ks_fold
of csrc/ks_host.hpp restated here, or the effective NTT plan).  Every comparison is exact equality against Python
integers, tests/rlwe_model.py, the CPU oracle's transform, or a composition of public calls that other tests check
against one of those; the two inequalities are proved noise bounds: 21 (2 N + 1) of a public-key encryption
(tests/test_rlwe_gpu.py) and ks_model.error_bound."""
import numpy as np
import pytest

import ks_model as km
import rlwe_model as rm
import test_poly_gpu as tpg
from test_ctmat_gpu import _check_against_separate_products
from test_ctmul_gpu import _check_against_the_composition
from test_keyswitch_gpu import CLASSES
from test_ks_shapes_gpu import (F64_BITS, LAYOUTS, PLANS, PLANS_GALOIS, U64_BITS, _ctx7, _moduli, _plan_ctx, _polys,
                                _prun, _random_rows)
from test_lintrans_gpu import DRIVER_PLAN, _compose
from test_rlwe_gpu import B_NOISE, FIRST_ID, KEY, KW, _dev, _mulmod, _qcol

pytestmark = pytest.mark.gpu

LEVEL, SP, K = 5, 5, 2              # the 5 + 2 limb contexts: the special limbs follow the Q limbs
ROWS = LEVEL + K


# ---------------------------------------------------------------------------------------------------------------
# the launch rules of csrc/ks_host.hpp, the model in batches, the oracle's transform
# ---------------------------------------------------------------------------------------------------------------
def _grid(ncoeff):
    """ks_row_grid: (threads of a block, blocks along x) for ncoeff elements of a row."""
    block = 256 if ncoeff >= 256 else (ncoeff + 63) // 64 * 64
    return block, -(-ncoeff // block)


def _runs(npoly, bx, rows):
    """ks_runs with kRlweMinRun = 4: (prun, runs, polynomials of the last run)."""
    prun = _prun(npoly, bx, rows)
    runs = -(-npoly // prun)
    return prun, runs, npoly - (runs - 1) * prun


def _fold(total):
    """ks_fold: (gy, gz)."""
    gy = min(total, 65535)
    return gy, -(-total // gy)


def _ids(first_id, npoly):
    return [(first_id + p) % (1 << 64) for p in range(npoly)]


def _mask(first_id, npoly, limbs, mod, n):
    """[npoly][len(limbs)][n]: the model's mask residues."""
    return np.stack([rm.mask_residues_ids(KW, l, _ids(first_id, npoly), n, int(mod[l])) for l in limbs], axis=1)


def _small(stream, first_id, npoly, limbs, mod, n):
    """([npoly][len(limbs)][n] coefficient rows, v or q + v; the integers [npoly][n]) of the model."""
    vals = rm.small_values_ids(KW, stream, _ids(first_id, npoly), n)
    q = np.array([int(mod[l]) for l in limbs], dtype=np.int64)[None, :, None]
    v = vals[:, None, :]
    return np.where(v < 0, v + q, v).astype(np.uint64), vals


def _fwd(orc, x, rmod, log_n):
    """The oracle's forward transform of rows x [..][len(rmod)][n]."""
    return orc.phantom_fwd(np.ascontiguousarray(x).ravel(), len(rmod), log_n, list(rmod)).reshape(x.shape)


def _centred_coefficients(orc, x, rmod, log_n):
    """The oracle's inverse transform of rows x [..][len(rmod)][n] (object or uint64), centred per row: int64."""
    u = np.ascontiguousarray(x.astype(np.uint64))
    c = orc.phantom_inv(u.ravel(), len(rmod), log_n, list(rmod)).reshape(u.shape)
    q = np.array([int(v) for v in rmod], dtype=np.uint64)[:, None]
    return np.where(c > q // np.uint64(2), c.astype(np.int64) - q.astype(np.int64), c.astype(np.int64))


def _assert_polys(got, want, what):
    npoly = want.shape[0]
    bad = np.flatnonzero((got != want).reshape(npoly, -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} wrong polynomials of {npoly}, the first {bad[:8].tolist()}"


def _layouts(*names):
    return [l for l in LAYOUTS if l[0] in names]


def _int32(mfhe, vals, cst):
    """The integers [npoly][n] as int32 on the device, cst apart, the gaps filled with 12345."""
    import torch
    npoly, n = vals.shape
    host = np.full((npoly, cst), 12345, dtype=np.int32)
    host[:, :n] = vals
    return torch.from_numpy(host.ravel()).cuda()


def _encrypt_sk_cases(mfhe, ctx, layouts, first_id, s_dev, a, want, msgs, npoly, rows, n, level, sp, k):
    """rlwe_encrypt_sk for every layout and message (None: zero): c1 == a and c0 == want[message given], every
    polynomial compared; pads and inputs untouched.  Yields (c0, c1, message) host arrays for further checks."""
    import torch
    for name, ppad, _, base in layouts:
        for msg in msgs:
            mb = _polys(mfhe, npoly, rows, n, ppad + 2, 0, msg) if msg is not None else None
            c0 = _polys(mfhe, npoly, rows, n, ppad, base)
            c1 = _polys(mfhe, npoly, rows, n, ppad, base)
            ctx.rlwe_encrypt_sk(KEY, first_id, s_dev, mb.t if mb else None, c0.t, c1.t, npoly, level, sp, k,
                                m_stride=mb.stride if mb else None, out_stride=c0.stride)
            torch.cuda.synchronize()
            g0, g1 = c0.blocks((npoly, rows, n)), c1.blocks((npoly, rows, n))
            _assert_polys(g1, a, f"c1 {name} m {msg is not None}")
            _assert_polys(g0, want[msg is not None], f"c0 {name} m {msg is not None}")
            c0.check_pads()
            c1.check_pads()
            if mb:
                np.testing.assert_array_equal(mb.blocks((npoly, rows, n)), msg)
                mb.check_pads()
            yield g0, g1, msg


def _encrypt_pk_cases(mfhe, ctx, layouts, first_id, pk0, pk1, u, e0, e1, msgs, npoly, level, mod, n):
    """rlwe_encrypt_pk for every layout and message against c0 = pk0 u + e0 + m, c1 = pk1 u + e1 in Python integers
    (u, e0, e1 [npoly][level][n] and pk0, pk1 [1][level][n] host rows in the evaluation domain)."""
    import torch
    qc = _qcol(range(level), mod)
    p0, p1, uo = pk0.astype(object), pk1.astype(object), u.astype(object)
    w0 = p0 * uo + e0.astype(object)
    w1 = ((p1 * uo + e1.astype(object)) % qc).astype(np.uint64)
    d0, d1 = _dev(mfhe, pk0), _dev(mfhe, pk1)
    for name, ppad, _, base in layouts:
        for msg in msgs:
            mb = _polys(mfhe, npoly, level, n, ppad + 2, 0, msg) if msg is not None else None
            c0 = _polys(mfhe, npoly, level, n, ppad, base)
            c1 = _polys(mfhe, npoly, level, n, ppad, base)
            ctx.rlwe_encrypt_pk(KEY, first_id, d0, d1, mb.t if mb else None, c0.t, c1.t, npoly, level,
                                m_stride=mb.stride if mb else None, out_stride=c0.stride)
            torch.cuda.synchronize()
            add = msg.astype(object) if msg is not None else 0
            g0, g1 = c0.blocks((npoly, level, n)), c1.blocks((npoly, level, n))
            _assert_polys(g0, ((w0 + add) % qc).astype(np.uint64), f"c0 {name} m {msg is not None}")
            _assert_polys(g1, w1, f"c1 {name} m {msg is not None}")
            c0.check_pads()
            c1.check_pads()
            if mb:
                np.testing.assert_array_equal(mb.blocks((npoly, level, n)), msg)
            yield g0, g1, msg
    np.testing.assert_array_equal(mfhe.to_host_u64(d0), pk0.ravel())
    np.testing.assert_array_equal(mfhe.to_host_u64(d1), pk1.ravel())


def _decrypt_cases(mfhe, ctx, layouts, rng, npoly, rows, mod, n):
    """rlwe_decrypt of random rows against c0 + c1 s in Python integers."""
    import torch
    rmod = list(mod[:rows])
    x0, x1 = _random_rows(rng, (npoly,), rmod, n), _random_rows(rng, (npoly,), rmod, n)
    s = _random_rows(rng, (1,), rmod, n)
    want = ((x0.astype(object) + x1.astype(object) * s.astype(object)) % _qcol(range(rows), mod)).astype(np.uint64)
    d_s = _dev(mfhe, s)
    for name, ppad, _, base in layouts:
        b0 = _polys(mfhe, npoly, rows, n, ppad, base, x0)
        b1 = _polys(mfhe, npoly, rows, n, ppad, base, x1)
        out = _polys(mfhe, npoly, rows, n, ppad + 2, base)
        ctx.rlwe_decrypt(b0.t, b1.t, d_s, out.t, npoly, rows, in_stride=b0.stride, out_stride=out.stride)
        torch.cuda.synchronize()
        _assert_polys(out.blocks((npoly, rows, n)), want, f"decrypt {name}")
        out.check_pads()
        np.testing.assert_array_equal(b0.blocks((npoly, rows, n)), x0, err_msg=name)
        np.testing.assert_array_equal(b1.blocks((npoly, rows, n)), x1, err_msg=name)
        b0.check_pads()
        b1.check_pads()
    np.testing.assert_array_equal(mfhe.to_host_u64(d_s), s.ravel())


# ---------------------------------------------------------------------------------------------------------------
# 1. beyond one workgroup
# ---------------------------------------------------------------------------------------------------------------
BX_LOG_N, BX_NPOLY = 12, 2
BX_LAYOUTS = _layouts("dense", "padded-odd")     # the 16-byte and the scalar stores


def _bx_ctx(bits):
    """The N = 2^12 context after the assertion of its geometry: the mask kernel (four coefficients a thread) has 4
    blocks along x and counters up to 1023, the small kernel (eight a thread) 2 and counters up to 511."""
    n = 1 << BX_LOG_N
    assert _grid(n // 4) == (256, 4) and _grid(n // 8) == (256, 2)
    assert _grid(n) == (256, 16) and _grid(n // 2) == (256, 8)      # the public-key and decryption kernels
    return _ctx7(BX_LOG_N, bits), _moduli(BX_LOG_N, bits), n


@CLASSES
def test_samplers_beyond_one_workgroup(mfhe, orc, bits):
    """sample_uniform against the model; sample_small of a ternary and a noise stream in the coefficient domain
    against the model and transformed against the oracle's transform of the model's rows; lift_small of the same
    integers gives the same rows."""
    import torch
    ctx, mod, n = _bx_ctx(bits)
    npoly, limbs = BX_NPOLY, list(range(ROWS))
    a = _mask(FIRST_ID, npoly, limbs, mod, n)
    small = {}
    for stream in (rm.SECRET, rm.NOISE):
        coef, vals = _small(stream, FIRST_ID, npoly, limbs, mod, n)
        assert 0 < np.abs(vals).max() <= (1 if stream == rm.SECRET else B_NOISE)
        small[stream] = (coef, _fwd(orc, coef, mod, BX_LOG_N), vals)
    for name, ppad, _, base in BX_LAYOUTS:
        out = _polys(mfhe, npoly, ROWS, n, ppad, base)
        ctx.rlwe_sample_uniform(KEY, FIRST_ID, out.t, npoly, LEVEL, SP, K, out_stride=out.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.blocks((npoly, ROWS, n)), a, err_msg=f"uniform {name}")
        out.check_pads()
        for stream, (coef, ev, vals) in small.items():
            ints = _int32(mfhe, vals, n + 3)
            for flags, want in ((mfhe.RLWE_COEFF, coef), (0, ev)):
                msg = f"stream {stream} {name} flags {flags}"
                out = _polys(mfhe, npoly, ROWS, n, ppad, base)
                ctx.rlwe_sample_small(KEY, stream, FIRST_ID, out.t, npoly, LEVEL, SP, K, flags, out_stride=out.stride)
                lifted = _polys(mfhe, npoly, ROWS, n, ppad, base)
                ctx.rlwe_lift_small(ints, lifted.t, npoly, LEVEL, SP, K, flags, coeff_stride=n + 3,
                                    out_stride=lifted.stride)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(out.blocks((npoly, ROWS, n)), want, err_msg="sample_small " + msg)
                np.testing.assert_array_equal(lifted.blocks((npoly, ROWS, n)), want, err_msg="lift_small " + msg)
                out.check_pads()
                lifted.check_pads()


@CLASSES
def test_encrypt_sk_beyond_one_workgroup(mfhe, orc, bits):
    """c1 is the model's mask and c0 = m + e - c1 s in Python integers, with s and e the oracle's transforms of the
    model's ternary and noise rows: nothing of the library enters the expected values."""
    ctx, mod, n = _bx_ctx(bits)
    npoly, limbs = BX_NPOLY, list(range(ROWS))
    s = _fwd(orc, _small(rm.SECRET, 7, 1, limbs, mod, n)[0], mod, BX_LOG_N)
    e = _fwd(orc, _small(rm.NOISE, FIRST_ID, npoly, limbs, mod, n)[0], mod, BX_LOG_N)
    a = _mask(FIRST_ID, npoly, limbs, mod, n)
    m = _random_rows(np.random.default_rng(120 + bits[0]), (npoly,), mod, n)
    qc = _qcol(limbs, mod)
    e_as = e.astype(object) - _mulmod(a, s, limbs, mod)
    want = {True: ((m.astype(object) + e_as) % qc).astype(np.uint64), False: (e_as % qc).astype(np.uint64)}
    s_dev = _dev(mfhe, s)
    for _ in _encrypt_sk_cases(mfhe, ctx, BX_LAYOUTS, FIRST_ID, s_dev, a, want, (m, None), npoly, ROWS, n, LEVEL, SP, K):
        pass
    np.testing.assert_array_equal(mfhe.to_host_u64(s_dev), s.ravel())


@CLASSES
def test_encrypt_pk_and_decrypt_beyond_one_workgroup(mfhe, orc, bits):
    """encrypt_pk against its definition with u, e0, e1 the oracle's transforms of the model's rows (the three-set small
    kernel on 2 blocks along x) and any rows as the public key; decrypt against Python integers."""
    ctx, mod, n = _bx_ctx(bits)
    npoly, limbs = BX_NPOLY, list(range(LEVEL))
    rng = np.random.default_rng(121 + bits[0])
    u, e0, e1 = (_fwd(orc, _small(st, FIRST_ID, npoly, limbs, mod, n)[0], mod[:LEVEL], BX_LOG_N)
                 for st in (rm.EPHEMERAL, rm.NOISE0, rm.NOISE1))
    pk0, pk1 = _random_rows(rng, (1,), mod[:LEVEL], n), _random_rows(rng, (1,), mod[:LEVEL], n)
    m = _random_rows(rng, (npoly,), mod[:LEVEL], n)
    for _ in _encrypt_pk_cases(mfhe, ctx, BX_LAYOUTS, FIRST_ID, pk0, pk1, u, e0, e1, (m, None), npoly, LEVEL, mod, n):
        pass
    _decrypt_cases(mfhe, ctx, BX_LAYOUTS, rng, npoly, LEVEL, mod, n)


# ---------------------------------------------------------------------------------------------------------------
# 2. more than one run of polynomials
# ---------------------------------------------------------------------------------------------------------------
RUN_LOG_N = 4
RUN_LAYOUTS = _layouts("dense", "misaligned")
# (rows, npoly): (prun, runs, polynomials of the last run) from ks_runs with one block along x
RUN_GEOMETRY = {(7, 5): (4, 2, 1), (7, 2341): (5, 469, 1), (7, 3001): (6, 501, 1), (5, 5): (4, 2, 1),
                (5, 3277): (5, 656, 2)}


def _run_ctx(rows, npoly):
    n = 1 << RUN_LOG_N
    assert _grid(n // 4) == (64, 1) and _grid(n) == (64, 1) and _grid(n // 2) == (64, 1), "one block per row"
    assert _runs(npoly, 1, rows) == RUN_GEOMETRY[rows, npoly]
    return _ctx7(RUN_LOG_N, U64_BITS), _moduli(RUN_LOG_N, U64_BITS), n


@pytest.mark.parametrize("npoly", [5, 2341, 3001])
def test_mask_kernel_walks_more_than_one_run(mfhe, orc, npoly):
    """sample_uniform and encrypt_sk (message and zero) at 5 + 2 rows: two runs the last of one polynomial, runs of 5,
    runs of 6 with a last of one.  Every polynomial is compared: a run that starts at the wrong polynomial shows as
    wrong blocks, a short last run or a run past the batch as unwritten blocks or a broken pad."""
    import torch
    ctx, mod, n = _run_ctx(ROWS, npoly)
    limbs = list(range(ROWS))
    a = _mask(FIRST_ID, npoly, limbs, mod, n)
    s = _fwd(orc, _small(rm.SECRET, 7, 1, limbs, mod, n)[0], mod, RUN_LOG_N)
    e = _fwd(orc, _small(rm.NOISE, FIRST_ID, npoly, limbs, mod, n)[0], mod, RUN_LOG_N)
    m = _random_rows(np.random.default_rng(npoly), (npoly,), mod, n)
    qc = _qcol(limbs, mod)
    e_as = e.astype(object) - _mulmod(a, s, limbs, mod)
    want = {True: ((m.astype(object) + e_as) % qc).astype(np.uint64), False: (e_as % qc).astype(np.uint64)}
    for name, ppad, _, base in RUN_LAYOUTS:
        out = _polys(mfhe, npoly, ROWS, n, ppad, base)
        ctx.rlwe_sample_uniform(KEY, FIRST_ID, out.t, npoly, LEVEL, SP, K, out_stride=out.stride)
        torch.cuda.synchronize()
        _assert_polys(out.blocks((npoly, ROWS, n)), a, f"uniform {name}")
        out.check_pads()
    s_dev = _dev(mfhe, s)
    for _ in _encrypt_sk_cases(mfhe, ctx, RUN_LAYOUTS, FIRST_ID, s_dev, a, want, (m, None), npoly, ROWS, n, LEVEL, SP, K):
        pass
    np.testing.assert_array_equal(mfhe.to_host_u64(s_dev), s.ravel())


@pytest.mark.parametrize("npoly", [5, 3277])
def test_public_key_and_decryption_kernels_walk_more_than_one_run(mfhe, orc, npoly):
    """encrypt_pk at level 5 and decrypt at 5 rows: two runs the last of one polynomial; 656 runs of 5 the last of two."""
    ctx, mod, n = _run_ctx(LEVEL, npoly)
    limbs = list(range(LEVEL))
    rng = np.random.default_rng(npoly + 1)
    u, e0, e1 = (_fwd(orc, _small(st, FIRST_ID, npoly, limbs, mod, n)[0], mod[:LEVEL], RUN_LOG_N)
                 for st in (rm.EPHEMERAL, rm.NOISE0, rm.NOISE1))
    pk0, pk1 = _random_rows(rng, (1,), mod[:LEVEL], n), _random_rows(rng, (1,), mod[:LEVEL], n)
    m = _random_rows(rng, (npoly,), mod[:LEVEL], n)
    for _ in _encrypt_pk_cases(mfhe, ctx, RUN_LAYOUTS, FIRST_ID, pk0, pk1, u, e0, e1, (m, None), npoly, LEVEL, mod, n):
        pass
    _decrypt_cases(mfhe, ctx, RUN_LAYOUTS, rng, npoly, LEVEL, mod, n)


# ---------------------------------------------------------------------------------------------------------------
# 3. the small kernel's fold over grid y and z
# ---------------------------------------------------------------------------------------------------------------
FOLD_LOG_N = 3        # the smallest the client accepts: a polynomial of one row is 8 words and one ChaCha block


def _fold_ctx():
    n = 1 << FOLD_LOG_N
    assert _grid(n // 8) == (64, 1)
    return _ctx7(FOLD_LOG_N, U64_BITS), _moduli(FOLD_LOG_N, U64_BITS), n


def test_small_kernel_folds_polynomials_over_grid_y_and_z(mfhe):
    """65538 polynomials of one row: gy = 65535, gz = 2, so polynomials 0, 1, 2 share their blocks with 65535, 65536,
    65537.  sample_small in the coefficient domain against the model, transformed against mfhe_ntt_fwd of the
    coefficient form, and lift_small of the same integers."""
    import torch
    ctx, mod, n = _fold_ctx()
    npoly = 65538
    assert _fold(npoly) == (65535, 2)
    for stream in (rm.SECRET, rm.NOISE):
        coef, vals = _small(stream, FIRST_ID, npoly, [0], mod, n)
        ints = _int32(mfhe, vals, n)
        ev = mfhe.to_host_u64(ctx.ntt_fwd(_dev(mfhe, coef), npoly, 0, 1)).reshape(npoly, 1, n)
        for flags, want in ((mfhe.RLWE_COEFF, coef), (0, ev)):
            out = _polys(mfhe, npoly, 1, n)
            ctx.rlwe_sample_small(KEY, stream, FIRST_ID, out.t, npoly, 1, 0, 0, flags)
            lifted = _polys(mfhe, npoly, 1, n)
            ctx.rlwe_lift_small(ints, lifted.t, npoly, 1, 0, 0, flags)
            torch.cuda.synchronize()
            _assert_polys(out.blocks((npoly, 1, n)), want, f"sample_small stream {stream} flags {flags}")
            _assert_polys(lifted.blocks((npoly, 1, n)), want, f"lift_small stream {stream} flags {flags}")
            out.check_pads()
            lifted.check_pads()


def test_small_kernel_folds_three_sets_over_grid_y_and_z(mfhe):
    """encrypt_pk of 21846 polynomials: 65538 (set, polynomial) pairs, the set boundaries at pair 21846 and 43692 lie
    inside z slab 0 and the slab boundary at pair 65535 inside set 2.  Against the definition with u, e0, e1 from
    sample_small of the three streams (one set each: no fold) and Python integers."""
    import torch
    ctx, mod, n = _fold_ctx()
    npoly = 21846
    assert _fold(3 * npoly) == (65535, 2) and _fold(npoly) == (npoly, 1) and 2 * npoly < 65535 < 3 * npoly
    rng = np.random.default_rng(33)
    draws = []
    for stream in (mfhe.RLWE_EPHEMERAL, mfhe.RLWE_NOISE0, mfhe.RLWE_NOISE1):
        b = _polys(mfhe, npoly, 1, n)
        ctx.rlwe_sample_small(KEY, stream, FIRST_ID, b.t, npoly, 1)
        draws.append(b)
    torch.cuda.synchronize()
    u, e0, e1 = (b.blocks((npoly, 1, n)) for b in draws)
    pk0, pk1 = _random_rows(rng, (1,), mod[:1], n), _random_rows(rng, (1,), mod[:1], n)
    m = _random_rows(rng, (npoly,), mod[:1], n)
    for _ in _encrypt_pk_cases(mfhe, ctx, _layouts("dense", "padded-odd"), FIRST_ID, pk0, pk1, u, e0, e1, (m, None),
                               npoly, 1, mod, n):
        pass


# ---------------------------------------------------------------------------------------------------------------
# 4. the client where the NTT plan changes
# ---------------------------------------------------------------------------------------------------------------
def _client_npoly(n):
    """5 polynomials, after the assertion of what they mean: the mask kernel (N / 1024 blocks along x, 7 rows) and the
    public-key kernel in its 16-byte form (N / 512 blocks, 5 rows) walk two runs, of 4 and of 1."""
    npoly = 5
    bx = _grid(n // 4)[1]
    assert bx == n // 1024 and _grid(n // 8)[1] == n // 2048 and _grid(n // 2)[1] == n // 512
    assert _runs(npoly, bx, ROWS) == (4, 2, 1) and _runs(npoly, n // 512, LEVEL) == (4, 2, 1)
    return npoly


@pytest.mark.parametrize("log_n,bits,plan", PLANS)
def test_sample_small_equals_the_oracle_transform_at_every_plan(mfhe, orc, log_n, bits, plan):
    """A ternary and a noise stream, transformed: the oracle's transform of the model's coefficient rows on the Q rows
    and on the special rows (two dense blocks of the workspace, each its own mfhe_ntt_fwd call)."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    npoly, limbs = _client_npoly(n), list(range(ROWS))
    for stream in (rm.SECRET, rm.NOISE):
        want = _fwd(orc, _small(stream, FIRST_ID, npoly, limbs, mod, n)[0], mod, log_n)
        out = _polys(mfhe, npoly, ROWS, n, 2)
        ctx.rlwe_sample_small(KEY, stream, FIRST_ID, out.t, npoly, LEVEL, SP, K, out_stride=out.stride)
        torch.cuda.synchronize()
        got = out.blocks((npoly, ROWS, n))
        np.testing.assert_array_equal(got[:, :LEVEL], want[:, :LEVEL], err_msg=f"stream {stream}, the Q rows")
        np.testing.assert_array_equal(got[:, LEVEL:], want[:, LEVEL:], err_msg=f"stream {stream}, the special rows")
        out.check_pads()


@pytest.mark.parametrize("log_n,bits,plan", PLANS)
def test_encrypt_sk_is_its_definition_at_every_plan(mfhe, orc, log_n, bits, plan):
    """c1 is the model's mask; c0 = m + e - c1 s with e from sample_small(NOISE) and Python integers.  And without the
    library's transforms: c0 + c1 s - m, formed limb by limb in Python integers and brought to coefficients by the
    oracle, is on every limb the model's noise polynomial, so at most 21."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    npoly, limbs = _client_npoly(n), list(range(ROWS))
    noise = rm.small_values_ids(KW, rm.NOISE, _ids(FIRST_ID, npoly), n)
    assert 0 < np.abs(noise).max() <= B_NOISE
    a = _mask(FIRST_ID, npoly, limbs, mod, n)
    s = _fwd(orc, _small(rm.SECRET, 7, 1, limbs, mod, n)[0], mod, log_n)
    eb = _polys(mfhe, npoly, ROWS, n)
    ctx.rlwe_sample_small(KEY, mfhe.RLWE_NOISE, FIRST_ID, eb.t, npoly, LEVEL, SP, K)
    torch.cuda.synchronize()
    m = _random_rows(np.random.default_rng(log_n + plan), (npoly,), mod, n)
    qc, so = _qcol(limbs, mod), s.astype(object)
    a_s = _mulmod(a, s, limbs, mod)
    e_as = eb.blocks((npoly, ROWS, n)).astype(object) - a_s
    want = {True: ((m.astype(object) + e_as) % qc).astype(np.uint64), False: (e_as % qc).astype(np.uint64)}
    s_dev = _dev(mfhe, s)
    layouts = _layouts("padded")
    for g0, g1, msg in _encrypt_sk_cases(mfhe, ctx, layouts, FIRST_ID, s_dev, a, want, (m, None), npoly, ROWS, n, LEVEL,
                                         SP, K):
        add = msg.astype(object) if msg is not None else 0
        d = (g0.astype(object) + g1.astype(object) * so - add) % qc
        cen = _centred_coefficients(orc, d, mod, log_n)
        assert (cen == noise[:, None, :]).all(), "c0 + c1 s - m is the model's noise on every limb"
        assert np.abs(cen).max() <= B_NOISE


@pytest.mark.parametrize("log_n,bits,plan", PLANS)
def test_encrypt_pk_is_its_definition_at_every_plan(mfhe, orc, log_n, bits, plan):
    """c0 = pk0 u + e0 + m and c1 = pk1 u + e1 with u, e0, e1 from sample_small (3 npoly polynomials through one
    mfhe_ntt_fwd call) and a public key from encrypt_sk; the centred coefficients of c0 + c1 s - m = e_pk u + e0 + e1 s,
    by the oracle's inverse transform, are at most 21 (2 N + 1) and not all zero."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    npoly, limbs = _client_npoly(n), list(range(LEVEL))
    s = _fwd(orc, _small(rm.SECRET, 9, 1, limbs, mod, n)[0], mod[:LEVEL], log_n)
    pk0, pk1 = _polys(mfhe, 1, LEVEL, n), _polys(mfhe, 1, LEVEL, n)
    ctx.rlwe_encrypt_sk(KEY, 5, _dev(mfhe, s), None, pk0.t, pk1.t, 1, LEVEL)
    draws = []
    for stream in (mfhe.RLWE_EPHEMERAL, mfhe.RLWE_NOISE0, mfhe.RLWE_NOISE1):
        b = _polys(mfhe, npoly, LEVEL, n)
        ctx.rlwe_sample_small(KEY, stream, FIRST_ID, b.t, npoly, LEVEL)
        draws.append(b)
    torch.cuda.synchronize()
    u, e0, e1 = (b.blocks((npoly, LEVEL, n)) for b in draws)
    m = _random_rows(np.random.default_rng(log_n + plan + 1), (npoly,), mod[:LEVEL], n)
    qc, so = _qcol(limbs, mod), s.astype(object)
    for g0, g1, msg in _encrypt_pk_cases(mfhe, ctx, _layouts("padded"), FIRST_ID, pk0.blocks((1, LEVEL, n)),
                                         pk1.blocks((1, LEVEL, n)), u, e0, e1, (m, None), npoly, LEVEL, mod, n):
        add = msg.astype(object) if msg is not None else 0
        d = (g0.astype(object) + g1.astype(object) * so - add) % qc
        cen = _centred_coefficients(orc, d, mod[:LEVEL], log_n)
        worst = int(np.abs(cen).max())
        assert worst <= B_NOISE * (2 * n + 1), worst
        assert (cen == cen[:, :1]).all(), "the same small integer on every limb"
        assert worst > 0


def _generated_keys(mfhe, ctx, n, first, g):
    """The three kinds of mfhe_rlwe_ksk_gen at (key_level, alpha, special_start, K) = (5, 2, 5, 2) from secrets 1 (to)
    and 2 (from) of the SECRET stream: ({kind: host key}, s_to, s_other device rows)."""
    import torch
    rows, beta = ROWS, 3
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    s_to, s_other = zeros(rows * n), zeros(rows * n)
    ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, 1, s_to, 1, LEVEL, SP, K)
    ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, 2, s_other, 1, LEVEL, SP, K)
    keys = {}
    for kind, arg in ((mfhe.RLWE_KEY_SWITCH, s_other), (mfhe.RLWE_KEY_RELIN, None), (mfhe.RLWE_KEY_GALOIS, None)):
        out = _polys(mfhe, 1, beta * 2 * rows, n)
        ctx.rlwe_ksk_gen(KEY, first, kind, s_to, out.t, LEVEL, 2, SP, K, s_from=arg, galois_elt=g)
        torch.cuda.synchronize()
        out.check_pads()
        keys[kind] = out
    return keys, s_to, s_other


@pytest.mark.parametrize("log_n,bits,plan", PLANS)
def test_ksk_gen_equals_ksk_assemble_fed_the_samplers_at_every_plan(mfhe, orc, log_n, bits, plan):
    """All three kinds at (key_level, alpha, special_start, K) = (5, 2, 5, 2), three digits the last partial: bit for bit
    mfhe_ksk_assemble of sample_uniform, sample_small(NOISE) and an s_from made outside.  At N = 2^14 in the F64
    class one key switch with the generated switching key: out0 + out1 s_to - c s_from, formed in Python integers and
    brought to coefficients by the oracle, is at most ks_model.error_bound(..., 21) and not 0."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    rows, beta, alpha, limbs = ROWS, 3, 2, list(range(ROWS))
    bx = _grid(n // 4)[1]
    assert _runs(beta, bx, rows) == (3, 1, 3)
    g, first = mfhe.galois_elt(3, log_n), FIRST_ID + LEVEL
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    keys, s_to, s_other = _generated_keys(mfhe, ctx, n, first, g)
    a, e = zeros(beta * rows * n), zeros(beta * rows * n)
    ctx.rlwe_sample_uniform(KEY, first, a, beta, LEVEL, SP, K)
    ctx.rlwe_sample_small(KEY, mfhe.RLWE_NOISE, first, e, beta, LEVEL, SP, K)
    torch.cuda.synchronize()
    sh = mfhe.to_host_u64(s_to).reshape(rows, n)
    s2 = _dev(mfhe, _mulmod(sh, sh, limbs, mod).astype(np.uint64))
    sg = ctx.automorphism(s_to, zeros(rows * n), 1, rows, g)
    for kind, s_from in ((mfhe.RLWE_KEY_SWITCH, s_other), (mfhe.RLWE_KEY_RELIN, s2), (mfhe.RLWE_KEY_GALOIS, sg)):
        want = ctx.ksk_assemble(s_from, s_to, a, e, zeros(beta * 2 * rows * n), LEVEL, alpha, SP, K)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(keys[kind].blocks((beta * 2 * rows * n,)), mfhe.to_host_u64(want),
                                      err_msg=f"kind {kind}")
    if (log_n, bits) != (14, F64_BITS):
        return
    q, p, level = list(mod[:LEVEL]), list(mod[LEVEL:]), LEVEL
    st = _fwd(orc, _small(rm.SECRET, 1, 1, limbs, mod, n)[0], mod, log_n)[0]
    sf = _fwd(orc, _small(rm.SECRET, 2, 1, limbs, mod, n)[0], mod, log_n)[0]
    c = _random_rows(np.random.default_rng(14), (1,), q, n)
    o0, o1 = zeros(level * n), zeros(level * n)
    ctx.keyswitch(_dev(mfhe, c), keys[mfhe.RLWE_KEY_SWITCH].t, o0, o1, 1, level, LEVEL, alpha, SP, K)
    torch.cuda.synchronize()
    h0 = mfhe.to_host_u64(o0).reshape(level, n).astype(object)
    h1 = mfhe.to_host_u64(o1).reshape(level, n).astype(object)
    qcol = np.array(q, dtype=object)[:, None]
    diff = (h0 + h1 * st[:level].astype(object) - c[0].astype(object) * sf[:level].astype(object)) % qcol
    coef = orc.phantom_inv(diff.astype(np.uint64).ravel(), level, log_n, q).reshape(level, n).astype(object)
    Ql = km.prod(q)
    lift = [(Ql // qi) * pow(Ql // qi, -1, qi) for qi in q]
    tot = sum(coef[r] * lift[r] for r in range(level)) % Ql
    err = max(abs(km.centered(int(v), Ql)) for v in tot)
    bound = km.error_bound(q, p, alpha, level, n, B_NOISE)
    print(f"keyswitch with a generated key, N 2^14: error {err}, bound {bound:.2f}")
    assert bound < Ql // 4, "the bound must mean something mod Q_level"
    assert err <= bound
    assert err > 0


def _with_one_polynomial_per_chunk(mfhe, ctx, n, run):
    """run() with the default chunk size and with MFHE_OPT_NTT_CHUNK_BYTES = 8 N (one limb of one polynomial); the
    option is restored, the context is shared."""
    whole = run()
    default = ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES)
    try:
        ctx.set_option(mfhe.OPT_NTT_CHUNK_BYTES, 8 * n)
        chunked = run()
    finally:
        ctx.set_option(mfhe.OPT_NTT_CHUNK_BYTES, default)
    assert ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES) == default
    assert whole.keys() == chunked.keys()
    for name in whole:
        assert whole[name].any(), name
        np.testing.assert_array_equal(whole[name], chunked[name], err_msg=name)


def test_the_client_returns_the_same_bits_with_one_polynomial_per_chunk(mfhe):
    """N = 2^16, U64: encrypt_sk (3 polynomials of 5 + 2 rows), encrypt_pk (9 small polynomials in one batch) and
    ksk_gen (3 digits) with every mfhe_ntt_fwd call of small_to_ws walking its batch one polynomial at a time."""
    import torch
    log_n = 16
    ctx, mod, n = _plan_ctx(mfhe, log_n, U64_BITS, 2)
    npoly = 3
    assert ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES) >= 3 * npoly * ROWS * n * 8, "the default holds every batch in a chunk"
    rng = np.random.default_rng(16)
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")
    s = ctx.rlwe_sample_small(KEY, mfhe.RLWE_SECRET, 1, zeros(ROWS * n), 1, LEVEL, SP, K)
    pk0, pk1 = (_dev(mfhe, _random_rows(rng, (1,), mod[:LEVEL], n)) for _ in range(2))
    m7 = _dev(mfhe, _random_rows(rng, (npoly,), mod, n))
    m5 = _dev(mfhe, _random_rows(rng, (npoly,), mod[:LEVEL], n))

    def run():
        sk = [zeros(npoly * ROWS * n) for _ in range(2)]
        pk = [zeros(npoly * LEVEL * n) for _ in range(2)]
        key = zeros(3 * 2 * ROWS * n)
        ctx.rlwe_encrypt_sk(KEY, FIRST_ID, s, m7, sk[0], sk[1], npoly, LEVEL, SP, K)
        ctx.rlwe_encrypt_pk(KEY, FIRST_ID, pk0, pk1, m5, pk[0], pk[1], npoly, LEVEL)
        ctx.rlwe_ksk_gen(KEY, FIRST_ID, mfhe.RLWE_KEY_RELIN, s, key, LEVEL, 2, SP, K)
        torch.cuda.synchronize()
        names = ("encrypt_sk c0", "encrypt_sk c1", "encrypt_pk c0", "encrypt_pk c1", "ksk_gen")
        return {name: mfhe.to_host_u64(t).copy() for name, t in zip(names, sk + pk + [key])}

    _with_one_polynomial_per_chunk(mfhe, ctx, n, run)


# ---------------------------------------------------------------------------------------------------------------
# 5. the evaluator drivers where the NTT plan changes
# ---------------------------------------------------------------------------------------------------------------
KEY_LEVEL, ALPHA, BETA = 5, 2, 3


def _random_key(mfhe, rng, mod, n):
    return mfhe.to_device_u64(_random_rows(rng, (BETA, 2), mod, n).ravel())


@pytest.mark.parametrize("log_n,bits,plan", PLANS_GALOIS)
def test_ctmul_equals_the_composition_at_every_plan(mfhe, log_n, bits, plan):
    """The check of test_ctmul_equals_the_composition at level 5 of a key at 5 with alpha 2 (a partial last digit):
    ctmul_tensor, keyswitch(KS_ADD) and in-place ntt_moddown; general and square, 1 and 3 terms, with and without
    rescale, the outputs as two padded allocations and as the halves of one.  2 polynomials at N = 2^14, 1 at 2^16."""
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    rng = np.random.default_rng(500 + log_n + plan)
    npoly = 2 if log_n == 14 else 1
    _check_against_the_composition(mfhe, ctx, mod, rng, _random_key(mfhe, rng, mod, n), npoly, 3, LEVEL, KEY_LEVEL,
                                   ALPHA, SP, K)


@pytest.mark.parametrize("log_n,bits,plan", PLANS_GALOIS)
def test_poly_apply_is_its_definition_at_every_plan(mfhe, log_n, bits, plan):
    """A degree-3 plan in each basis at level 5 (depth at most 3): mfhe_poly_apply equals its exported node list run
    through ctmul, ct_lincomb and ntt_moddown.  2 polynomials at N = 2^14, 1 at 2^16."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    rng = np.random.default_rng(510 + log_n + plan)
    npoly = 2 if log_n == 14 else 1
    rlk = _random_key(mfhe, rng, mod, n)
    c0 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:LEVEL], n).ravel())
    c1 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:LEVEL], n).ravel())
    for basis in (mfhe.POLY_MONOMIAL, mfhe.POLY_CHEBYSHEV):
        pl = ctx.poly_plan(tpg._seeded_coeffs(rng, 3), basis, 2.0 ** bits[0], LEVEL)
        info = pl.info()
        assert 1 <= info.depth <= 3 and info.out_level >= 2 and info.nnodes >= 1
        want = tpg._run_by_public_calls(mfhe, ctx, pl, c0, c1, rlk, npoly, KEY_LEVEL, ALPHA, SP, K)
        ol = info.out_level
        o0, o1 = _polys(mfhe, npoly, ol, n, 2), _polys(mfhe, npoly, ol, n, 2)
        ctx.poly_apply(pl, c0, c1, rlk, o0.t, o1.t, npoly, KEY_LEVEL, ALPHA, SP, K, out_stride=o0.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(o0.blocks((npoly, ol, n)), want[0], err_msg=f"out0 basis {basis}")
        np.testing.assert_array_equal(o1.blocks((npoly, ol, n)), want[1], err_msg=f"out1 basis {basis}")
        o0.check_pads()
        o1.check_pads()
        assert want[0].any() and want[1].any()
        pl.close()


@pytest.mark.parametrize("log_n,bits,plan", PLANS[:2])
def test_ctmat_equals_the_separate_products_at_n_2_to_14(mfhe, log_n, bits, plan):
    """The check of test_ctmat_equals_the_separate_products, a 2 x 3 product of 3 terms and 2 polynomials at level 5
    against six calls of ctmul, in both prime classes: the pipelined single pass and two passes."""
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    assert log_n == 14
    rng = np.random.default_rng(520 + plan)
    _check_against_separate_products(mfhe, ctx, mod, rng, _random_key(mfhe, rng, mod, n), 2, 3, 3, 2, LEVEL, KEY_LEVEL,
                                     ALPHA, SP, K, 2)


@pytest.mark.parametrize("log_n,bits,plan", PLANS[:2])
def test_lt_apply_equals_the_composition_at_n_2_to_14(mfhe, log_n, bits, plan):
    """lt_apply on DRIVER_PLAN against test_lintrans_gpu's composition of the public calls: 2 polynomials at level 3 of
    a key made at 5, plaintexts encoded at level 4, padded inputs and outputs."""
    import torch
    ctx, mod, n = _plan_ctx(mfhe, log_n, bits, plan)
    assert log_n == 14
    rng = np.random.default_rng(530 + plan)
    npoly, level, pt_level = 2, 3, 4
    lt = dict(DRIVER_PLAN)
    lt["baby_elt"] = [mfhe.galois_elt(s, log_n) for s in lt["baby_steps"]]
    lt["giant_elt"] = [mfhe.galois_elt(s, log_n) for s in lt["giant_steps"]]
    keys = [_random_key(mfhe, rng, mod, n) for _ in range(3)]
    keys_b, keys_g = [None, keys[0], keys[1]], [None, None, keys[2]]
    ptmod = [mod[l] for l in rm.row_limbs(pt_level, SP, K)]
    pt_h = _random_rows(rng, (5,), ptmod, n)
    c0_h, c1_h = (_random_rows(rng, (npoly,), mod[:level], n) for _ in range(2))
    pt, c0, c1 = (mfhe.to_device_u64(x.ravel()) for x in (pt_h, c0_h, c1_h))
    want = _compose(mfhe, ctx, mod, c0, c1, pt, lt, keys_b, keys_g, npoly, level, KEY_LEVEL, pt_level, ALPHA, SP, K)
    want = [mfhe.to_host_u64(w).reshape(npoly, level, n) for w in want]
    assert want[0].any() and want[1].any()
    b0, b1 = _polys(mfhe, npoly, level, n, 2, 0, c0_h), _polys(mfhe, npoly, level, n, 2, 0, c1_h)
    o0, o1 = _polys(mfhe, npoly, level, n, 4), _polys(mfhe, npoly, level, n, 4)
    ctx.lt_apply(b0.t, b1.t, pt, o0.t, o1.t, npoly, level, KEY_LEVEL, ALPHA, SP, K, lt["baby_elt"], lt["giant_elt"],
                 keys_b, keys_g, lt["term_giant"], lt["term_baby"], pt_level=pt_level, in_stride=b0.stride,
                 out_stride=o0.stride)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(o0.blocks((npoly, level, n)), want[0], err_msg="out0")
    np.testing.assert_array_equal(o1.blocks((npoly, level, n)), want[1], err_msg="out1")
    o0.check_pads()
    o1.check_pads()
    np.testing.assert_array_equal(b0.blocks((npoly, level, n)), c0_h)
    np.testing.assert_array_equal(b1.blocks((npoly, level, n)), c1_h)
    np.testing.assert_array_equal(mfhe.to_host_u64(pt), pt_h.ravel())


def test_the_drivers_return_the_same_bits_with_one_polynomial_per_chunk(mfhe):
    """N = 2^16, U64: ctmul of 3 terms with rescale (the rescale of both outputs one batch) and poly_apply of a degree-3
    Chebyshev plan on 2 polynomials, with every NTT call walking its batch one polynomial at a time."""
    import torch
    log_n = 16
    ctx, mod, n = _plan_ctx(mfhe, log_n, U64_BITS, 2)
    npoly, nt = 2, 3
    assert ctx.get_option(mfhe.OPT_NTT_CHUNK_BYTES) >= 2 * npoly * ROWS * n * 8, "the default holds every batch in a chunk"
    rng = np.random.default_rng(540)
    rlk = _random_key(mfhe, rng, mod, n)
    ops = [mfhe.to_device_u64(_random_rows(rng, (nt, npoly), mod[:LEVEL], n).ravel()) for _ in range(4)]
    pl = ctx.poly_plan(tpg._seeded_coeffs(rng, 3), mfhe.POLY_CHEBYSHEV, 2.0 ** U64_BITS[0], LEVEL)
    ol = pl.info().out_level
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")

    def run():
        both = zeros(2 * npoly * LEVEL * n)
        ctx.ctmul(ops[0], ops[1], ops[2], ops[3], rlk, both[:npoly * LEVEL * n], both[npoly * LEVEL * n:], npoly, LEVEL,
                  KEY_LEVEL, ALPHA, SP, K, nt, mfhe.CTMUL_RESCALE)
        p0, p1 = zeros(npoly * ol * n), zeros(npoly * ol * n)
        ctx.poly_apply(pl, ops[0], ops[1], rlk, p0, p1, npoly, KEY_LEVEL, ALPHA, SP, K)
        torch.cuda.synchronize()
        kept = mfhe.to_host_u64(both).reshape(2, npoly, LEVEL, n)[:, :, :LEVEL - 1].copy()
        return {"ctmul out0": kept[0], "ctmul out1": kept[1], "poly_apply out0": mfhe.to_host_u64(p0).copy(),
                "poly_apply out1": mfhe.to_host_u64(p1).copy()}

    try:
        _with_one_polynomial_per_chunk(mfhe, ctx, n, run)
    finally:
        pl.close()
