"""GPU checks of the encrypted linear transform (csrc/lintrans.hip; include/mfhe.h mfhe_lt_baby_step, mfhe_lt_pt_mac,
mfhe_lt_reserve, mfhe_lt_apply), bit-exact against Python integers: the formulas computed here, the composition of the
public pieces and the coefficient-domain model of tests/lt_model.py.  Every comparison is exact equality: the
arithmetic is integer (ModDown's one f64 sum only selects the multiple of P; tests/test_lintrans_cpu.py shows the
model's seeded inputs stay 2^-30 P away from where it could flip)."""
import ctypes

import numpy as np
import pytest

import ks_model as km
import lt_model as lm
from primes import primes_of_size
from test_galois_gpu import LAYOUTS, _Blocks, _ctx7, _device_key, _perm_np, _polys
from test_keyswitch_gpu import _inner_product_int, _moduli, _random_rows, _residues, _row_limbs, _u64

pytestmark = pytest.mark.gpu

UNROLL = 8   # csrc/lintrans.hip kLtUnroll: term counts 1 .. 8 have their own instantiation


# ---------------------------------------------------------------------------------------------------------------
# the baby step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 8])
def test_baby_step_bit_exact(mfhe, log_n):
    """u = the gathered inner product + (P mod q_r) c0[pi_g] on component 0 of the Q rows, for g in {5, 25, 3, 2N - 1},
    and the keyless g = 1 form u = ((P mod q_r) c0, (P mod q_r) c1), 0 on the special rows; 1 and 5 polynomials, the four
    layouts (16-byte and scalar form), level 5 and level 3 < key_level 5; pads untouched, inputs unmodified."""
    import torch
    bits = (50, 61)
    ctx, mod, n = _ctx7(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(70 + log_n)
    key_level, alpha, sp, k = 5, 2, 5, 2
    P = km.prod(mod[sp:sp + k])
    kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
    gk = _random_rows(rng, (3, 2), kmod, n)
    d_gk = mfhe.to_device_u64(gk.ravel())
    for level in (5, 3):
        rows, beta = level + k, -(-level // alpha)
        rmod = [mod[l] for l in _row_limbs(level, sp, k)]
        raised = _random_rows(rng, (beta, 5), rmod, n)
        c0 = _random_rows(rng, (5,), mod[:level], n)
        c1 = _random_rows(rng, (5,), mod[:level], n)
        qcol = np.array(mod[:level], dtype=object)[None, :, None]
        pm = np.array([P % q for q in mod[:level]], dtype=object)[None, :, None]
        for g in (5, 25 % (2 * n), 3, 2 * n - 1, None):
            if g is None:   # keyless: u[p][c][r] = (P mod q_r) c_c[p][r], 0 on the special rows
                want = np.zeros((5, 2, rows, n), dtype=np.uint64)
                want[:, 0, :level] = (c0.astype(object) * pm % qcol).astype(np.uint64)
                want[:, 1, :level] = (c1.astype(object) * pm % qcol).astype(np.uint64)
            else:
                pi = _perm_np(log_n, g)
                want = _inner_product_int(raised[..., pi], gk, mod, level, key_level, sp, k)
                add = (want[:, 0, :level].astype(object) + c0[:, :, pi].astype(object) * pm) % qcol
                want[:, 0, :level] = add.astype(np.uint64)
            for npoly in (1, 5):
                for name, ppad, dpad, off in LAYOUTS:
                    msg = f"{name} level {level} g {g} npoly {npoly}"
                    b0 = _polys(mfhe, npoly, level, n, ppad, off, c0[:npoly])
                    bu = _polys(mfhe, npoly, 2 * rows, n, 2 * ppad, off)
                    if g is None:
                        b1 = _polys(mfhe, npoly, level, n, ppad, off, c1[:npoly])
                        ctx.lt_baby_step(b0.t, b1.t, None, bu.t, npoly, level, key_level, alpha, sp, k, 1,
                                         in_stride=b0.stride, u_stride=bu.stride)
                        src1 = c1[:npoly]
                        shape1 = (npoly, level, n)
                    else:
                        pst = rows * n + ppad
                        dst = npoly * pst + dpad
                        src1 = np.ascontiguousarray(raised[:, :npoly])
                        b1 = _Blocks(mfhe, [j * dst + p * pst for j in range(beta) for p in range(npoly)], rows * n,
                                     off, src1)
                        ctx.lt_baby_step(b0.t, b1.t, d_gk, bu.t, npoly, level, key_level, alpha, sp, k, g,
                                         in_stride=b0.stride, digit_stride=dst, poly_stride=pst, u_stride=bu.stride)
                        shape1 = (beta, npoly, rows, n)
                    torch.cuda.synchronize()
                    np.testing.assert_array_equal(bu.blocks((npoly, 2, rows, n)), want[:npoly], err_msg=msg)
                    bu.check_pads()
                    np.testing.assert_array_equal(b0.blocks((npoly, level, n)), c0[:npoly], err_msg=msg)
                    np.testing.assert_array_equal(b1.blocks(shape1), src1, err_msg=msg)
                    b0.check_pads()
                    b1.check_pads()
    np.testing.assert_array_equal(mfhe.to_host_u64(d_gk), gk.ravel())


def test_baby_step_with_key_and_g_1_is_the_plain_inner_product_plus_c0(mfhe):
    """g = 1 with a key: no gather; equals ksk_inner_product with P c0 added."""
    import torch
    bits, log_n = (45, 49), 4
    ctx, mod, n = _ctx7(log_n, bits), _moduli(log_n, bits), 16
    rng = np.random.default_rng(71)
    level, key_level, alpha, sp, k, npoly = 5, 5, 2, 5, 2, 2
    rows = level + k
    P = km.prod(mod[sp:sp + k])
    gk = _random_rows(rng, (3, 2), mod, n)
    raised = _random_rows(rng, (3, npoly), mod, n)
    c0 = _random_rows(rng, (npoly,), mod[:level], n)
    u = torch.zeros(npoly * 2 * rows * n, dtype=torch.int64, device="cuda")
    ctx.lt_baby_step(mfhe.to_device_u64(c0.ravel()), mfhe.to_device_u64(raised.ravel()), mfhe.to_device_u64(gk.ravel()),
                     u, npoly, level, key_level, alpha, sp, k, 1)
    torch.cuda.synchronize()
    want = _inner_product_int(raised, gk, mod, level, key_level, sp, k)
    qcol = np.array(mod[:level], dtype=object)[None, :, None]
    pm = np.array([P % q for q in mod[:level]], dtype=object)[None, :, None]
    want[:, 0, :level] = ((want[:, 0, :level].astype(object) + c0.astype(object) * pm) % qcol).astype(np.uint64)
    np.testing.assert_array_equal(mfhe.to_host_u64(u).reshape(npoly, 2, rows, n), want)


# ---------------------------------------------------------------------------------------------------------------
# the plaintext multiply-accumulate
# ---------------------------------------------------------------------------------------------------------------
MAC_N, MAC_LEVEL, MAC_PT_LEVEL, MAC_K = 256, 3, 4, 2
# 1, every unrolled count, unroll + 1, and the fold boundaries of the lazy u128 sum
MAC_TERMS = list(range(1, UNROLL + 2)) + [16, 17, 32, 33, 64]


@pytest.fixture(scope="module")
def mac_ctx(mfhe):
    """Primes of 62 bits: 4 Q limbs (the plaintexts are encoded at pt_level 4, the sums run at level 3) and 2 special."""
    mod = primes_of_size(62, 2 * MAC_N, MAC_PT_LEVEL + MAC_K)
    assert all(q >> 61 for q in mod)
    return mfhe.Context(mod, 8, mfhe.CONV_PHANTOM), mod


def _mac_int(u, pt, term_u, term_pt, mod, level, pt_level, sp, k):
    """acc [npoly][2][rows][N] from u [nslots][npoly][2][rows][N] and pt [npt][pt_level + K][N], in Python integers."""
    _, npoly, _, rows, n = u.shape
    out = np.zeros((npoly, 2, rows, n), dtype=np.uint64)
    for r, limb in enumerate(_row_limbs(level, sp, k)):
        pr = r if r < level else pt_level + r - level
        acc = np.zeros((npoly, 2, n), dtype=object)
        for tu, tp in zip(term_u, term_pt):
            acc = acc + u[tu, :, :, r, :].astype(object) * pt[tp, pr, :].astype(object)[None, None, :]
        out[:, :, r, :] = (acc % int(mod[limb])).astype(np.uint64)
    return out


def _run_mac(mfhe, ctx, u, pt, term_u, term_pt, npoly, layout):
    """The device sum on the first npoly polynomials of u in the given layout: (acc blocks, the buffers)."""
    import torch
    name, ppad, dpad, off = layout
    level, ptl, k, n = MAC_LEVEL, MAC_PT_LEVEL, MAC_K, MAC_N
    rows, nslots, npt = level + k, u.shape[0], pt.shape[0]
    pst = 2 * rows * n + ppad
    sst = npoly * pst + dpad
    src = np.ascontiguousarray(u[:, :npoly])
    bu = _Blocks(mfhe, [s * sst + p * pst for s in range(nslots) for p in range(npoly)], 2 * rows * n, off, src)
    bp = _polys(mfhe, npt, ptl + k, n, ppad, 0, pt)
    ba = _polys(mfhe, npoly, 2 * rows, n, ppad, off)
    ctx.lt_pt_mac(bu.t, bp.t, ba.t, term_u, term_pt, npoly, level, ptl, k, nslots, npt, pt_level=ptl, slot_stride=sst,
                  poly_stride=pst, pt_stride=bp.stride, acc_stride=ba.stride)
    torch.cuda.synchronize()
    ba.check_pads()
    np.testing.assert_array_equal(bu.blocks(src.shape), src, err_msg=f"{name}: u modified")
    np.testing.assert_array_equal(bp.blocks(pt.shape), pt, err_msg=f"{name}: pt modified")
    bu.check_pads()
    bp.check_pads()
    return ba.blocks((npoly, 2, rows, n))


def test_pt_mac_of_all_q_minus_1(mfhe, mac_ctx):
    """Both operands q - 1 everywhere with 62-bit primes, the worst case of the lazy u128 sum: (q - 1)^2 = 1 mod q, so
    the sum of nterms products is nterms.  17, 33 and 64 terms overflow a u128 unless the sum folds every 16."""
    ctx, mod = mac_ctx
    level, ptl, k, n = MAC_LEVEL, MAC_PT_LEVEL, MAC_K, MAC_N
    rows = level + k
    top_u = _u64([mod[l] for l in _row_limbs(level, ptl, k)]) - np.uint64(1)
    top_p = _u64(mod) - np.uint64(1)
    u = np.broadcast_to(top_u[None, None, None, :, None], (2, 5, 2, rows, n)).copy()
    pt = np.broadcast_to(top_p[None, :, None], (2, ptl + k, n)).copy()
    for nt in MAC_TERMS:
        term_u, term_pt = [t % 2 for t in range(nt)], [(t // 2) % 2 for t in range(nt)]
        for npoly in (1, 5):
            for layout in (LAYOUTS if nt in (1, UNROLL, UNROLL + 1, 17, 64) else (LAYOUTS[0], LAYOUTS[3])):
                got = _run_mac(mfhe, ctx, u, pt, term_u, term_pt, npoly, layout)
                assert (got == np.uint64(nt)).all(), f"{layout[0]} nterms {nt} npoly {npoly}"


def test_pt_mac_bit_exact(mfhe, mac_ctx):
    """Random canonical operands, 3 slots and 4 plaintexts with repeats among the terms, pt_level 4 > level 3 (the
    special rows of a plaintext sit at rows 4 and 5), every term count of MAC_TERMS, 1 and 5 polynomials, four layouts."""
    ctx, mod = mac_ctx
    level, ptl, k, n = MAC_LEVEL, MAC_PT_LEVEL, MAC_K, MAC_N
    rng = np.random.default_rng(72)
    rmod = [mod[l] for l in _row_limbs(level, ptl, k)]
    u = _random_rows(rng, (3, 5, 2), rmod, n)
    pt = _random_rows(rng, (4,), mod, n)
    for nt in MAC_TERMS:
        term_u = [(2 * t + t // 3) % 3 for t in range(nt)]
        term_pt = [(3 * t + t // 4) % 4 for t in range(nt)]
        want = _mac_int(u, pt, term_u, term_pt, mod, level, ptl, ptl, k)
        for npoly in (1, 5):
            for layout in (LAYOUTS if nt in (1, 3, UNROLL, UNROLL + 1, 33) else (LAYOUTS[0], LAYOUTS[3])):
                got = _run_mac(mfhe, ctx, u, pt, term_u, term_pt, npoly, layout)
                np.testing.assert_array_equal(got, want[:npoly], err_msg=f"{layout[0]} nterms {nt} npoly {npoly}")


def test_pt_mac_long_runs_with_a_one_pair_tail(mfhe, mac_ctx):
    """1643 polynomials = 3286 (polynomial, component) pairs at N = 256 and 5 rows: the 4096-workgroup rule makes runs
    of 5 pairs (longer than the minimum of 4), 657 of them and a last run of one pair.  The polynomials repeat with
    period 7, which no run length divides, so a pair read or written at the wrong place shows."""
    ctx, mod = mac_ctx
    level, ptl, k, n, npoly = MAC_LEVEL, MAC_PT_LEVEL, MAC_K, MAC_N, 1643
    rng = np.random.default_rng(73)
    rmod = [mod[l] for l in _row_limbs(level, ptl, k)]
    u7 = _random_rows(rng, (2, 7, 2), rmod, n)
    pt = _random_rows(rng, (2,), mod, n)
    term_u, term_pt = [0, 1, 1], [1, 0, 1]
    want7 = _mac_int(u7, pt, term_u, term_pt, mod, level, ptl, ptl, k)
    idx = np.arange(npoly) % 7
    u = np.ascontiguousarray(u7[:, idx])
    for layout in (LAYOUTS[0], LAYOUTS[3]):
        got = _run_mac(mfhe, ctx, u, pt, term_u, term_pt, npoly, layout)
        np.testing.assert_array_equal(got, want7[idx], err_msg=layout[0])


# ---------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------
def _add_mod(torch, acc, x, qrow):
    s = acc + x
    return torch.where(s >= qrow, s - qrow, s)


def _compose(mfhe, ctx, mod, c0, c1, pt, plan, keys_b, keys_g, npoly, level, key_level, pt_level, alpha, sp, k):
    """lt_apply as the composition of the public calls and torch additions mod q: (out0, out1) device tensors."""
    import torch
    n, rows = ctx.N, level + k
    beta = -(-level // alpha)
    pw, lw = rows * n, level * n
    nb = len(plan["baby_elt"])
    raised = torch.zeros(beta * npoly * pw, dtype=torch.int64, device="cuda")
    ctx.keyswitch_raise(c1, raised, npoly, level, alpha, sp, k)
    U = torch.zeros(nb * npoly * 2 * pw, dtype=torch.int64, device="cuda")
    slot = npoly * 2 * pw
    ctx.lt_baby_step(c0, c1, None, U[:slot], npoly, level, key_level, alpha, sp, k, 1)
    for b in range(1, nb):
        if keys_b[b] is not None:
            ctx.lt_baby_step(c0, raised, keys_b[b], U[b * slot:(b + 1) * slot], npoly, level, key_level, alpha, sp, k,
                             plan["baby_elt"][b])
    qrow = torch.tensor(np.array(mod[:level], dtype=np.int64), device="cuda").reshape(1, level, 1)
    outs = [torch.zeros((npoly, level, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    for a in sorted(set(plan["term_giant"])):
        ts = [t for t, ta in enumerate(plan["term_giant"]) if ta == a]
        A = torch.zeros(npoly * 2 * pw, dtype=torch.int64, device="cuda")
        ctx.lt_pt_mac(U, pt, A, [plan["term_baby"][t] for t in ts], ts, npoly, level, sp, k, nb,
                      len(plan["term_giant"]), pt_level=pt_level)
        w = []
        for c in range(2):
            down = torch.zeros(npoly * lw, dtype=torch.int64, device="cuda")
            ctx.ntt_moddown(A[c * pw:], down, npoly, level, sp, k, in_stride=2 * pw)
            w.append(down)
        if a != 0:
            r0, r1 = torch.zeros_like(w[0]), torch.zeros_like(w[1])
            ctx.galois_apply(w[0], w[1], keys_g[a], r0, r1, npoly, level, key_level, alpha, sp, k,
                             plan["giant_elt"][a])
            w = [r0, r1]
        torch.cuda.synchronize()
        outs = [_add_mod(torch, o, x.reshape(npoly, level, n), qrow) for o, x in zip(outs, w)]
    return outs


# three baby and three giant steps; giant step 1 has no terms; baby step 1 is used by giant step 0 only
DRIVER_PLAN = {"baby_steps": [0, 1, 2], "giant_steps": [0, 3, 6],
               "term_giant": [0, 0, 0, 2, 2], "term_baby": [0, 1, 2, 0, 2]}


@pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("log_n", [4, 10])
def test_lt_apply_equals_the_composition(mfhe, log_n, bits):
    """npoly 3, level 3 of a key made at 5, plaintexts encoded at level 4, dense and padded outputs.  The keys are
    random residues: the comparison is between two ways of running the same kernels' arithmetic."""
    import torch
    ctx, mod, n = _ctx7(log_n, bits), _moduli(log_n, bits), 1 << log_n
    rng = np.random.default_rng(80 + log_n)
    npoly, level, key_level, pt_level, alpha, sp, k = 3, 3, 5, 4, 2, 5, 2
    plan = dict(DRIVER_PLAN)
    plan["baby_elt"] = [mfhe.galois_elt(s, log_n) for s in plan["baby_steps"]]
    plan["giant_elt"] = [mfhe.galois_elt(s, log_n) for s in plan["giant_steps"]]
    kmod = [mod[l] for l in _row_limbs(key_level, sp, k)]
    keys = [mfhe.to_device_u64(_random_rows(rng, (3, 2), kmod, n).ravel()) for _ in range(3)]
    keys_b, keys_g = [None, keys[0], keys[1]], [None, None, keys[2]]
    ptmod = [mod[l] for l in _row_limbs(pt_level, sp, k)]
    pt_h = _random_rows(rng, (5,), ptmod, n)
    c0_h = _random_rows(rng, (npoly,), mod[:level], n)
    c1_h = _random_rows(rng, (npoly,), mod[:level], n)
    pt, c0, c1 = (mfhe.to_device_u64(x.ravel()) for x in (pt_h, c0_h, c1_h))
    want = _compose(mfhe, ctx, mod, c0, c1, pt, plan, keys_b, keys_g, npoly, level, key_level, pt_level, alpha, sp, k)
    want = [mfhe.to_host_u64(w).reshape(npoly, level, n) for w in want]
    assert want[0].any() and want[1].any()
    for ipad, opad in ((0, 0), (2, 4), (3, 5)):
        b0 = _polys(mfhe, npoly, level, n, ipad, 0, c0_h)
        b1 = _polys(mfhe, npoly, level, n, ipad, 0, c1_h)
        o0 = _polys(mfhe, npoly, level, n, opad)
        o1 = _polys(mfhe, npoly, level, n, opad)
        ctx.lt_apply(b0.t, b1.t, pt, o0.t, o1.t, npoly, level, key_level, alpha, sp, k, plan["baby_elt"],
                     plan["giant_elt"], keys_b, keys_g, plan["term_giant"], plan["term_baby"], pt_level=pt_level,
                     in_stride=b0.stride, out_stride=o0.stride)
        torch.cuda.synchronize()
        msg = f"pads {ipad}, {opad}"
        np.testing.assert_array_equal(o0.blocks((npoly, level, n)), want[0], err_msg="out0 " + msg)
        np.testing.assert_array_equal(o1.blocks((npoly, level, n)), want[1], err_msg="out1 " + msg)
        o0.check_pads()
        o1.check_pads()
        np.testing.assert_array_equal(b0.blocks((npoly, level, n)), c0_h)
        np.testing.assert_array_equal(b1.blocks((npoly, level, n)), c1_h)
    np.testing.assert_array_equal(mfhe.to_host_u64(pt), pt_h.ravel())
    # a plan whose first giant step with terms is not step 0: the sum starts from the rotation
    late = dict(plan)
    late["term_giant"], late["term_baby"] = [2, 2], [1, 2]
    want = _compose(mfhe, ctx, mod, c0, c1, pt, late, keys_b, keys_g, npoly, level, key_level, pt_level, alpha, sp, k)
    o0 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    ctx.lt_apply(c0, c1, pt, o0, o1, npoly, level, key_level, alpha, sp, k, late["baby_elt"], late["giant_elt"], keys_b,
                 keys_g, late["term_giant"], late["term_baby"], pt_level=pt_level)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mfhe.to_host_u64(o0), mfhe.to_host_u64(want[0]).ravel())
    np.testing.assert_array_equal(mfhe.to_host_u64(o1), mfhe.to_host_u64(want[1]).ravel())


@pytest.mark.parametrize("bits", km.PRIME_CLASSES, ids=["f64-ntt", "u64-ntt"])
def test_lt_apply_equals_the_model(mfhe, bits):
    """N = 16, the seeded inputs of tests/test_lintrans_cpu.py: keys assembled on the device, plaintexts sent through
    ntt_fwd on all 7 limbs (pt_level 5), the transform back through ntt_inv equals lt_model.transform on every limb."""
    import torch
    cs = lm.seeded_case(bits)
    q, p, n, plan = cs["q"], cs["p"], cs["n"], cs["plan"]
    mod = q + p
    ctx = mfhe.Context(mod, 4, mfhe.CONV_PHANTOM)
    dev = {g: _device_key(mfhe, ctx, dict(kp, q=q, p=p, n=n, alpha=cs["alpha"])) for g, kp in cs["key_parts"].items()}
    keys_b = [None] + [dev[g] for g in plan["baby_elt"][1:]]
    keys_g = [None] + [dev[g] for g in plan["giant_elt"][1:]]
    pt = ctx.ntt_fwd(mfhe.to_device_u64(_residues(cs["pts"], mod).ravel()), len(cs["pts"]), 0, 7)
    for level in km.CASE_LEVELS:
        c0, c1 = cs["ct"][level]
        w0, w1, margin = lm.transform(q, p, cs["alpha"], level, c0, c1, plan, cs["keys"], cs["pts"])
        assert margin >= 2.0 ** -30
        d = ctx.ntt_fwd(mfhe.to_device_u64(_residues([c0, c1], q[:level]).ravel()), 2, 0, level)
        o0 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        o1 = torch.zeros(level * n, dtype=torch.int64, device="cuda")
        ctx.lt_apply(d[:level * n], d[level * n:], pt, o0, o1, 1, level, 5, cs["alpha"], 5, 2, plan["baby_elt"],
                     plan["giant_elt"], keys_b, keys_g, plan["term_giant"], plan["term_baby"], pt_level=5)
        ctx.ntt_inv(o0, 1, 0, level)
        ctx.ntt_inv(o1, 1, 0, level)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mfhe.to_host_u64(o0).reshape(1, level, n), _residues([w0], q[:level]),
                                      err_msg=f"out0 level {level}")
        np.testing.assert_array_equal(mfhe.to_host_u64(o1).reshape(1, level, n), _residues([w1], q[:level]),
                                      err_msg=f"out1 level {level}")


def test_graph_capture_after_reserve(mfhe):
    """After lt_reserve, lt_apply allocates nothing and copies nothing to the device: it is captured into a graph on one
    stream (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed twice on changed inputs; each
    replay equals the eager call on those inputs."""
    import torch
    log_n, bits = 10, (45, 49)
    mod, n = _moduli(log_n, bits), 1 << log_n
    ctx = mfhe.Context(list(mod), log_n, mfhe.CONV_PHANTOM)   # a fresh context: no table cached yet
    npoly, level, key_level, alpha, sp, k = 2, 5, 5, 2, 5, 2
    plan = mfhe.bsgs_plan([0, 1, 2, 3, 5], 2, log_n)
    nb, ng, nt = len(plan["baby_elt"]), len(plan["giant_elt"]), len(plan["term_giant"])
    assert (nb, ng, nt) == (2, 3, 5)
    ctx.lt_reserve(npoly, level, key_level, alpha, sp, k, nb)
    rng = np.random.default_rng(6)
    keys_b = [None] + [mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, n).ravel()) for _ in range(nb - 1)]
    keys_g = [None] + [mfhe.to_device_u64(_random_rows(rng, (3, 2), mod, n).ravel()) for _ in range(ng - 1)]
    pt = mfhe.to_device_u64(_random_rows(rng, (nt,), mod, n).ravel())
    d0 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    d1 = mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel())
    o0 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.zeros(npoly * level * n, dtype=torch.int64, device="cuda")

    def apply(a0, a1):
        ctx.lt_apply(d0, d1, pt, a0, a1, npoly, level, key_level, alpha, sp, k, plan["baby_elt"], plan["giant_elt"],
                     keys_b, keys_g, plan["term_giant"], plan["term_baby"])

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        apply(o0, o1)
    first = None
    for _ in range(2):                                         # the captured inputs, then fresh ones
        o0.zero_()
        o1.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = (mfhe.to_host_u64(o0).copy(), mfhe.to_host_u64(o1).copy())
        e0, e1 = torch.zeros_like(o0), torch.zeros_like(o1)
        apply(e0, e1)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[0], mfhe.to_host_u64(e0))
        np.testing.assert_array_equal(got[1], mfhe.to_host_u64(e1))
        assert got[0].any() and got[1].any()
        if first is not None:
            assert (first[0] != got[0]).any() and (first[1] != got[1]).any()
        first = got
        d0.copy_(mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel()))
        d1.copy_(mfhe.to_device_u64(_random_rows(rng, (npoly,), mod[:level], n).ravel()))


# ---------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(mfhe):
    import torch
    lib = mfhe.lib
    mod, N = _moduli(4, (45, 49)), 16
    ctx = mfhe.Context(list(mod), 4, mfhe.CONV_PHANTOM)
    h = ctx.handle
    names = ("c0", "c1", "gk", "u", "pt", "acc", "o0", "o1", "rs")
    bufs = {name: _polys(mfhe, 1, 3 * 2 * 7, N) for name in names}
    p0, p1, pk, pu, pp, pa, q0, q1, pr = (bufs[name].t.data_ptr() for name in names)
    E = mfhe.EINVAL
    L5, L7 = 5 * N, 7 * N
    ints = lambda xs: (ctypes.c_int * max(len(xs), 1))(*xs)   # noqa: E731

    def bs(c0=p0, ist=L5, r=pr, dst=L7, pst=L7, key=pk, u=pu, ust=2 * L7, npoly=1, level=5, kl=5, alpha=2, sp=5, k=2,
           g=3):
        return lib.mfhe_lt_baby_step(h, c0, ist, r, dst, pst, key, u, ust, npoly, level, kl, alpha, sp, k, g, None)

    def mac(u=pu, sst=2 * L7, pst=2 * L7, nslots=2, pt=pp, tst=L7, npt=2, ptl=5, acc=pa, ast=2 * L7, tu=(0, 1),
            tp=(1, 0), nt=None, npoly=1, level=5, sp=5, k=2):
        return lib.mfhe_lt_pt_mac(h, u, sst, pst, nslots, pt, tst, npt, ptl, acc, ast, ints(tu), ints(tp),
                                  len(tu) if nt is None else nt, npoly, level, sp, k, None)

    def ap(be=(1, 5), ge=(1, 3), kb=(None, pk), kg=(None, pk), tg=(0, 1), tb=(0, 1), c0=p0, c1=p1, ist=L5, pt=pp,
           tst=L7, ptl=5, o0=q0, o1=q1, ost=L5, npoly=1, level=5, kl=5, alpha=2, sp=5, k=2, noplan=False):
        a_kb, a_kg = (ctypes.c_void_p * len(kb))(*kb), (ctypes.c_void_p * len(kg))(*kg)
        plan = mfhe.LtPlan(len(be), len(ge), len(tg), ints(be), ints(ge), a_kb, a_kg, ints(tg), ints(tb))
        return lib.mfhe_lt_apply(h, None if noplan else ctypes.byref(plan), c0, c1, ist, pt, tst, ptl, o0, o1, ost,
                                 npoly, level, kl, alpha, sp, k, None)

    cases = {
        "baby null c0": lambda: bs(c0=None),
        "baby null raised": lambda: bs(r=None),
        "baby null u": lambda: bs(u=None),
        "baby null key with g = 3": lambda: bs(key=None),
        "baby even g": lambda: bs(g=4),
        "baby g < 1": lambda: bs(g=0),
        "baby g >= 2N": lambda: bs(g=33),
        "baby keyless even g": lambda: bs(key=None, g=2),
        "baby alpha < 1": lambda: bs(alpha=0),
        "baby level > key_level": lambda: bs(kl=4),
        "baby special outside": lambda: bs(sp=6),
        "baby in stride": lambda: bs(ist=L5 - 1, npoly=2),
        "baby u stride": lambda: bs(ust=2 * L7 - 1),
        "baby poly stride": lambda: bs(pst=L7 - 1),
        "baby digit stride": lambda: bs(dst=L7 - 1),
        "baby c0 is u": lambda: bs(u=p0),
        "baby c0 overlaps u": lambda: bs(c0=pu + 8 * N),
        "baby raised overlaps u": lambda: bs(u=pr + 8 * N),
        "baby keyless c1 is u": lambda: bs(key=None, g=1, r=pu),
        "baby key overlaps u": lambda: bs(u=pk + 8 * N),
        "mac null u": lambda: mac(u=None),
        "mac null pt": lambda: mac(pt=None),
        "mac null acc": lambda: mac(acc=None),
        "mac no terms": lambda: mac(tu=(), tp=()),
        "mac 65 terms": lambda: mac(tu=(0,) * 65, tp=(0,) * 65),
        "mac nterms negative": lambda: mac(nt=-1),
        "mac term_u == nslots": lambda: mac(tu=(0, 2)),
        "mac term_u negative": lambda: mac(tu=(-1, 0)),
        "mac term_pt == npt": lambda: mac(tp=(2, 0)),
        "mac term_pt negative": lambda: mac(tp=(0, -1)),
        "mac pt_level < level": lambda: mac(ptl=4),
        "mac special overlaps pt_level": lambda: mac(level=3, ptl=5, sp=4),
        "mac poly stride": lambda: mac(pst=2 * L7 - 1),
        "mac slot stride": lambda: mac(sst=2 * L7 - 1, npoly=1, nslots=2),
        "mac pt stride": lambda: mac(tst=L7 - 1),
        "mac acc stride": lambda: mac(ast=2 * L7 - 1),
        "mac acc is u": lambda: mac(acc=pu),
        "mac acc is the second slot": lambda: mac(acc=pu + 8 * 2 * L7),
        "mac acc overlaps pt": lambda: mac(acc=pp + 8 * N),
        "apply null plan": lambda: ap(noplan=True),
        "apply null c0": lambda: ap(c0=None),
        "apply null c1": lambda: ap(c1=None),
        "apply null pt": lambda: ap(pt=None),
        "apply null out0": lambda: ap(o0=None),
        "apply null out1": lambda: ap(o1=None),
        "apply alpha < 1": lambda: ap(alpha=0),
        "apply level > key_level": lambda: ap(kl=4),
        "apply pt_level < level": lambda: ap(ptl=4),
        "apply in stride": lambda: ap(ist=L5 - 1, npoly=2),
        "apply out stride": lambda: ap(ost=L5 - 1, npoly=2),
        "apply pt stride": lambda: ap(tst=L7 - 1),
        "apply 65 terms in one giant": lambda: ap(tg=(0,) * 65, tb=(0,) * 65),
        "apply baby_elt[0] != 1": lambda: ap(be=(5, 1)),
        "apply giant_elt[0] != 1": lambda: ap(ge=(3, 1)),
        "apply even element": lambda: ap(be=(1, 6)),
        "apply term_baby out of range": lambda: ap(tb=(0, 2)),
        "apply term_giant decreases": lambda: ap(tg=(1, 0)),
        "apply no terms": lambda: ap(tg=(), tb=()),
        "apply used baby step without a key": lambda: ap(kb=(None, None)),
        "apply used giant step without a key": lambda: ap(kg=(None, None)),
        "apply c0 is out0": lambda: ap(o0=p0),
        "apply c1 overlaps out1": lambda: ap(o1=p1 + 8 * N),
        "apply pt overlaps out0": lambda: ap(o0=pp + 8 * N),
        "apply key overlaps out1": lambda: ap(o1=pk + 8 * N),
        "apply outputs overlap": lambda: ap(o1=q0 + 8 * N),
        "reserve alpha < 1": lambda: lib.mfhe_lt_reserve(h, 1, 5, 5, 0, 5, 2, 2),
        "reserve n_baby < 1": lambda: lib.mfhe_lt_reserve(h, 1, 5, 5, 2, 5, 2, 0),
        "reserve level > key_level": lambda: lib.mfhe_lt_reserve(h, 1, 5, 4, 2, 5, 2, 2),
        "reserve special outside": lambda: lib.mfhe_lt_reserve(h, 1, 5, 5, 2, 6, 2, 2),
    }
    for name, call in cases.items():
        assert call() == E, name
        assert lib.mfhe_last_error(), name
    # the same calls with nothing wrong pass the checks (npoly 0: nothing is launched)
    assert bs(npoly=0) == mfhe.OK and mac(npoly=0) == mfhe.OK and ap(npoly=0) == mfhe.OK
    # a context without the phantom tables
    plain = mfhe.Context(list(mod), 4, 0)
    hp, R = plain.handle, mfhe.ENOTREADY
    assert lib.mfhe_lt_baby_step(hp, p0, L5, pr, L7, L7, pk, pu, 2 * L7, 1, 5, 5, 2, 5, 2, 3, None) == R
    assert lib.mfhe_lt_pt_mac(hp, pu, 2 * L7, 2 * L7, 1, pp, L7, 1, 5, pa, 2 * L7, ints((0,)), ints((0,)), 1, 1, 5, 5, 2,
                              None) == R
    assert lib.mfhe_lt_reserve(hp, 1, 5, 5, 2, 5, 2, 2) == R
    torch.cuda.synchronize()
    for name, b in bufs.items():   # nothing ran: every word is still the canary
        assert b.all_canary(), name
