"""GPU checks of the RNS basis conversion kernels (csrc/bconv.hip; include/mfhe.h mfhe_rns_bconv, mfhe_rns_moddown,
mfhe_rns_modup and the NTT-domain forms), bit-exact against Python integers computed here.

Notation (include/mfhe.h): source moduli s_i with product S, y_i = [x_i (S/s_i)^-1]_(s_i);
FAST out_j = (sum_i y_i (S/s_i)) mod d_j; CENTERED out_j = x~ mod d_j for the centred value x~ of x;
ModDown out_i = round(x / P) mod q_i.  Every bound is exact equality: the arithmetic is integer (the one f64 sum
of CENTERED only selects the multiple of S, and the inputs stay 0.01 S away from where it could flip, against the
documented 2^-40 S)."""
import ctypes
import functools
import random

import numpy as np
import pytest

from primes import primes_of_size

pytestmark = pytest.mark.gpu

CANARY = 0xDEADBEEFCAFEF00D
RNS = [17592186435073, 17182765057, 17184541441, 17186120449, 17186515201, 17186909953,
       17188883713, 17190462721, 17190857473, 17191844353, 17192831233]
PMOD = [18014398515156481, 549757491457, 549759662593]


def _prod(xs):
    r = 1
    for x in xs:
        r *= int(x)
    return r


def _obj(a):
    return np.array(a, dtype=object)


def _u64(a):
    return np.array(a, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _mixed_moduli():
    """57 primes of 20, 35, 50, 55 and 61 bits: limbs [0, 17) are the sources, [17, 57) the destinations, every size
    in both.  The small sizes fill up the count: a context's modulus product must stay below 2^2047 (wide CRT)."""
    sizes = ([61, 20, 55, 35, 50, 61, 20, 55, 35, 50, 61, 20, 35, 20, 35, 20, 35] +
             [55, 50, 61, 35, 20, 50] + [35] * 11 + [20] * 23)
    pools = {b: iter(primes_of_size(b, 2, sizes.count(b))) for b in set(sizes)}
    out = [next(pools[b]) for b in sizes]
    assert len(set(out)) == 57 and _prod(out).bit_length() < 2047
    return tuple(out)


@pytest.fixture(scope="module")
def mixed_ctx(mfhe):
    return mfhe.Context(list(_mixed_moduli()), 1, 0)


@pytest.fixture(scope="module")
def ref_ctx(mfhe):
    return mfhe.Context(RNS + PMOD, 8, 0)


def _random_residues(rng, npoly, moduli, nc):
    """Canonical residues [npoly][len(moduli)][nc]; coefficient 0 of poly 0 is 0 on every limb, coefficient 1 of poly 0
    and coefficient 0 of the last poly are q - 1 on every limb."""
    q = _u64(moduli)[None, :, None]
    x = rng.integers(0, 2 ** 63, (npoly, len(moduli), nc), dtype=np.uint64) % q
    x[0, :, 0] = 0
    if nc > 1:
        x[0, :, 1] = _u64(moduli) - np.uint64(1)
    if npoly > 1:
        x[-1, :, 0] = _u64(moduli) - np.uint64(1)
    return x


def _fast_integer(x, src):
    """sum_i y_i (S/s_i) as Python integers, [npoly][nc], from residues x [npoly][ns][nc]."""
    S = _prod(src)
    xo = x.astype(object)
    tot = np.zeros((x.shape[0], x.shape[2]), dtype=object)
    for i, s in enumerate(src):
        m = S // s
        y = xo[:, i, :] * pow(m, -1, s) % s
        tot = tot + y * m
    return tot


def _residues_of(vals, moduli):
    """[len(moduli)][len(vals)] uint64 residues of Python integers (negative values allowed)."""
    return _u64([[int(v) % int(m) for v in vals] for m in moduli])


class _Buf:
    """A device buffer of npoly blocks of rows * nc words, `stride` words apart, `offset` words into an allocation
    filled with a canary; check_pads() asserts every word outside the blocks is still the canary."""

    def __init__(self, mfhe, npoly, rows, nc, stride, offset=0, data=None):
        self.mfhe, self.npoly, self.words, self.stride, self.offset = mfhe, npoly, rows * nc, stride, offset
        self.shape = (npoly, rows, nc)
        host = np.full(offset + npoly * stride + 2, CANARY, dtype=np.uint64)
        if data is not None:
            for p in range(npoly):
                host[offset + p * stride: offset + p * stride + self.words] = data[p].ravel()
        self.full = mfhe.to_device_u64(host)
        self.t = self.full[offset:]

    def blocks(self):
        h = self.mfhe.to_host_u64(self.full)
        return np.stack([h[self.offset + p * self.stride: self.offset + p * self.stride + self.words]
                         for p in range(self.npoly)]).reshape(self.shape)

    def check_pads(self):
        h = self.mfhe.to_host_u64(self.full).copy()
        for p in range(self.npoly):
            h[self.offset + p * self.stride: self.offset + p * self.stride + self.words] = CANARY
        assert (h == np.uint64(CANARY)).all(), "words outside the output rows were written"


# (name, in pad, out pad, base offset in words): even pads keep the 16-byte form for even ncoeff, the odd pad and the
# one-word offset force the scalar variant
LAYOUTS = [("dense", 0, 0, 0), ("padded", 2, 4, 0), ("padded-odd", 3, 5, 0), ("misaligned", 0, 0, 1)]


@pytest.mark.parametrize("dst_count", [1, 11, 40])
@pytest.mark.parametrize("src_count", [1, 2, 3, 17])
def test_fast_conversion_bit_exact(mfhe, mixed_ctx, src_count, dst_count):
    import torch
    mod = _mixed_moduli()
    src, dst = mod[:src_count], mod[17:17 + dst_count]
    rng = np.random.default_rng(100 * src_count + dst_count)
    x = _random_residues(rng, 3, src, 258)
    for nc in (1, 2, 255, 258):
        xs = np.ascontiguousarray(x[:, :, :nc])
        if nc > 1:
            xs[0, :, 1] = _u64(src) - np.uint64(1)
        tot = _fast_integer(xs, src)
        want = np.stack([(tot % int(d)).astype(np.uint64) for d in dst], axis=1)   # [3][dst_count][nc]
        for npoly in (1, 3):
            for name, ipad, opad, off in LAYOUTS:
                bi = _Buf(mfhe, npoly, src_count, nc, src_count * nc + ipad, off, xs)
                bo = _Buf(mfhe, npoly, dst_count, nc, dst_count * nc + opad, off)
                mixed_ctx.rns_bconv(bi.t, bo.t, npoly, nc, 0, src_count, 17, dst_count, mfhe.BCONV_FAST,
                                    in_stride=bi.stride, out_stride=bo.stride)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(bo.blocks(), want[:npoly], err_msg=f"{name} nc={nc} npoly={npoly}")
                bo.check_pads()
                np.testing.assert_array_equal(bi.blocks(), xs[:npoly])   # input untouched


def _centered_values(S, count, seed):
    lim = 49 * S // 100
    rnd = random.Random(seed)
    vals = [0, 1, -1, lim, -lim]
    vals += [rnd.randint(-lim, lim) for _ in range(count - len(vals))]
    return vals


@pytest.mark.parametrize("src_count", [1, 2, 3, 17])
def test_centered_conversion_bit_exact(mfhe, mixed_ctx, src_count):
    import torch
    mod = _mixed_moduli()
    src, dst = mod[:src_count], mod[17:28]
    S = _prod(src)
    vals = _centered_values(S, 130, src_count)
    x = _residues_of(vals, src)[None]
    want = _residues_of(vals, dst)[None]
    for nc in (130, 129):   # the 16-byte form, then the scalar variant
        bi = _Buf(mfhe, 1, src_count, nc, src_count * nc, 0, np.ascontiguousarray(x[:, :, :nc]))
        bo = _Buf(mfhe, 1, 11, nc, 11 * nc + 2)
        mixed_ctx.rns_bconv(bi.t, bo.t, 1, nc, 0, src_count, 17, 11, mfhe.BCONV_CENTERED, out_stride=bo.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want[:, :, :nc])
        bo.check_pads()


@pytest.mark.parametrize("src_count", [1, 2, 3, 17])
def test_centered_conversion_at_half_s_returns_a_documented_value(mfhe, mixed_ctx, src_count):
    import torch
    mod = _mixed_moduli()
    src, dst = mod[:src_count], mod[17:28]
    S = _prod(src)
    vals = [S // 2, -(S // 2)]
    bi = _Buf(mfhe, 1, src_count, 2, src_count * 2, 0, _residues_of(vals, src)[None])
    bo = _Buf(mfhe, 1, 11, 2, 22)
    mixed_ctx.rns_bconv(bi.t, bo.t, 1, 2, 0, src_count, 17, 11, mfhe.BCONV_CENTERED)
    torch.cuda.synchronize()
    got = bo.blocks()[0]
    for k, (v, alt) in enumerate(((vals[0], vals[0] - S), (vals[1], vals[1] + S))):
        col = [int(g) for g in got[:, k]]
        assert col in ([v % d for d in dst], [alt % d for d in dst]), (k, col)


def _moddown_case(keep, drop, nc, npoly, seed):
    """x = k P + r with |r| <= 0.49 P; rows: kept residues then dropped residues; want k mod q_i."""
    P, Q = _prod(drop), _prod(keep)
    lim = 49 * P // 100
    rnd = random.Random(seed)
    rs = [0, 1, -1, lim, -lim]
    xin, want = [], []
    for p in range(npoly):
        r = (rs + [rnd.randint(-lim, lim) for _ in range(nc)])[:nc]
        k = [rnd.randint(-(Q // 2), Q // 2) for _ in range(nc)]
        k[:3] = [0, 1, -1][:nc]
        xv = [kk * P + rr for kk, rr in zip(k, r)]
        xin.append(_residues_of(xv, list(keep) + list(drop)))
        want.append(_residues_of(k, keep))
    return np.stack(xin), np.stack(want)


def _run_moddown(mfhe, ctx, keep_count, drop_start, drop_count, nc, npoly, seed):
    import torch
    mod = ctx.moduli
    keep, drop = mod[:keep_count], mod[drop_start:drop_start + drop_count]
    x, want = _moddown_case(keep, drop, nc, npoly, seed)
    rows = keep_count + drop_count
    # out of place, padded strides
    bi = _Buf(mfhe, npoly, rows, nc, rows * nc + 2, 0, x)
    bo = _Buf(mfhe, npoly, keep_count, nc, keep_count * nc + 4)
    ctx.rns_moddown(bi.t, bo.t, npoly, nc, keep_count, drop_start, drop_count, in_stride=bi.stride,
                    out_stride=bo.stride)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bo.blocks(), want)
    bo.check_pads()
    np.testing.assert_array_equal(bi.blocks(), x)
    # in place on the kept rows: the dropped rows stay as they were
    bp = _Buf(mfhe, npoly, rows, nc, rows * nc + 2, 0, x)
    ctx.rns_moddown(bp.t, bp.t, npoly, nc, keep_count, drop_start, drop_count, in_stride=bp.stride)
    torch.cuda.synchronize()
    got = bp.blocks()
    np.testing.assert_array_equal(got[:, :keep_count], want)
    np.testing.assert_array_equal(got[:, keep_count:], x[:, keep_count:])
    bp.check_pads()


@pytest.mark.parametrize("nc", [258, 255])
@pytest.mark.parametrize("drop_count", [1, 3])
def test_moddown_mixed_primes(mfhe, mixed_ctx, drop_count, nc):
    _run_moddown(mfhe, mixed_ctx, 5, 20, drop_count, nc, 2, 7 * drop_count + nc)


@pytest.mark.parametrize("drop_count", [1, 3])
def test_moddown_reference_basis(mfhe, ref_ctx, drop_count):
    _run_moddown(mfhe, ref_ctx, 11, 11, drop_count, 256, 2, drop_count)


def test_rescale_reference_basis(mfhe, ref_ctx):
    """rns_rescale(level): drop limb level - 1 of the Q basis, rows [0, level)."""
    import torch
    for level in (11, 7, 2):
        x, want = _moddown_case(RNS[:level - 1], RNS[level - 1:level], 256, 2, level)
        bi = _Buf(mfhe, 2, level, 256, level * 256, 0, x)
        bo = _Buf(mfhe, 2, level - 1, 256, (level - 1) * 256)
        ref_ctx.rns_rescale(bi.t, bo.t, 2, 256, level)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want)
        bo.check_pads()


def _modup_want(x, moduli, level, ds, dc, special):
    """Expected [npoly][level + len(special)][nc]: digit rows copied, the others the FAST formula."""
    src = moduli[ds:ds + dc]
    tot = _fast_integer(np.ascontiguousarray(x[:, ds:ds + dc]), src)
    rows = []
    for r, d in enumerate(list(moduli[:level]) + list(special)):
        rows.append(x[:, r] if ds <= r < ds + dc else (tot % int(d)).astype(np.uint64))
    return np.stack(rows, axis=1)


@pytest.mark.parametrize("level", [11, 7])
def test_modup_reference_basis(mfhe, ref_ctx, level):
    import torch
    rng = np.random.default_rng(level)
    nc, npoly = 256, 2
    x = _random_residues(rng, npoly, RNS[:level], nc)
    for ds in range(0, level, 3):
        dc = min(3, level - ds)
        want = _modup_want(x, RNS, level, ds, dc, PMOD)
        bi = _Buf(mfhe, npoly, level, nc, level * nc + 2, 0, x)
        bo = _Buf(mfhe, npoly, level + 3, nc, (level + 3) * nc + 6)
        ref_ctx.rns_modup(bi.t, bo.t, npoly, nc, level, ds, dc, 11, 3, in_stride=bi.stride, out_stride=bo.stride)
        torch.cuda.synchronize()
        got = bo.blocks()
        np.testing.assert_array_equal(got[:, ds:ds + dc], x[:, ds:ds + dc], err_msg="digit rows are copies")
        np.testing.assert_array_equal(got, want, err_msg=f"digit {ds}+{dc}")
        bo.check_pads()


def test_modup_scalar_variant_and_long_digit(mfhe, mixed_ctx):
    """Odd ncoeff (scalar kernel) and a 17-limb digit (the generic loop across the 16-term chunk), with destination
    rows on both sides of the digit and special limbs."""
    import torch
    mod = list(_mixed_moduli())
    rng = np.random.default_rng(5)
    level, ds, dc, sp, nsp, nc, npoly = 22, 2, 17, 30, 4, 255, 2
    x = _random_residues(rng, npoly, mod[:level], nc)
    want = _modup_want(x, mod, level, ds, dc, mod[sp:sp + nsp])
    bi = _Buf(mfhe, npoly, level, nc, level * nc, 0, x)
    bo = _Buf(mfhe, npoly, level + nsp, nc, (level + nsp) * nc + 1)
    mixed_ctx.rns_modup(bi.t, bo.t, npoly, nc, level, ds, dc, sp, nsp, out_stride=bo.stride)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bo.blocks(), want)
    bo.check_pads()


# ---------------------------------------------------------------------------------------------------------------
# every instantiation of bconv_kernel, and the generic loop's chunk boundaries
#
# pick_ns (csrc/bconv.hip) unrolls source counts 1 .. 8 and sends every longer source to a loop that reduces after
# every 16 terms.  The tests above run 1, 2, 3 and 17; these run 4 .. 8, the first generic count 9, one full chunk
# (16), two full chunks (32) and two chunks and one term (33), in all three modes the kernel has, in the 16-byte form
# (ncoeff 258) and the scalar one (ncoeff 255), on more than one block.
# ---------------------------------------------------------------------------------------------------------------
SRC_COUNTS = [4, 5, 6, 7, 8, 9, 16, 32, 33]


def _dst_range(src_count):
    """Destination limbs (start, count): [17, 57) while the sources end below 17, else [33, 57)."""
    return (17, 40) if src_count <= 17 else (33, 24)


@pytest.mark.parametrize("src_count", SRC_COUNTS)
def test_fast_conversion_every_source_count(mfhe, mixed_ctx, src_count):
    import torch
    mod = _mixed_moduli()
    ds, dc = _dst_range(src_count)
    src, dst = mod[:src_count], mod[ds:ds + dc]
    rng = np.random.default_rng(1000 + src_count)
    npoly = 3
    for nc in (258, 255):
        x = _random_residues(rng, npoly, src, nc)
        tot = _fast_integer(x, src)
        want = np.stack([(tot % int(d)).astype(np.uint64) for d in dst], axis=1)   # [3][dc][nc]
        bi = _Buf(mfhe, npoly, src_count, nc, src_count * nc + 2, 0, x)
        bo = _Buf(mfhe, npoly, dc, nc, dc * nc + 4)
        mixed_ctx.rns_bconv(bi.t, bo.t, npoly, nc, 0, src_count, ds, dc, mfhe.BCONV_FAST, in_stride=bi.stride,
                            out_stride=bo.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want, err_msg=f"nc={nc}")
        bo.check_pads()
        np.testing.assert_array_equal(bi.blocks(), x)   # input untouched


@pytest.mark.parametrize("src_count", SRC_COUNTS)
def test_centered_conversion_every_source_count(mfhe, mixed_ctx, src_count):
    import torch
    mod = _mixed_moduli()
    ds, dc = _dst_range(src_count)
    src, dst = mod[:src_count], mod[ds:ds + dc]
    S = _prod(src)
    npoly = 3
    vals = [_centered_values(S, 258, 10 * src_count + p) for p in range(npoly)]
    x = np.stack([_residues_of(v, src) for v in vals])
    want = np.stack([_residues_of(v, dst) for v in vals])
    for nc in (258, 255):
        xs = np.ascontiguousarray(x[:, :, :nc])
        bi = _Buf(mfhe, npoly, src_count, nc, src_count * nc + 2, 0, xs)
        bo = _Buf(mfhe, npoly, dc, nc, dc * nc + 4)
        mixed_ctx.rns_bconv(bi.t, bo.t, npoly, nc, 0, src_count, ds, dc, mfhe.BCONV_CENTERED, in_stride=bi.stride,
                            out_stride=bo.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want[:, :, :nc], err_msg=f"nc={nc}")
        bo.check_pads()
        np.testing.assert_array_equal(bi.blocks(), xs)


@pytest.mark.parametrize("nc", [258, 255])
@pytest.mark.parametrize("drop_count", [4, 5, 8, 9, 17])
def test_moddown_every_kind_of_drop_count(mfhe, mixed_ctx, drop_count, nc):
    """Unrolled counts, the first generic count and the generic loop across its 16-term chunk; the dropped limbs
    [17, 17 + drop_count) hold primes of 55, 50, 61, 35 and 20 bits.  Out of place and in place."""
    _run_moddown(mfhe, mixed_ctx, 5, 17, drop_count, nc, 2, 100 * drop_count + nc)


@pytest.mark.parametrize("nc", [258, 255])
@pytest.mark.parametrize("digit_count", [4, 5, 8, 9])
def test_modup_every_kind_of_digit_count(mfhe, mixed_ctx, digit_count, nc):
    """A digit inside level 22, so destination rows lie on both sides of it, and 4 special limbs."""
    import torch
    mod = list(_mixed_moduli())
    rng = np.random.default_rng(50 + digit_count)
    level, ds, sp, nsp, npoly = 22, 2, 30, 4, 2
    x = _random_residues(rng, npoly, mod[:level], nc)
    want = _modup_want(x, mod, level, ds, digit_count, mod[sp:sp + nsp])
    bi = _Buf(mfhe, npoly, level, nc, level * nc + 2, 0, x)
    bo = _Buf(mfhe, npoly, level + nsp, nc, (level + nsp) * nc + 4)
    mixed_ctx.rns_modup(bi.t, bo.t, npoly, nc, level, ds, digit_count, sp, nsp, in_stride=bi.stride,
                        out_stride=bo.stride)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bo.blocks(), want)
    bo.check_pads()
    np.testing.assert_array_equal(bi.blocks(), x)


# ---------------------------------------------------------------------------------------------------------------
# the centred estimate at the documented limit
#
# include/mfhe.h promises the centred value for |x~| <= (1/2 - 2^-40) S.  m = floor(S/2) - ceil(S 2^-39) and m + 1 lie
# inside that window with a factor of two to spare (S > 2^40 here), so x~ = +-m, +-(m - 1), +-(m + 1) must come out as
# exactly x~ mod d_j: an f64 estimate that had lost ten of its bits would round some of them to the wrong multiple of S.
# ---------------------------------------------------------------------------------------------------------------
def _limit_values(S):
    assert S > 1 << 40
    m = S // 2 - -(-S // (1 << 39))
    assert 2 * (m + 1) * (1 << 40) <= ((1 << 40) - 2) * S, "inside (1/2 - 2^-40) S"
    return [m, -m, m - 1, -(m - 1), m + 1, -(m + 1)]


@pytest.mark.parametrize("src_count", [1, 3, 8, 17, 33])
def test_centered_conversion_exact_at_the_documented_limit(mfhe, mixed_ctx, src_count):
    import torch
    mod = _mixed_moduli()
    ds, dc = (17, 11) if src_count <= 17 else (33, 24)
    src, dst = mod[:src_count], mod[ds:ds + dc]
    vals = _limit_values(_prod(src))
    x, want = _residues_of(vals, src)[None], _residues_of(vals, dst)[None]
    nc = len(vals)
    for off in (0, 1):   # the 16-byte form, then (one word off) the scalar variant
        bi = _Buf(mfhe, 1, src_count, nc, src_count * nc, off, x)
        bo = _Buf(mfhe, 1, dc, nc, dc * nc + 2, off)
        mixed_ctx.rns_bconv(bi.t, bo.t, 1, nc, 0, src_count, ds, dc, mfhe.BCONV_CENTERED, out_stride=bo.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want, err_msg=f"offset {off}")
        bo.check_pads()


@pytest.mark.parametrize("drop_count", [1, 3, 9])
def test_moddown_exact_at_the_documented_limit(mfhe, mixed_ctx, drop_count):
    """x = k P + r with the remainders r of _limit_values(P): round(x / P) = k on every kept limb."""
    import torch
    mod = _mixed_moduli()
    keep_count, drop_start = 5, 17
    keep, drop = mod[:keep_count], mod[drop_start:drop_start + drop_count]
    P, Q = _prod(drop), _prod(keep)
    rnd = random.Random(drop_count)
    rs = _limit_values(P)
    ks = [[0, 0, 1, 1, -1, -1], [rnd.randint(-(Q // 2), Q // 2) for _ in rs]]
    x = np.stack([_residues_of([k * P + r for k, r in zip(kk, rs)], list(keep) + list(drop)) for kk in ks])
    want = np.stack([_residues_of(kk, keep) for kk in ks])
    nc, rows = len(rs), keep_count + drop_count
    for off in (0, 1):
        bi = _Buf(mfhe, 2, rows, nc, rows * nc, off, x)
        bo = _Buf(mfhe, 2, keep_count, nc, keep_count * nc + 2, off)
        mixed_ctx.rns_moddown(bi.t, bo.t, 2, nc, keep_count, drop_start, drop_count, out_stride=bo.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want, err_msg=f"offset {off}")
        bo.check_pads()


def _ntt_moduli(log_n, bits):
    return primes_of_size(bits[0], 2 << log_n, 5) + primes_of_size(bits[1], 2 << log_n, 2)


@pytest.mark.parametrize("bits", [(45, 49), (50, 61)], ids=["f64-ntt", "u64-ntt"])
@pytest.mark.parametrize("log_n", [4, 10])
def test_ntt_domain_forms_equal_the_composition(mfhe, log_n, bits):
    """mfhe_ntt_modup / mfhe_ntt_moddown against ntt_inv on contiguous copies of the rows, the rns_* call, ntt_fwd."""
    import torch
    moduli = _ntt_moduli(log_n, bits)
    assert len(moduli) == 7
    ctx = mfhe.Context(moduli, log_n, mfhe.CONV_PHANTOM)
    N, batch = 1 << log_n, 3
    rng = np.random.default_rng(log_n)
    ctx.ntt_bconv_reserve(batch, 7)
    # ModUp: level 5, two special limbs; digits of 2, 2 and 1 limbs
    ev = _random_residues(rng, batch, moduli[:5], N)
    for ds, dc in ((0, 2), (2, 2), (4, 1)):
        bi = _Buf(mfhe, batch, 5, N, 5 * N + 2, 0, ev)
        bo = _Buf(mfhe, batch, 7, N, 7 * N + 4)
        ctx.ntt_modup(bi.t, bo.t, batch, 5, ds, dc, 5, 2, in_stride=bi.stride, out_stride=bo.stride)
        coef = mfhe.to_device_u64(ev.ravel())
        ctx.ntt_inv(coef, batch, 0, 5)
        comp = torch.zeros(batch * 7 * N, dtype=torch.int64, device="cuda")
        ctx.rns_modup(coef, comp, batch, N, 5, ds, dc, 5, 2)
        ctx.ntt_fwd(comp, batch, 0, 7)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), mfhe.to_host_u64(comp).reshape(batch, 7, N), err_msg=f"modup {ds}")
        bo.check_pads()
        np.testing.assert_array_equal(bi.blocks(), ev)
    # ModDown: 5 kept + 2 dropped; rescale-like 6 kept + 1 dropped; out of place and in place
    ev7 = _random_residues(rng, batch, moduli, N)
    for keep, drop in ((5, 2), (6, 1)):
        coef = mfhe.to_device_u64(ev7.ravel())
        ctx.ntt_inv(coef, batch, 0, 7)
        comp = torch.zeros(batch * keep * N, dtype=torch.int64, device="cuda")
        ctx.rns_moddown(coef, comp, batch, N, keep, keep, drop)
        ctx.ntt_fwd(comp, batch, 0, keep)
        torch.cuda.synchronize()
        want = mfhe.to_host_u64(comp).reshape(batch, keep, N)
        bi = _Buf(mfhe, batch, 7, N, 7 * N + 2, 0, ev7)
        bo = _Buf(mfhe, batch, keep, N, keep * N + 4)
        ctx.ntt_moddown(bi.t, bo.t, batch, keep, keep, drop, in_stride=bi.stride, out_stride=bo.stride)
        ctx.ntt_moddown(bi.t, bi.t, batch, keep, keep, drop, in_stride=bi.stride)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bo.blocks(), want, err_msg=f"moddown keep {keep}")
        bo.check_pads()
        got = bi.blocks()
        np.testing.assert_array_equal(got[:, :keep], want, err_msg=f"moddown in place keep {keep}")
        np.testing.assert_array_equal(got[:, keep:], ev7[:, keep:])
        bi.check_pads()


def test_graph_capture_after_reserve(mfhe):
    """After the reserve calls rns_modup and rns_moddown allocate nothing and copy nothing to the device: both are
    captured into a graph (a hipMalloc or a synchronous hipMemcpy would fail the capture) and replayed twice."""
    import torch
    ctx = mfhe.Context(RNS + PMOD, 8, 0)   # a fresh context: no table cached yet
    ctx.rns_modup_reserve(11, 3, 3, 11, 3)
    ctx.rns_moddown_reserve(11, 11, 3)
    nc, npoly = 256, 2
    rng = np.random.default_rng(9)
    x = _random_residues(rng, npoly, RNS, nc)
    d_in = mfhe.to_device_u64(x.ravel())
    d_up = torch.zeros(npoly * 14 * nc, dtype=torch.int64, device="cuda")
    d_down = torch.zeros(npoly * 11 * nc, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.rns_modup(d_in, d_up, npoly, nc, 11, 3, 3, 11, 3)
        ctx.rns_moddown(d_up, d_down, npoly, nc, 11, 11, 3)
    outs = []
    for _ in range(2):
        d_up.zero_()
        d_down.zero_()
        g.replay()
        torch.cuda.synchronize()
        outs.append((mfhe.to_host_u64(d_up).copy(), mfhe.to_host_u64(d_down).copy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    want_up = _modup_want(x, RNS, 11, 3, 3, PMOD)
    np.testing.assert_array_equal(outs[0][0].reshape(npoly, 14, nc), want_up)
    # ModDown of the raised polynomial: round((x + u Q_digit) / P) mod q_i from the integer itself
    tot = _fast_integer(np.ascontiguousarray(x[:, 3:6]), RNS[3:6])
    P = _prod(PMOD)
    up = want_up.astype(object)
    want_down = []
    for i, q in enumerate(RNS):
        # r~ = centred value of the P rows; out = (x_i - r~) P^-1 mod q_i
        Pi = [P // p for p in PMOD]
        r = sum(up[:, 11 + k] * pow(Pi[k], -1, PMOD[k]) % PMOD[k] * Pi[k] for k in range(3)) % P
        r = np.where(r > P // 2, r - P, r)
        want_down.append(((up[:, i] - r) * pow(P, -1, q) % q).astype(np.uint64))
    np.testing.assert_array_equal(outs[0][1].reshape(npoly, 11, nc), np.stack(want_down, axis=1))
    del tot


def test_argument_errors_return_before_any_launch(mfhe, ref_ctx):
    import torch
    lib, h = mfhe.lib, ref_ctx.handle
    nc = 4
    inp = _Buf(mfhe, 1, 14, nc, 14 * nc)
    out = _Buf(mfhe, 1, 14, nc, 14 * nc)
    pi, po = inp.t.data_ptr(), out.t.data_ptr()
    E = mfhe.EINVAL
    cases = {
        "bconv null in": lambda: lib.mfhe_rns_bconv(h, None, 3 * nc, po, 2 * nc, 1, nc, 0, 3, 3, 2, 0, None),
        "bconv null out": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, None, 2 * nc, 1, nc, 0, 3, 3, 2, 0, None),
        "bconv src outside": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc, 1, nc, 12, 3, 0, 2, 0, None),
        "bconv src negative": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc, 1, nc, -1, 3, 5, 2, 0, None),
        "bconv dst outside": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc, 1, nc, 0, 3, 13, 2, 0, None),
        "bconv empty src": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc, 1, nc, 0, 0, 3, 2, 0, None),
        "bconv overlap": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc, 1, nc, 0, 3, 2, 2, 0, None),
        "bconv in stride": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc - 1, po, 2 * nc, 2, nc, 0, 3, 3, 2, 0, None),
        "bconv out stride": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc - 1, 2, nc, 0, 3, 3, 2, 0, None),
        "bconv mode": lambda: lib.mfhe_rns_bconv(h, pi, 3 * nc, po, 2 * nc, 1, nc, 0, 3, 3, 2, 2, None),
        "reserve outside": lambda: lib.mfhe_rns_bconv_reserve(h, 0, 3, 13, 2),
        "reserve overlap": lambda: lib.mfhe_rns_bconv_reserve(h, 0, 3, 2, 2),
        "moddown null": lambda: lib.mfhe_rns_moddown(h, None, 14 * nc, po, 11 * nc, 1, nc, 11, 11, 3, None),
        "moddown drop_start < keep": lambda: lib.mfhe_rns_moddown(h, pi, 14 * nc, po, 11 * nc, 1, nc, 11, 10, 3, None),
        "moddown drop outside": lambda: lib.mfhe_rns_moddown(h, pi, 14 * nc, po, 11 * nc, 1, nc, 11, 12, 3, None),
        "moddown in stride": lambda: lib.mfhe_rns_moddown(h, pi, 14 * nc - 1, po, 11 * nc, 1, nc, 11, 11, 3, None),
        "moddown out stride": lambda: lib.mfhe_rns_moddown(h, pi, 14 * nc, po, 11 * nc - 1, 1, nc, 11, 11, 3, None),
        "modup null": lambda: lib.mfhe_rns_modup(h, pi, 11 * nc, None, 14 * nc, 1, nc, 11, 0, 3, 11, 3, None),
        "modup level": lambda: lib.mfhe_rns_modup(h, pi, 11 * nc, po, 14 * nc, 1, nc, 15, 0, 3, 11, 3, None),
        "modup digit outside level": lambda: lib.mfhe_rns_modup(h, pi, 7 * nc, po, 10 * nc, 1, nc, 7, 6, 3, 11, 3, None),
        "modup special overlaps": lambda: lib.mfhe_rns_modup(h, pi, 11 * nc, po, 14 * nc, 1, nc, 11, 0, 3, 10, 3, None),
        "modup special outside": lambda: lib.mfhe_rns_modup(h, pi, 11 * nc, po, 14 * nc, 1, nc, 11, 0, 3, 12, 3, None),
        "modup out stride": lambda: lib.mfhe_rns_modup(h, pi, 11 * nc, po, 14 * nc - 1, 1, nc, 11, 0, 3, 11, 3, None),
    }
    for name, call in cases.items():
        assert call() == E, name
        assert lib.mfhe_last_error(), name
    # NTT-domain forms: no phantom tables in this context
    assert lib.mfhe_ntt_bconv_reserve(h, 1, 14) == mfhe.ENOTREADY
    assert lib.mfhe_ntt_modup(h, pi, 11 * 256, po, 14 * 256, 1, 11, 0, 3, 11, 3, None) == mfhe.ENOTREADY
    assert lib.mfhe_ntt_moddown(h, pi, 14 * 256, po, 11 * 256, 1, 11, 11, 3, None) == mfhe.ENOTREADY
    # and with them, the same argument checks
    moduli = _ntt_moduli(4, (45, 49))
    ctx = mfhe.Context(moduli, 4, mfhe.CONV_PHANTOM)
    hn, N = ctx.handle, 16
    big_in = _Buf(mfhe, 1, 7, N, 7 * N)
    big_out = _Buf(mfhe, 1, 7, N, 7 * N)
    qi, qo = big_in.t.data_ptr(), big_out.t.data_ptr()
    ntt_cases = {
        "ntt_modup null": lambda: lib.mfhe_ntt_modup(hn, None, 5 * N, qo, 7 * N, 1, 5, 0, 2, 5, 2, None),
        "ntt_modup digit": lambda: lib.mfhe_ntt_modup(hn, qi, 5 * N, qo, 7 * N, 1, 5, 4, 2, 5, 2, None),
        "ntt_modup special": lambda: lib.mfhe_ntt_modup(hn, qi, 5 * N, qo, 7 * N, 1, 5, 0, 2, 6, 2, None),
        "ntt_modup stride": lambda: lib.mfhe_ntt_modup(hn, qi, 5 * N - 1, qo, 7 * N, 1, 5, 0, 2, 5, 2, None),
        "ntt_moddown null": lambda: lib.mfhe_ntt_moddown(hn, qi, 7 * N, None, 5 * N, 1, 5, 5, 2, None),
        "ntt_moddown drop_start": lambda: lib.mfhe_ntt_moddown(hn, qi, 7 * N, qo, 5 * N, 1, 5, 4, 2, None),
        "ntt_moddown outside": lambda: lib.mfhe_ntt_moddown(hn, qi, 7 * N, qo, 5 * N, 1, 5, 6, 2, None),
        "ntt_moddown stride": lambda: lib.mfhe_ntt_moddown(hn, qi, 7 * N, qo, 5 * N - 1, 1, 5, 5, 2, None),
    }
    for name, call in ntt_cases.items():
        assert call() == E, name
    torch.cuda.synchronize()
    for b in (inp, out, big_in, big_out):   # nothing ran: every word is still the canary
        assert (mfhe.to_host_u64(b.full) == np.uint64(CANARY)).all()
