"""Model of the FP64 matrix codec's transforms (csrc/cdft.hip, csrc/wtrans.hip; no GPU, no product code).

W axis.  Output w = 256 (a - 1) + (b - 1), a in {1, 2}, b in [1, 256], has exponent e_w = (257 a + 3 b) mod 771; the
e_w are the 512 units of Z_771 and zeta = e^(2 pi i / 771).  On [512][P] interleaved complex columns
    wdft_fwd:  out[w][p] = sum_(r < 512) zeta^((e_w r) mod 771) in[r][p]           (V, 512 x 512)
    wdft_inv:  the inverse of that map                                              (V^-1)
XY axes.  g_j = 5^j mod 4n, xi = e^(2 pi i / 4n), V[j][k] = xi^((g_j k) mod 4n), V^-1 = V^H / n.  On [lanes][n][n]
    xy_dft(M) = V M V^T,   xy_idft(M) = V^-1 M V^-T                                 (per lane)

Precision, as in slot_model.py: np.clongdouble (x87 extended, 63 fraction bits) is the truth that errors are measured
from.  pi comes from a decimal string, every root is cos / sin of one angle formed from exact reduced integers, and
every table is indexed by an integer exponent: no repeated products.  *_f64 are the same tables rounded once to double
and multiplied by numpy in complex128: the best a float64 routine can be expected to do (E_best).

V^-1 of the W axis is not computed by elimination.  The polynomial f of degree < 512 with f(zeta^(e_w)) = y_w is
g mod Phi_771, g the degree < 771 interpolant through y_w at the units and 0 at the 259 non-units of Z_771:
g_j = (1 / 771) sum_w y_w zeta^(-e_w j).  With x^j = sum_r R[r][j] x^r mod Phi_771 (R integer, exact),
    V^-1[r][w] = (1 / 771) (zeta^(-e_w r) + sum_(512 <= j < 771) R[r][j] zeta^(-e_w j)),
one long-double sum of exactly known terms per entry.  Computed once per process and cached.

The *_eref helpers run the oracle's float64 routines (tests/oracle.py, passed in by the caller) on the same doubles
and return their max-abs error against this model: E_ref, the unit of the bounds in test_cdft_gpu.py."""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "cdft_model needs an extended-precision longdouble"
_PI_LD = LD("3.14159265358979323846264338327950288")
PHI = 512
U53 = 2.0 ** -53


def unit_ld(num, den):
    """e^(2 pi i num / den) in clongdouble for integer arrays num: reduced into (-den / 2, den / 2] first, so the
    angle is formed from exact integers and lies in (-pi, pi]."""
    num = np.asarray(num, dtype=np.int64) % den
    num = np.where(2 * num > den, num - den, num)
    ang = (LD(2) * _PI_LD) * num.astype(LD) / LD(den)
    return (np.cos(ang) + 1j * np.sin(ang)).astype(CLD)


# ---------------------------------------------------------------- W axis
@functools.lru_cache(maxsize=None)
def w_exponents():
    """e_w = (257 a + 3 b) mod 771 at w = 256 (a - 1) + (b - 1)."""
    return np.array([(257 * a + 3 * b) % 771 for a in (1, 2) for b in range(1, 257)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def w_roots():
    """zeta^e for e < 771: the one root table every W entry is read from."""
    return unit_ld(np.arange(771), 771)


@functools.lru_cache(maxsize=None)
def w_table():
    """V[w][r] = zeta^((e_w r) mod 771), [512][512] clongdouble."""
    e = (w_exponents()[:, None] * np.arange(PHI)[None, :]) % 771
    return w_roots()[e]


@functools.lru_cache(maxsize=None)
def phi771():
    """Phi_771 = (x^514 + x^257 + 1) / (x^2 + x + 1) as 513 Python integers, lowest degree first."""
    num = [0] * 515
    num[0] = num[257] = num[514] = 1
    quo = [0] * 513
    for d in range(514, 1, -1):
        c = num[d]
        quo[d - 2] = c
        num[d] -= c
        num[d - 1] -= c
        num[d - 2] -= c
    assert not any(num) and quo[512] == 1
    return quo


@functools.lru_cache(maxsize=None)
def w_reduction():
    """R[r][j - 512] for 512 <= j < 771: x^j = sum_r R[r][j] x^r mod Phi_771, exact int64."""
    phi = np.array(phi771()[:PHI], dtype=np.int64)
    cur = -phi                       # x^512
    out = np.empty((PHI, 771 - PHI), dtype=np.int64)
    for j in range(PHI, 771):
        out[:, j - PHI] = cur
        top = cur[PHI - 1]
        cur = np.concatenate([[0], cur[:-1]]) - top * phi   # times x, reduced
    assert np.max(np.abs(out)) < 2 ** 20
    return out


@functools.lru_cache(maxsize=None)
def w_inverse():
    """V^-1[r][w], [512][512] clongdouble (see the module docstring)."""
    e = w_exponents()
    lo = w_roots()[(-(np.arange(PHI)[:, None] * e[None, :])) % 771]                 # zeta^(-e_w r), [r][w]
    hi = w_roots()[(-(np.arange(PHI, 771)[:, None] * e[None, :])) % 771]            # zeta^(-e_w j), [j][w]
    R = w_reduction().astype(LD)
    return ((lo + (R @ hi.real.copy() + 1j * (R @ hi.imag.copy()))) / LD(771)).astype(CLD)


def _cols(x, cols):
    """Columns cols of a [512][P] complex (or interleaved float64 [512 * P * 2]) array, as clongdouble."""
    x = np.asarray(x)
    if x.dtype == np.float64:
        x = x.view(np.complex128)
    x = x.reshape(PHI, -1)
    return x[:, np.asarray(cols, dtype=np.int64)].astype(CLD)


def wdft_fwd(x, cols, rows=None):
    """out[w][i] = sum_r V[w][r] x[r][cols[i]] for w in rows (default: all), clongdouble."""
    V = w_table() if rows is None else w_table()[np.asarray(rows, dtype=np.int64)]
    return V @ _cols(x, cols)


def wdft_inv(y, cols):
    """out[r][i] = sum_w V^-1[r][w] y[w][cols[i]], clongdouble."""
    return w_inverse() @ _cols(y, cols)


def w_fwd_scale(x, cols):
    """S of the forward: sum_r |x[r][p]| per checked column (|V| = 1), the same for every output row."""
    return np.abs(_cols(x, cols)).sum(axis=0).astype(np.float64)[None, :]


def w_inv_scale(y, cols):
    """S of the inverse: sum_w |V^-1[r][w]| |y[w][p]|, [512][len(cols)]."""
    return (np.abs(w_inverse()) @ np.abs(_cols(y, cols))).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _w_tables_f64():
    return w_table().astype(np.complex128), w_inverse().astype(np.complex128)


def wdft_fwd_f64(x, cols):
    return _w_tables_f64()[0] @ _cols(x, cols).astype(np.complex128)


def wdft_inv_f64(y, cols):
    return _w_tables_f64()[1] @ _cols(y, cols).astype(np.complex128)


def w_check_columns(P, seed=0):
    """The columns the model checks at n^2 = P (at most 96): 0, 1, 2, 31-33, 62-65, P / 2 - 1, P / 2, the four
    columns 66 ... 63 from the end, P - 2, P - 1 (each where inside [0, P)), and 32 seeded random ones."""
    fixed = [0, 1, 2, 31, 32, 33, 62, 63, 64, 65, P // 2 - 1, P // 2, P - 66, P - 65, P - 64, P - 63, P - 2, P - 1]
    cols = {c for c in fixed if 0 <= c < P}
    rng = np.random.default_rng(1000 + seed)
    cols |= {int(c) for c in rng.integers(0, P, 32)}
    out = np.array(sorted(cols), dtype=np.int64)
    assert out.size <= 96
    return out


def w_impulse_shifts(P, cols):
    """Shifts s for the impulse class (column p holds a single 1 at row (p + s) mod 512), chosen greedily until the
    checked columns have hit every row 0 ... 511."""
    cols = np.asarray(cols, dtype=np.int64)
    hit = np.zeros(PHI, dtype=bool)
    rows = (cols[None, :] + np.arange(PHI)[:, None]) % PHI     # [s][checked column]
    shifts = []
    while not hit.all():
        s = int(np.argmax((~hit[rows]).sum(axis=1)))           # the shift that hits the most new rows
        hit[rows[s]] = True
        shifts.append(s)
    return shifts


def w_input(kind, P, seed, shift=0):
    """[512][P] complex128 input of class (a) 'normal', (b) 'impulse' or (c) 'range' (standard normal rows scaled by
    2^(-40 r / 511))."""
    if kind == "impulse":
        x = np.zeros((PHI, P), dtype=np.complex128)
        p = np.arange(P)
        x[(p + shift) % PHI, p] = 1.0
        return x
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((PHI, P)) + 1j * rng.standard_normal((PHI, P))
    if kind == "range":
        x = x * np.exp2(-40.0 * np.arange(PHI) / 511.0)[:, None]
    else:
        assert kind == "normal"
    return x


# ---------------------------------------------------------------- XY axes
@functools.lru_cache(maxsize=None)
def xy_exponents(n):
    """g_j = 5^j mod 4n, j < n."""
    g, out = 1, np.empty(n, dtype=np.int64)
    for j in range(n):
        out[j] = g
        g = g * 5 % (4 * n)
    return out


@functools.lru_cache(maxsize=None)
def xy_table(n):
    """V[j][k] = xi^((g_j k) mod 4n), [n][n] clongdouble."""
    e = (xy_exponents(n)[:, None] * np.arange(n)[None, :]) % (4 * n)
    return unit_ld(e, 4 * n)


@functools.lru_cache(maxsize=None)
def xy_inverse(n):
    """V^-1 = V^H / n; every entry again cos / sin of one reduced angle, divided by the power of two n."""
    e = (-(np.arange(n)[:, None] * xy_exponents(n)[None, :])) % (4 * n)
    return unit_ld(e, 4 * n) / LD(n)


def _lanes(M, n, lanes):
    M = np.asarray(M)
    if M.dtype == np.float64:
        M = M.view(np.complex128)
    return M.reshape(-1, n, n)[np.asarray(lanes, dtype=np.int64)].astype(CLD)


def xy_dft(M, n, lanes):
    """V M_l V^T for l in lanes, [len(lanes)][n][n] clongdouble."""
    V = xy_table(n)
    return np.stack([V @ m @ V.T for m in _lanes(M, n, lanes)])


def xy_idft(M, n, lanes):
    """V^-1 M_l V^-T for l in lanes."""
    Vi = xy_inverse(n)
    return np.stack([Vi @ m @ Vi.T for m in _lanes(M, n, lanes)])


def xy_dft_f64(M, n, lanes):
    V = xy_table(n).astype(np.complex128)
    return np.stack([V @ m @ V.T for m in _lanes(M, n, lanes).astype(np.complex128)])


def xy_idft_f64(M, n, lanes):
    Vi = xy_inverse(n).astype(np.complex128)
    return np.stack([Vi @ m @ Vi.T for m in _lanes(M, n, lanes).astype(np.complex128)])


def xy_scale(M, n, lanes, inverse):
    """S of the XY forms: sum_(y, x) |M_l[y][x]| per lane (|V| = 1), times 1 / n^2 for the idft."""
    s = np.abs(_lanes(M, n, lanes)).sum(axis=(1, 2)).astype(np.float64)
    return (s / (n * n) if inverse else s)[:, None, None]


def xy_check_lanes(lanes, seed=0):
    """The first lane, the last lane and up to 6 seeded random lanes."""
    rng = np.random.default_rng(2000 + seed)
    pick = {0, lanes - 1} | {int(v) for v in rng.integers(0, lanes, 6)}
    return np.array(sorted(pick), dtype=np.int64)


def xy_input(kind, n, lanes, seed, shift=0):
    """[lanes][n][n] complex128 of class (a) 'normal' or (b) 'impulse': lane l holds a single 1 at flat position
    (l + shift) mod n^2."""
    if kind == "impulse":
        M = np.zeros((lanes, n * n), dtype=np.complex128)
        l = np.arange(lanes)
        M[l, (l + shift) % (n * n)] = 1.0
        return M.reshape(lanes, n, n)
    assert kind == "normal"
    rng = np.random.default_rng(seed)
    return rng.standard_normal((lanes, n, n)) + 1j * rng.standard_normal((lanes, n, n))


# ---------------------------------------------------------------- the codec's FP path on exact integers
def decode_truth(k_re, k_im, n, delta, lanes):
    """xy_dft(wdft_fwd(k)) / delta for lanes of the output, from integer coefficients k[r][p] (int64 arrays
    [512][n^2], below 2^63 in magnitude so the conversion to longdouble is exact)."""
    k = np.asarray(k_re).reshape(PHI, -1).astype(LD) + 1j * np.asarray(k_im).reshape(PHI, -1).astype(LD)
    lanes = np.asarray(lanes, dtype=np.int64)
    ev = w_table()[lanes] @ k.astype(CLD)
    V = xy_table(n)
    return np.stack([V @ m.reshape(n, n) @ V.T for m in ev]) / LD(delta)


def decode_scale(k_re, k_im, delta):
    """S of the decode: every weight has unit modulus, so sum_(r, p) |k[r][p]| / delta feeds every output."""
    k = np.asarray(k_re).astype(LD) + 1j * np.asarray(k_im).astype(LD)
    return float(np.abs(k).sum() / LD(delta))


# ---------------------------------------------------------------- the reference's own error, E_ref
def bound(e_ref, scale):
    """The one bound of test_cdft_gpu.py: 4 E_ref + 8 * 2^-53 * S, S the largest scale over the checked outputs."""
    return 4.0 * e_ref + 8.0 * U53 * float(np.max(scale))


def err(got, truth):
    """max |got - truth| with the difference taken in clongdouble."""
    return float(np.max(np.abs(np.asarray(got).astype(CLD) - truth)))


class Report:
    """Collects the lines of one test; fails after all of them are printed."""

    def __init__(self):
        self.bad = []

    def line(self, what, kind, n, mode, e_gpu, e_ref, e_best, scale, e_ref_name="E_ref"):
        bnd = bound(e_ref, scale)
        ratio = e_gpu / e_ref if e_ref > 0 else float("inf") if e_gpu > 0 else 0.0
        best = e_gpu / e_best if e_best > 0 else float("inf") if e_gpu > 0 else 0.0
        print(f"CDFT | {what:<14s} | {kind:<7s} | n={n:<3d} | mode {mode} | E_gpu {e_gpu:.3e} | {e_ref_name} {e_ref:.3e} | "
              f"ratio {ratio:8.3f} | E_gpu/E_best {best:9.3f} | bound {bnd:.3e} | {'ok' if e_gpu <= bnd else 'OVER'}")
        if not e_gpu <= bnd:
            self.bad.append((what, kind, n, mode, e_gpu, bnd))

    def check(self):
        assert not self.bad, self.bad


@functools.lru_cache(maxsize=None)
def _orc_w_tables(orc):
    from oracle import P
    V = np.zeros(PHI * PHI * 2)
    ViT = np.zeros(PHI * PHI * 2)
    assert orc.L.orc_wdft_tables(P(V), P(ViT)) == 0
    return V, ViT


def orc_wdft(orc, x, cols, inverse):
    """The oracle's float64 W transform (orc_wdft_forward / orc_w_idft) of columns cols of x, [512][len(cols)]: it
    works column by column, so it is handed the checked columns alone."""
    from oracle import P
    V, ViT = _orc_w_tables(orc)
    xc = np.ascontiguousarray(_cols(x, cols).astype(np.complex128))
    out = np.zeros(xc.size * 2)
    if inverse:
        orc.L.orc_w_idft(P(xc), P(out), P(ViT), xc.shape[1], PHI)
    else:
        orc.L.orc_wdft_forward(P(xc), P(out), P(V), xc.shape[1], PHI)
    return out.view(np.complex128).reshape(PHI, -1)


@functools.lru_cache(maxsize=None)
def _orc_xy_tables(orc, n):
    from oracle import P
    t = [np.zeros(n * n * 2) for _ in range(4)]
    orc.L.orc_encoder_matrices(n, *[P(a) for a in t])
    return t   # V, VT, Vinv, VinvT


def orc_xy(orc, M, n, lanes, inverse):
    """The oracle's float64 XY transform of lanes of M: two orc_cmatmul per lane (encoder.cu:460-467, 492-501)."""
    from oracle import P
    V, VT, Vi, ViT = _orc_xy_tables(orc, n)
    A, B = (Vi, ViT) if inverse else (V, VT)
    out = []
    for m in _lanes(M, n, lanes).astype(np.complex128):
        m = np.ascontiguousarray(m)
        T, R = np.zeros(n * n * 2), np.zeros(n * n * 2)
        orc.L.orc_cmatmul(P(A), P(m), P(T), n)
        orc.L.orc_cmatmul(P(T), P(B), P(R), n)
        out.append(R.view(np.complex128).reshape(n, n))
    return np.stack(out)


def w_eref(orc, x, cols, inverse, truth=None):
    """E_ref of a W transform: max |oracle - model| over the checked columns of x."""
    if truth is None:
        truth = (wdft_inv if inverse else wdft_fwd)(x, cols)
    return err(orc_wdft(orc, x, cols, inverse), truth)


def xy_eref(orc, M, n, lanes, inverse, truth=None):
    """E_ref of an XY transform: max |oracle - model| over the checked lanes of M."""
    if truth is None:
        truth = (xy_idft if inverse else xy_dft)(M, n, lanes)
    return err(orc_xy(orc, M, n, lanes, inverse), truth)
