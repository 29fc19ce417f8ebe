"""Model of the CKKS slot encoder (include/mfhe.h mfhe_slot_encode / mfhe_slot_decode; no GPU, no product code).

N the ring degree, n = N / 2, zeta = e^(i pi / N), g_j = 5^j mod 2N.  Slot j of a real polynomial m is m(zeta^(g_j)).
    decode:  z_j = sum_k m_k zeta^(g_j k)                       (coeffs_to_slots; the caller divides by the scale)
    encode:  c_k = (2 / N) Re sum_j z_j zeta^(-g_j k), k < N    (slots_to_coeffs; the caller scales and rounds)
Every g_j is 1 mod 4 and j -> t_j = (g_j - 1) / 4 is a permutation of [0, n); with u_k = m_k + i m_(k+n) and w =
e^(2 pi i / n), m(zeta^(g_j)) = sum_k (u_k zeta^k) w^(k t_j): a twist, an n-point DFT and a gather by t_j.

Two precisions of the same two maps: np.clongdouble (a vectorised radix-2 FFT whose twiddles are cos / sin of
integer-reduced arguments; x87 extended precision, 63 fraction bits) is the truth that errors are measured from, and
plain float64 through np.fft is the reference that tolerances are multiples of.  definition_* are the O(N^2) sums."""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "slot_model needs an extended-precision longdouble"
_PI_LD = LD("3.14159265358979323846264338327950288")


@functools.lru_cache(maxsize=None)
def t_map(log_n):
    """t_j = (5^j mod 2N - 1) / 4 for j < n, as an int64 array."""
    N = 1 << log_n
    g, out = 1, np.empty(N // 2, dtype=np.int64)
    for j in range(N // 2):
        out[j] = (g - 1) >> 2
        g = g * 5 % (2 * N)
    return out


def _unit_ld(num, den):
    """e^(2 pi i num / den) in longdouble for integer arrays num (reduced mod den first; den a power of two >= 1)."""
    num = np.asarray(num, dtype=np.int64) % den
    ang = (LD(2) * _PI_LD) * num.astype(LD) / LD(den)   # below 2 pi, formed from exact integers
    return np.cos(ang) + 1j * np.sin(ang)


@functools.lru_cache(maxsize=None)
def _bitrev(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


@functools.lru_cache(maxsize=None)
def _roots_ld(n, sign):
    return _unit_ld(sign * np.arange(max(n // 2, 1)), n)


def fft_ld(x, sign):
    """X[t] = sum_k x[k] e^(sign 2 pi i k t / n) in clongdouble; n a power of two."""
    x = np.asarray(x, dtype=CLD)
    n = x.shape[0]
    if n == 1:
        return x.copy()
    a = x[_bitrev(n)].copy()
    w = _roots_ld(n, sign)
    size = 2
    while size <= n:
        half = size // 2
        tw = w[:: n // size][:half]
        a = a.reshape(n // size, size)
        lo, hi = a[:, :half], a[:, half:] * tw[None, :]
        a = np.concatenate([lo + hi, lo - hi], axis=1).reshape(n)
        size *= 2
    return a


def _as_ld(m):
    """Real numbers to longdouble; Python integers go through np.longdouble(int), which rounds once."""
    if isinstance(m, np.ndarray) and m.dtype != object:
        return m.astype(LD)
    return np.array([LD(int(v)) for v in m], dtype=LD)


def coeffs_to_slots(m, log_n):
    """z_j = m(zeta^(g_j)), unscaled, in clongdouble.  m: N real numbers (Python integers are converted exactly enough:
    through longdouble)."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    m = _as_ld(m)
    u = (m[:n] + 1j * m[n:]).astype(CLD) * _unit_ld(np.arange(n), 2 * N)
    return fft_ld(u, +1)[t_map(log_n)]


def slots_to_coeffs(z, log_n):
    """c_k = (2 / N) Re sum_j z_j zeta^(-g_j k), k < N, unscaled and unrounded, in longdouble."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    a = np.zeros(n, dtype=CLD)
    a[t_map(log_n)] = np.asarray(z).astype(CLD)
    u = fft_ld(a, -1) * _unit_ld(-np.arange(n), 2 * N) / LD(n)
    return np.concatenate([u.real, u.imag])


def coeffs_to_slots_f64(m, log_n):
    """coeffs_to_slots in plain float64 through np.fft: the reference tolerances are measured against."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    m = np.asarray(m, dtype=np.float64)
    u = (m[:n] + 1j * m[n:]) * np.exp(1j * np.pi * np.arange(n) / N)
    return (np.fft.ifft(u) * n)[t_map(log_n)]


def slots_to_coeffs_f64(z, log_n):
    """slots_to_coeffs in plain float64 through np.fft."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    a = np.zeros(n, dtype=np.complex128)
    a[t_map(log_n)] = np.asarray(z, dtype=np.complex128)
    u = np.fft.fft(a) * np.exp(-1j * np.pi * np.arange(n) / N) / n
    return np.concatenate([u.real, u.imag])


def definition_decode(m, log_n):
    """The O(N^2) sum z_j = sum_k m_k zeta^(g_j k) in clongdouble, exponents reduced mod 2N in integers."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    g = 4 * t_map(log_n) + 1
    e = (g[:, None] * np.arange(N)[None, :]) % (2 * N)
    return (_unit_ld(e, 2 * N) * _as_ld(m)[None, :]).sum(axis=1)


def definition_encode(z, log_n):
    """The O(N^2) sum c_k = (2 / N) Re sum_j z_j zeta^(-g_j k) in longdouble."""
    N, n = 1 << log_n, 1 << (log_n - 1)
    g = 4 * t_map(log_n) + 1
    e = (-(g[:, None] * np.arange(N)[None, :])) % (2 * N)
    return (LD(2) / LD(N)) * (_unit_ld(e, 2 * N) * np.asarray(z).astype(CLD)[:, None]).sum(axis=0).real


def garner_lift(r0, r1, q0, q1):
    """The centred value in (-q0 q1 / 2, q0 q1 / 2) of residues r0 mod q0 and r1 mod q1 (Python integers)."""
    h = (r1 - r0) * pow(q0, -1, q1) % q1
    x = r0 + q0 * h
    return x - q0 * q1 if x > (q0 * q1 - 1) // 2 else x


def center(r0, q0):
    return r0 - q0 if r0 > (q0 - 1) // 2 else r0


def encode_int(z, log_n, scale):
    """The integers the encoder should produce, from the longdouble model: rint(scale c_k) as Python integers, and the
    unrounded longdouble values."""
    c = slots_to_coeffs(z, log_n) * LD(scale)
    return [int(np.rint(v)) for v in c], c
