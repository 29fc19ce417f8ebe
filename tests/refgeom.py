"""Inputs and oracle products of the reference-geometry tests (n = 64, 512 lanes, the 11 reference moduli, delta 2^35):
tests/test_refgeom_cpu.py and tests/test_refgeom_gpu.py.  No GPU and no product code here.

The oracle is slow at this shape (seconds per W-CRT), so every product is computed once per process and kept in
_CACHE until drop() is called: the CPU module's preconditions and the GPU module's parity checks read the same arrays.
One [512][11][4096] u64 array is 184.5 MB; drop() what a test no longer needs.

Also here, for tests/test_cdft_gpu.py as well: residues() / lift() between centred integers and matrix-major residues
on any number of limbs."""
import numpy as np

import cdft_model as cm
from oracle import P, U64

RNS = [17592186435073, 17182765057, 17184541441, 17186120449, 17186515201, 17186909953,
       17188883713, 17190462721, 17190857473, 17191844353, 17192831233]
N, LOG_N, L, PHI = 64, 6, 11, 512
N2 = N * N
WORDS = PHI * L * N2
CONV = 1 | 4   # PHANTOM | WCRT
DELTA = 2.0 ** 35

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def drop(*prefixes):
    """Forget every cached product whose key starts with one of prefixes (all of them without arguments)."""
    for k in list(_CACHE):
        if not prefixes or any(k == p or (isinstance(k, tuple) and k[0] == p) for p in prefixes):
            del _CACHE[k]


def he(orc):
    """The oracle's pipeline context at the reference geometry."""
    return cached("he", lambda: orc.HE(N, RNS, DELTA))


def sk_ref(orc):
    return cached("sk", lambda: he(orc).keygen())


def wcrt_digits(q):
    """Balanced base-256 digits the W-CRT GEMM needs for q (ctx.cpp wcrt_digits, at least the 5 the kernels take)."""
    d, top = 1, 127
    while d < 9 and q - 1 > top:
        top = top * 256 + 127
        d += 1
    return max(d, 5)


# ---------------------------------------------------------------- integers <-> residues, any limb count
def residues(k, moduli):
    """[512][n^2] int64 -> matrix-major [512][L][n^2] residues k mod q_l, flat."""
    q = np.array(moduli, dtype=np.int64)[None, :, None]
    return np.mod(np.asarray(k, dtype=np.int64)[:, None, :], q).astype(np.uint64).ravel()


def lift(res, n, moduli):
    """Matrix-major residues [512][L][n^2] -> the centred integers (int64) of limb 0, checked on every other limb."""
    r = np.asarray(res).reshape(PHI, len(moduli), n * n).astype(np.int64)
    q0 = int(moduli[0])
    k = np.where(r[:, 0] > (q0 - 1) // 2, r[:, 0] - q0, r[:, 0])
    for l in range(1, len(moduli)):
        np.testing.assert_array_equal(np.mod(k, int(moduli[l])), r[:, l], err_msg=f"limb {l}")
    return k


def rand_residues(rng, shape_head, moduli, cols):
    """Uniform residues [*shape_head][L][cols] u64."""
    q = np.array(moduli, np.uint64)[None, :, None]
    return rng.integers(0, 2 ** 63, (shape_head, len(moduli), cols), dtype=np.uint64) % q


def sub_mod_poly(a, b, n, moduli):
    """(a - b) mod q_l elementwise on poly-major [512 n][L][n] arrays of canonical residues."""
    q = np.array(moduli, np.uint64)[None, :, None]
    a3, b3 = a.reshape(-1, len(moduli), n), b.reshape(-1, len(moduli), n)
    return np.where(a3 >= b3, a3 - b3, a3 + q - b3).ravel()


# ---------------------------------------------------------------- the encrypt's noise: distance from a rounding tie
def splitmix64(x):
    """orc_splitmix64 on a uint64 array (wrapping arithmetic)."""
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_samples(n):
    """The unrounded Box-Muller samples z of the 512 n^2 noise draws (oracle orc_gaussian_noise, HE.cu:581-627): draw
    id = w n^2 + pos, the same in every limb."""
    ids = np.arange(PHI * n * n, dtype=np.uint64)
    r1 = splitmix64(np.uint64(0xD6E8FEB86659FD93) ^ ids)
    r2 = splitmix64(r1)
    inv53 = 1.0 / 9007199254740992.0
    u1 = ((r1 >> np.uint64(11)).astype(np.float64) + 1.0) * inv53
    u2 = ((r2 >> np.uint64(11)).astype(np.float64) + 1.0) * inv53
    return 3.2 * np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def noise_tie_distance(n):
    """(min over the draws of | |z| mod 1 - 0.5 |, its id, its z): how far the draw nearest a llround tie is from it."""
    z = noise_samples(n)
    d = np.abs(np.abs(z) % 1.0 - 0.5)
    i = int(np.argmin(d))
    return float(d[i]), i, float(z[i])


# ---------------------------------------------------------------- W-CRT inputs and oracle outputs
def wcrt_products(orc):
    """x (random residues, lane w = 0 all q - 1), xp (random, poly-major, its first n polynomials all q - 1), v (vector
    layout) and the oracle's forward of x, inverse of xp and vector forward of v."""
    def make():
        h = he(orc)
        rng = np.random.default_rng(6411)
        qv = np.array(RNS, np.uint64)
        x = rand_residues(rng, PHI, RNS, N2)
        x[0] = (qv - np.uint64(1))[:, None]
        x = x.ravel()
        xp = rand_residues(rng, PHI * N, RNS, N)
        xp[:N] = (qv - np.uint64(1))[None, :, None]
        xp = xp.ravel()
        v = rand_residues(rng, PHI, RNS, N).ravel()
        m = P(U64(RNS))
        ref_f, ref_b2, ref_v = np.zeros_like(x), np.zeros_like(xp), np.zeros_like(v)
        orc.L.orc_wntt_forward_matrix(P(x), P(ref_f), N, L, PHI, m, orc.L.orc_he_V(h.h))
        orc.L.orc_wntt_inverse_matrix(P(xp), P(ref_b2), N, L, PHI, m, orc.L.orc_he_VinvT(h.h))
        orc.L.orc_wntt_forward_vector(P(v), P(ref_v), N, L, PHI, m, orc.L.orc_he_V(h.h))
        return dict(x=x, xp=xp, v=v, ref_f=ref_f, ref_b2=ref_b2, ref_v=ref_v)
    return cached("wcrt", make)


# ---------------------------------------------------------------- ciphertexts of planted integers
def check_lanes():
    return cm.xy_check_lanes(PHI, N)


def planted_ct(orc, bits):
    """Ciphertexts whose decrypted coefficients are exactly the integers k_re, k_im, uniform in (-2^bits, 2^bits):
        ev = orc_wntt_forward_matrix(k mod q)      (poly-major, what a decrypt returns)
        a  = random residues, matrix-major, shared by both ciphertexts
        t  = decrypt_to_eval([0 | a], sk) = a s    b = poly_to_matrix(ev - t mod q)     ct = [b | a],
    so b + a s = ev.  With them: the model's message on the checked lanes (truth), the oracle's decode of ev on those
    lanes (ref), its error E_ref against the model, E_best (numpy complex128 on the model's tables rounded once to
    double) and S (cdft_model.decode_scale)."""
    def make():
        h, sk = he(orc), sk_ref(orc)
        rng = np.random.default_rng(7000 + bits)
        k_re, k_im = (rng.integers(-2 ** bits + 1, 2 ** bits, (PHI, N2), dtype=np.int64) for _ in range(2))
        a = rand_residues(rng, PHI, RNS, N2).ravel()
        t = h.decrypt_to_eval(np.concatenate([np.zeros_like(a), a]), sk)
        m = P(U64(RNS))
        out = dict(k_re=k_re, k_im=k_im)
        for part, k in (("re", k_re), ("im", k_im)):
            ev = np.zeros(WORDS, np.uint64)
            orc.L.orc_wntt_forward_matrix(P(residues(k, RNS)), P(ev), N, L, PHI, m, orc.L.orc_he_V(h.h))
            bp, b = sub_mod_poly(ev, t, N, RNS), np.zeros(WORDS, np.uint64)
            orc.L.orc_poly_to_matrix(P(bp), P(b), N, L, PHI)
            out["ev_" + part], out["ct_" + part] = ev, np.concatenate([b, a])
        lanes = check_lanes()
        out["lanes"] = lanes
        out["truth"] = cm.decode_truth(k_re, k_im, N, DELTA, lanes)
        out["ref"] = h.decode(out["ev_re"], out["ev_im"]).reshape(PHI, N, N)[lanes]
        out["e_ref"] = cm.err(out["ref"], out["truth"])
        kc = (k_re.astype(np.float64) + 1j * k_im.astype(np.float64)) / DELTA   # E_best: numpy on tables rounded once
        V = cm.xy_table(N).astype(np.complex128)
        best = np.stack([V @ m.reshape(N, N) @ V.T for m in cm._w_tables_f64()[0][lanes] @ kc])
        out["e_best"] = cm.err(best, out["truth"])
        out["scale"] = cm.decode_scale(k_re, k_im, DELTA)
        return out
    return cached(("planted_ct", bits), make)


# ---------------------------------------------------------------- a message that encodes to planted integers
def planted_positions():
    """The columns p = 64 y + x that carry a planted value: the whole rows y = 0 and y = 63, and 15 seeded columns of
    every other row (so every aligned run of 64 holds at least one): 1058 of the 4096, sorted."""
    rng = np.random.default_rng(8064)
    cols = set(range(N)) | set(range(N2 - N, N2))
    for y in range(1, N - 1):
        cols |= {y * N + int(x) for x in rng.choice(N, 15, replace=False)}
    return np.array(sorted(cols), dtype=np.int64)


def planted_message(orc, k_bits=30):
    """msg = xy_dft(wdft_fwd(c)) by the long-double model, rounded to double, for c = (k + f) / delta on
    planted_positions() (|k| < 2^k_bits, f uniform in [-0.4, 0.4]) and exactly 0 elsewhere; with it the encode
    precondition: the largest |delta wc - (k + f)| over all 512 x 4096 coefficients, wc the oracle's float64 stages
    (two orc_cmatmul per lane, orc_w_idft) on msg."""
    def make():
        rng = np.random.default_rng(8000 + k_bits)
        cols = planted_positions()
        shape = (PHI, cols.size)
        kr, ki = (rng.integers(-2 ** k_bits + 1, 2 ** k_bits, shape, dtype=np.int64) for _ in range(2))
        fr, fi = (rng.uniform(-0.4, 0.4, shape) for _ in range(2))
        c = ((kr.astype(cm.LD) + fr.astype(cm.LD)) + 1j * (ki.astype(cm.LD) + fi.astype(cm.LD))) / cm.LD(DELTA)
        ev = np.zeros((PHI, N2), dtype=cm.CLD)
        ev[:, cols] = cm.w_table() @ c.astype(cm.CLD)   # the other columns of c are zero, so are those of ev
        V = cm.xy_table(N)
        msg = np.stack([V @ m.reshape(N, N) @ V.T for m in ev]).astype(np.complex128)
        k_re, k_im, kf_re, kf_im = (np.zeros((PHI, N2), dtype=t) for t in (np.int64, np.int64, np.float64, np.float64))
        k_re[:, cols], k_im[:, cols] = kr, ki
        kf_re[:, cols], kf_im[:, cols] = kr + fr, ki + fi
        xy = cm.orc_xy(orc, msg, N, np.arange(PHI), True).reshape(PHI, N2)
        wc = cm.orc_wdft(orc, xy, np.arange(N2), True)
        pre_err = float(max(np.max(np.abs(DELTA * wc.real - kf_re)), np.max(np.abs(DELTA * wc.imag - kf_im))))
        return dict(cols=cols, k_re=k_re, k_im=k_im, msg=msg, pre_err=pre_err, k_bits=k_bits)
    return cached(("planted_msg", k_bits), make)
