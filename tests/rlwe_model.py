"""A Python restatement of csrc/rlwe_draw.hpp, the seeded draws of the RLWE client side (include/mfhe.h mfhe_rlwe_*):
the ChaCha20 block function of RFC 8439 section 2.3 on numpy uint32 arrays (one lane per block counter), the nonce
layout, and the maps from a block's words to a uniform residue, a ternary digit and a centred-binomial noise value.
Written from the RFC and the header's comment, not from the header's code."""
import numpy as np

MASK, NOISE, SECRET, EPHEMERAL, NOISE0, NOISE1 = 1, 2, 3, 4, 5, 6
SMALL_STREAMS = (NOISE, SECRET, EPHEMERAL, NOISE0, NOISE1)
TERNARY_STREAMS = (SECRET, EPHEMERAL)
NOISE_BITS = 21
NOISE_VARIANCE = 2 * NOISE_BITS / 4          # 42 fair bits, half of them subtracted: 42 / 4 = 10.5
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)   # "expand 32-byte k"


def seed_words(key: bytes):
    """The eight little-endian key words of a 32-byte seed."""
    assert len(key) == 32
    return [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _quarter(x, a, b, c, d):
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_blocks(key_words, counters, nonce_words):
    """out [len(counters)][16] uint32: the ChaCha20 block of every 32-bit counter under one key and nonce.  A nonce word
    may also be an array with one entry per counter: every lane then has its own nonce (small_values_ids and
    mask_residues_ids below draw all their (id, counter) pairs in one call this way)."""
    counters = np.asarray(counters, dtype=np.uint64)
    assert (counters < (1 << 32)).all()
    n = len(counters)
    assert all(np.ndim(v) == 0 or np.shape(v) == (n,) for v in nonce_words)
    const = [np.full(n, v, dtype=np.uint32) for v in SIGMA + tuple(key_words)]
    init = const + [counters.astype(np.uint32)] + [np.full(n, v, dtype=np.uint32) for v in nonce_words]
    x = [v.copy() for v in init]
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return np.stack([a + b for a, b in zip(x, init)], axis=1)


def nonce(stream, limb, pid):
    assert 0 <= pid < 1 << 64 and 0 <= stream < 256
    return [(stream | (limb << 8)) & 0xFFFFFFFF, pid & 0xFFFFFFFF, pid >> 32]


def mask_words(key_words, limb, pid, n):
    """The n 128-bit integers (Python ints) of the mask of (limb, polynomial id), before the reduction."""
    out = chacha20_blocks(key_words, np.arange((n + 3) // 4), nonce(MASK, limb, pid)).astype(object)
    w = out.reshape(-1, 4, 4)
    v = w[:, :, 0] | (w[:, :, 1] << 32) | (w[:, :, 2] << 64) | (w[:, :, 3] << 96)
    return v.reshape(-1)[:n]


def mask_residues(key_words, limb, pid, n, q):
    return np.array([int(v) % q for v in mask_words(key_words, limb, pid, n)], dtype=np.uint64)


def small_words(key_words, stream, pid, n):
    """The n 64-bit words (uint64) of a small stream's polynomial."""
    out = chacha20_blocks(key_words, np.arange((n + 7) // 8), nonce(stream, 0, pid)).astype(np.uint64)
    w = out.reshape(-1, 8, 2)
    return (w[:, :, 0] | (w[:, :, 1] << np.uint64(32))).reshape(-1)[:n]


def ternary(w):
    """floor(3 w / 2^64) - 1"""
    return np.array([(3 * int(v) >> 64) - 1 for v in np.asarray(w).ravel()], dtype=np.int64)


def noise(w):
    """popcount(w & (2^21 - 1)) - popcount((w >> 21) & (2^21 - 1))"""
    m = (1 << NOISE_BITS) - 1
    return np.array([bin(int(v) & m).count("1") - bin((int(v) >> NOISE_BITS) & m).count("1")
                     for v in np.asarray(w).ravel()], dtype=np.int64)


def small_values(key_words, stream, pid, n):
    """The n small integers of (stream, polynomial id): ternary for SECRET and EPHEMERAL, noise otherwise."""
    assert stream in SMALL_STREAMS
    w = small_words(key_words, stream, pid, n)
    return ternary(w) if stream in TERNARY_STREAMS else noise(w)


def _id_lanes(first_word, ids, nblocks):
    """(counters, nonce words) of nblocks blocks of every id, id-major: one lane per (id, counter) pair."""
    ids = [int(i) for i in ids]
    assert all(0 <= i < 1 << 64 for i in ids)
    lo = np.repeat(np.array([i & 0xFFFFFFFF for i in ids], dtype=np.uint32), nblocks)
    hi = np.repeat(np.array([i >> 32 for i in ids], dtype=np.uint32), nblocks)
    return np.tile(np.arange(nblocks, dtype=np.uint64), len(ids)), [first_word, lo, hi]


def small_values_ids(key_words, stream, ids, n):
    """[len(ids)][n] int64: small_values of every id, from one ChaCha call over all (id, counter) pairs and the two
    maps restated on uint64 arrays (tests/test_rlwe_cpu.py compares it with the per-id function)."""
    assert stream in SMALL_STREAMS
    nb = (n + 7) // 8
    counters, nw = _id_lanes(nonce(stream, 0, 0)[0], ids, nb)
    out = chacha20_blocks(key_words, counters, nw).astype(np.uint64).reshape(len(ids), nb * 8, 2)
    lo, hi = out[:, :n, 0], out[:, :n, 1]
    if stream in TERNARY_STREAMS:
        # floor(3 w / 2^64) with w = 2^32 hi + lo: 3 hi + floor(3 lo / 2^32) is below 2^34
        three = np.uint64(3)
        return (((three * hi + ((three * lo) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64) - 1)
    w = lo | (hi << np.uint64(32))
    one = np.uint64(1)
    v = np.zeros(w.shape, dtype=np.int64)
    for k in range(NOISE_BITS):
        v += ((w >> np.uint64(k)) & one).astype(np.int64) - ((w >> np.uint64(NOISE_BITS + k)) & one).astype(np.int64)
    return v


def mask_residues_ids(key_words, limb, ids, n, q):
    """[len(ids)][n] uint64: mask_residues of every id, from one ChaCha call over all (id, counter) pairs."""
    nb = (n + 3) // 4
    counters, nw = _id_lanes(nonce(MASK, limb, 0)[0], ids, nb)
    w = chacha20_blocks(key_words, counters, nw).astype(object).reshape(len(ids), nb * 4, 4)[:, :n]
    v = w[:, :, 0] | (w[:, :, 1] << 32) | (w[:, :, 2] << 64) | (w[:, :, 3] << 96)
    return (v % int(q)).astype(np.uint64)


def row_limbs(level, special_start, nspecial):
    return list(range(level)) + list(range(special_start, special_start + nspecial))


def uniform_rows(key_words, first_id, npoly, limbs, moduli, n):
    """[npoly][len(limbs)][n] uint64: mfhe_rlwe_sample_uniform."""
    return np.stack([np.stack([mask_residues(key_words, l, (first_id + p) % (1 << 64), n, int(moduli[l])) for l in limbs])
                     for p in range(npoly)])


def small_rows(values, limbs, moduli):
    """The residues of small integers [npoly][n] on every row: [npoly][len(limbs)][n] uint64 (v or q + v)."""
    v = np.asarray(values).astype(object)
    return np.stack([np.stack([(p % int(moduli[l])) for l in limbs]) for p in v]).astype(np.uint64)


def small_coeff_rows(key_words, stream, first_id, npoly, limbs, moduli, n):
    """[npoly][rows][n]: mfhe_rlwe_sample_small with MFHE_RLWE_COEFF; also returns the integers [npoly][n]."""
    vals = np.stack([small_values(key_words, stream, (first_id + p) % (1 << 64), n) for p in range(npoly)])
    return small_rows(vals, limbs, moduli), vals
