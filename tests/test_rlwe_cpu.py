"""CPU checks of csrc/rlwe_draw.hpp, the seeded draws of the RLWE client side (include/mfhe.h mfhe_rlwe_*):
tests/rlwe_model.py (a Python restatement of RFC 8439's block function and of the draws) against the RFC's vector and
the local OpenSSL, tests/cpp/rlwe_draw_main.cpp (the header alone, host compiler, address and undefined-behaviour
sanitizers) against the model, the distributions of the small draws against their definitions, and the C ABI's new
symbols."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rlwe_model as rm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matrix-fhe-gpu_amd" / "csrc"
KEY = bytes(range(32))
KW = rm.seed_words(KEY)
SYMBOLS = ["mfhe_rlwe_reserve", "mfhe_rlwe_sample_uniform", "mfhe_rlwe_sample_small", "mfhe_rlwe_lift_small",
           "mfhe_rlwe_encrypt_sk", "mfhe_rlwe_ksk_gen", "mfhe_rlwe_encrypt_pk", "mfhe_rlwe_decrypt"]


def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return cc
    llvm = Path("/opt/rocm/lib/llvm/bin/clang++")
    return str(llvm) if llvm.exists() else None


# ---------------------------------------------------------------------------------------------------------------
# 1. the block function
# ---------------------------------------------------------------------------------------------------------------
def test_block_function_equals_rfc_8439():
    """RFC 8439 2.3.2: key bytes 00..1f, counter 1, nonce words (0x09000000, 0x4a000000, 0)."""
    out = rm.chacha20_blocks(KW, [1], [0x09000000, 0x4A000000, 0])[0]
    assert [int(v) for v in out[:4]] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3]


def _openssl_keystream(counter, nonce_words, nbytes):
    iv = b"".join(int(w).to_bytes(4, "little") for w in [counter] + list(nonce_words))
    r = subprocess.run(["openssl", "enc", "-chacha20", "-K", KEY.hex(), "-iv", iv.hex()], input=bytes(nbytes),
                       capture_output=True)
    assert r.returncode == 0, r.stderr[-500:]
    return r.stdout


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on the PATH")
def test_block_function_and_nonce_layout_equal_openssl():
    """The RFC's vector and the header's nonce layout (stream 1, limb 3, id 2^32 - 1, counter 5; two blocks, so the
    counter's increment too) against `openssl enc -chacha20` with -iv = counter || nonce, little-endian."""
    for counter, nw in ((1, [0x09000000, 0x4A000000, 0]), (5, rm.nonce(rm.MASK, 3, (1 << 32) - 1)),
                        (0xFFFFFFFE, rm.nonce(rm.NOISE1, 0, (1 << 64) - 1))):
        want = _openssl_keystream(counter, nw, 128)
        got = rm.chacha20_blocks(KW, [counter, counter + 1], nw)
        assert b"".join(int(v).to_bytes(4, "little") for v in got.ravel()) == want
    assert rm.nonce(rm.MASK, 3, (1 << 32) - 1) == [0x301, 0xFFFFFFFF, 0]
    assert rm.nonce(rm.NOISE, 0, 1 << 32) == [2, 0, 1]


# ---------------------------------------------------------------------------------------------------------------
# 2. the header, on the host, against the model
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("rlwe_draw") / "rlwe_draw_main"
    cmd = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "rlwe_draw_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_the_header_includes_the_standard_library_alone():
    text = (CSRC / "rlwe_draw.hpp").read_text()
    assert "#include <hip" not in text and '#include "' not in text


def test_header_blocks_equal_the_model(lines):
    rfc = [f for f in lines if f[0] == "rfc"]
    assert len(rfc) == 1
    assert [int(v, 16) for v in rfc[0][1:5]] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3]
    assert [int(v, 16) for v in rfc[0][1:]] == [int(v) for v in rm.chacha20_blocks(KW, [1], [0x09000000, 0x4A000000, 0])[0]]
    blk = [f for f in lines if f[0] == "block"]
    assert len(blk) == 1
    stream, limb, pid, counter = (int(v) for v in blk[0][1:5])
    assert (stream, limb, pid, counter) == (1, 3, (1 << 32) - 1, 5)
    assert [int(v, 16) for v in blk[0][5:]] == [int(v) for v in rm.chacha20_blocks(KW, [5], rm.nonce(1, 3, pid))[0]]


def test_header_draws_equal_the_model(lines):
    """Mask words, ternary and noise draws for ids 0, 2^32 - 1, 2^32, 2^64 - 1 (and one more), limbs 0, 3, 13, 255, and
    i on both sides of the block edges of both kinds."""
    masks = [f for f in lines if f[0] == "mask"]
    smalls = [f for f in lines if f[0] == "small"]
    ids = {int(f[2]) for f in masks}
    assert {0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1} <= ids
    iset = {int(f[3]) for f in masks}
    assert {3, 4, 7, 8, 15, 16, 65535} <= iset == {int(f[3]) for f in smalls}
    assert len(masks) == len(ids) * 4 * len(iset) and len(smalls) == 5 * len(ids) * len(iset)
    cache = {}
    for _, limb, pid, i, lo, hi in masks:
        key = (int(limb), int(pid))
        if key not in cache:
            cache[key] = rm.mask_words(KW, key[0], key[1], 65536)
        assert int(lo) | (int(hi) << 64) == cache[key][int(i)], (limb, pid, i)
    assert len({int(f[4]) for f in masks}) == len(masks), "every (limb, id, i) draws its own word"
    cache = {}
    for _, stream, pid, i, w, t, e, v in smalls:
        key = (int(stream), int(pid))
        if key not in cache:
            cache[key] = rm.small_words(KW, key[0], key[1], 65536)
        assert int(w) == int(cache[key][int(i)]), (stream, pid, i)
        assert int(t) == int(rm.ternary([int(w)])[0]) and int(e) == int(rm.noise([int(w)])[0])
        assert int(v) == (int(t) if int(stream) in rm.TERNARY_STREAMS else int(e))
    assert len({int(f[4]) for f in smalls}) == len(smalls)


def test_header_maps_at_their_extremes(lines):
    maps = {int(f[1]): (int(f[2]), int(f[3])) for f in lines if f[0] == "map"}
    third = (1 << 64) // 3
    assert maps[0] == (-1, 0) and maps[(1 << 64) - 1] == (1, 0)
    assert maps[third] == (-1, maps[third][1]) and maps[third + 1][0] == 0       # 3 (2^64 - 1) / 3 + 3 = 2^64 + 2
    assert maps[2 * third][0] == 0 and maps[2 * third + 1][0] == 1
    assert maps[(1 << 21) - 1] == (-1, 21) and maps[((1 << 21) - 1) << 21][1] == -21 and maps[1 << 42] == (-1, 0)
    for w, (t, e) in maps.items():
        assert t == (3 * w >> 64) - 1 and e == int(rm.noise([w])[0])
    res = [(int(f[1]), int(f[2]), int(f[3])) for f in lines if f[0] == "res"]
    assert len(res) == 15
    for v, q, r in res:
        assert r == v % q


# ---------------------------------------------------------------------------------------------------------------
# 3. the distributions (the model's; the header equals it above)
# ---------------------------------------------------------------------------------------------------------------
def test_small_draws_follow_their_distributions():
    """2^15 draws under a fixed seed.  Noise = B(21, 1/2) - B(21, 1/2), a sum of 42 independent terms of +-1/2: mean 0,
    variance 42 / 4 = 10.5, fourth central moment computed below from those terms; the sample mean is within 5
    standard errors sqrt(var / n) of 0, the sample variance within 5 standard errors sqrt((mu4 - var^2) / n) of 10.5,
    |e| <= 21.  Ternary: each count is Binomial(n, 1/3), within 5 sigma of n / 3.  Two streams, and two ids of one
    stream, are uncorrelated: the sample correlation of n pairs has standard deviation 1 / sqrt(n)."""
    n = 1 << 15
    e = rm.small_values(KW, rm.NOISE, 7, n)
    var = rm.NOISE_VARIANCE
    assert var == 10.5
    assert np.abs(e).max() <= 21
    mean = float(e.mean())
    assert abs(mean) <= 5 * math.sqrt(var / n), mean
    # a sum of m = 42 independent centred terms of variance 1/4 and fourth moment 1/16: mu4 = m / 16 + 3 m (m - 1) / 16
    m = 2 * rm.NOISE_BITS
    mu4 = m / 16 + 3 * m * (m - 1) / 16
    se_var = math.sqrt((mu4 - var * var) / n)
    s2 = float(((e - mean) ** 2).mean())
    assert abs(s2 - var) <= 5 * se_var, (s2, se_var)
    t = rm.small_values(KW, rm.SECRET, 7, n)
    counts = [int((t == v).sum()) for v in (-1, 0, 1)]
    assert sum(counts) == n
    sd = math.sqrt(n * (1 / 3) * (2 / 3))
    for c in counts:
        assert abs(c - n / 3) <= 5 * sd, counts
    # streams and ids are independent draws: no two agree on more than chance allows
    e2 = rm.small_values(KW, rm.NOISE0, 7, n)
    e3 = rm.small_values(KW, rm.NOISE, 8, n)
    for other in (e2, e3):
        corr = float((e * other).mean()) / var
        assert abs(corr) <= 5 / math.sqrt(n)


def test_mask_residues_are_canonical_and_spread():
    q = (1 << 61) - 1
    a = rm.mask_residues(KW, 2, 11, 1 << 12, q)
    assert (a < np.uint64(q)).all() and len(set(a.tolist())) == len(a)
    # the top bit of a uniform residue of a modulus just below 2^61 is set half the time
    top = int((a >> np.uint64(60)).sum())
    assert abs(top - len(a) / 2) <= 5 * math.sqrt(len(a) / 4)


def test_the_batched_draws_equal_the_per_id_functions():
    """small_values_ids and mask_residues_ids (one ChaCha call with a nonce per lane) against small_values and
    mask_residues id by id, on ids on both sides of the id's word boundary and at the end of its range, at a length
    that is no whole number of blocks and at one of several blocks; and a one-id call of the lane form of
    chacha20_blocks against the scalar form."""
    ids = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) + 5, (1 << 64) - 1]
    nw = rm.nonce(rm.MASK, 3, ids[2])
    lanes = [nw[0], np.full(4, nw[1], dtype=np.uint32), np.full(4, nw[2], dtype=np.uint32)]
    np.testing.assert_array_equal(rm.chacha20_blocks(KW, np.arange(4), lanes), rm.chacha20_blocks(KW, np.arange(4), nw))
    for n in (13, 64):
        for stream in rm.SMALL_STREAMS:
            got = rm.small_values_ids(KW, stream, ids, n)
            assert got.shape == (len(ids), n) and got.dtype == np.int64
            for row, pid in zip(got, ids):
                np.testing.assert_array_equal(row, rm.small_values(KW, stream, pid, n), err_msg=f"{stream} {pid}")
        for limb, q in ((0, (1 << 61) - 1), (13, 65537), (255, (1 << 45) - 229)):
            got = rm.mask_residues_ids(KW, limb, ids, n, q)
            assert got.shape == (len(ids), n) and got.dtype == np.uint64
            for row, pid in zip(got, ids):
                np.testing.assert_array_equal(row, rm.mask_residues(KW, limb, pid, n, q), err_msg=f"{limb} {pid}")
    assert len({tuple(r) for r in rm.small_values_ids(KW, rm.NOISE, ids, 64).tolist()}) == len(ids)


# ---------------------------------------------------------------------------------------------------------------
# 4. the C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(mfhe):
    names = mfhe.declared_symbols()
    assert set(SYMBOLS) <= set(names)
    out = subprocess.run(["nm", "-D", "--defined-only", str(mfhe.LIB_PATH)], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported
    for n in SYMBOLS:
        assert getattr(mfhe.lib, n).argtypes is not None
    assert (mfhe.RLWE_MASK, mfhe.RLWE_NOISE, mfhe.RLWE_SECRET, mfhe.RLWE_EPHEMERAL, mfhe.RLWE_NOISE0,
            mfhe.RLWE_NOISE1) == (rm.MASK, rm.NOISE, rm.SECRET, rm.EPHEMERAL, rm.NOISE0, rm.NOISE1)
    text = (ROOT / "include" / "mfhe.h").read_text()
    for name, val in (("MFHE_RLWE_MASK", 1), ("MFHE_RLWE_NOISE", 2), ("MFHE_RLWE_SECRET", 3), ("MFHE_RLWE_EPHEMERAL", 4),
                      ("MFHE_RLWE_NOISE0", 5), ("MFHE_RLWE_NOISE1", 6)):
        assert f"#define {name}" in text and getattr(mfhe, name[5:]) == val


def test_seed_hands_out_disjoint_id_ranges(mfhe):
    s = mfhe.Seed(KEY)
    assert list(s.words) == KW
    assert s.take(3) == 0 and s.take(1) == 3 and s.take(0) == 4 and s.take(5) == 4 and s.next_id == 9
    assert len(mfhe.Seed().key) == 32 and mfhe.Seed().key != mfhe.Seed().key
    with pytest.raises(ValueError):
        mfhe.Seed(b"short")
    with pytest.raises(ValueError):
        mfhe.Seed(KEY, (1 << 64) - 1).take(2)


def test_arguments_are_checked_without_a_device(mfhe):
    """A null context is MFHE_EINVAL from every call, before anything touches a device."""
    L = mfhe.lib
    assert L.mfhe_rlwe_reserve(None, 1, 1, 0, 0) == mfhe.EINVAL
    assert L.mfhe_rlwe_sample_uniform(None, None, 0, None, 0, 1, 1, 0, 0, None) == mfhe.EINVAL
    assert L.mfhe_rlwe_sample_small(None, None, 2, 0, None, 0, 1, 1, 0, 0, 0, None) == mfhe.EINVAL
    assert L.mfhe_rlwe_lift_small(None, None, 0, None, 0, 1, 1, 0, 0, 0, None) == mfhe.EINVAL
    assert L.mfhe_rlwe_encrypt_sk(None, None, 0, None, None, 0, None, None, 0, 1, 1, 0, 0, None) == mfhe.EINVAL
    assert L.mfhe_rlwe_ksk_gen(None, None, 0, 0, 1, None, None, None, 1, 1, 1, 1, None) == mfhe.EINVAL
    assert L.mfhe_rlwe_encrypt_pk(None, None, 0, None, None, None, 0, None, None, 0, 1, 1, None) == mfhe.EINVAL
    assert L.mfhe_rlwe_decrypt(None, None, None, 0, None, None, 0, 1, 1, None) == mfhe.EINVAL
