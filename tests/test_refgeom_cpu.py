"""The arguments that tests/test_refgeom_gpu.py rests on, checked on the oracle and the long-double model alone (no
GPU), at the reference geometry: n = 64, 512 lanes, the 11 reference moduli, delta 2^35.

* b of encrypt_pair may be required bit for bit: no noise draw of this shape is near a llround tie.
* The planted ciphertexts decrypt to exactly the planted integers' W-CRT image, and one coefficient off by one unit
  would show: cdft_model.bound(E_ref, S) < 2^-36, half of the 2^-35 such a unit moves every output by.
* The planted message encodes back to its integers: the oracle's float64 stages land within 0.025 of k + f.
The products are shared with the GPU module through tests/refgeom.py, which computes each once per process."""
import numpy as np
import pytest

import cdft_model as cm
import refgeom as rg
from oracle import P


@pytest.fixture(scope="module", autouse=True)
def _release():
    """Without a GPU nothing after this module reads the cached arrays (1.5 GB); with one, test_refgeom_gpu.py does,
    and drops them itself."""
    yield
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    if not gpu:
        rg.drop()


def test_splitmix64_matches_oracle(orc):
    x = np.array([0, 1, 590968, 2 ** 63, 2 ** 64 - 1, 0xD6E8FEB86659FD93], dtype=np.uint64)
    x = np.concatenate([x, np.random.default_rng(1).integers(0, 2 ** 64, 250, dtype=np.uint64)])
    want = np.array([orc.L.orc_splitmix64(int(v)) for v in x], dtype=np.uint64)
    np.testing.assert_array_equal(rg.splitmix64(x), want)


def test_noise_draws_match_oracle_and_sit_far_from_ties(orc):
    """The vectorised Box-Muller draws round to the oracle's noise (orc_gaussian_noise at n = 8: every word of every
    limb), and over the 512 * 64^2 = 2,097,152 draws of the reference geometry the sample nearest a rounding tie is
    more than 1e-9 from it.  Device libm differs from glibc by a few ulp of z (about 1e-15), so no draw can round
    differently on the GPU: test_refgeom_gpu.py requires b bit for bit."""
    n, L_ = 8, 2
    e = np.zeros(rg.PHI * L_ * n * n, np.uint64)
    orc.L.orc_gaussian_noise(P(e), rg.PHI, L_, n, P(np.array(rg.RNS[:L_], np.uint64)))
    nz = np.rint(rg.noise_samples(n)).astype(np.int64).reshape(rg.PHI, 1, n * n)   # no tie within 2.8e-5 at n = 8
    q = np.array(rg.RNS[:L_], np.int64)[None, :, None]
    np.testing.assert_array_equal(e.reshape(rg.PHI, L_, n * n).astype(np.int64), np.mod(nz, q))
    for n_ in (8, 32, 64):
        d, i, z = rg.noise_tie_distance(n_)
        print(f"REFGEOM | noise tie distance n={n_:<2d}: {d:.3e} at id {i} (z = {z!r}) over {rg.PHI * n_ * n_} draws")
    assert d > 1e-9
    assert np.max(np.abs(rg.noise_samples(64))) < 27.5   # the one signed digit of the small-operand GEMM


def test_planted_ciphertext_decrypts_to_planted_eval(orc):
    """h.decrypt_to_eval([b | a], sk) returns ev = W-CRT(k mod q) exactly, for both parts, and the residues behind ev
    lift back to k on every limb."""
    h, sk = rg.he(orc), rg.sk_ref(orc)
    p = rg.planted_ct(orc, 20)
    for part in ("re", "im"):
        np.testing.assert_array_equal(h.decrypt_to_eval(p["ct_" + part], sk), p["ev_" + part], err_msg=part)
        k = p["k_" + part]
        assert np.max(np.abs(k)) < 2 ** 20
        np.testing.assert_array_equal(rg.lift(rg.residues(k, rg.RNS), rg.N, rg.RNS), k)
    a_re, a_im = p["ct_re"][rg.WORDS:], p["ct_im"][rg.WORDS:]
    np.testing.assert_array_equal(a_re, a_im)
    assert np.count_nonzero(a_re) > 0.99 * rg.WORDS


def test_planted_decode_bound_resolves_one_unit(orc):
    """cm.bound(E_ref, S) < 2^-36 for |k| < 2^20: every W and XY weight has modulus 1, so one coefficient off by one
    unit moves every output by exactly 2^-35, twice what the bound admits."""
    p = rg.planted_ct(orc, 20)
    bnd = cm.bound(p["e_ref"], p["scale"])
    print(f"REFGEOM | planted decode |k| < 2^20: lanes {p['lanes'].tolist()} E_ref {p['e_ref']:.3e} S {p['scale']:.3f} "
          f"floor {8 * cm.U53 * p['scale']:.3e} bound {bnd:.3e} (< 2^-36 = {2.0 ** -36:.3e})")
    assert bnd < 2.0 ** -36
    # the model itself resolves the unit: its message moves by 2^-35 in modulus when one coefficient moves by one
    k2 = p["k_re"].copy()
    k2[17, 1234] += 1
    moved = np.abs(cm.decode_truth(k2, p["k_im"], rg.N, rg.DELTA, p["lanes"][:2]) - p["truth"][:2]).astype(np.float64)
    np.testing.assert_allclose(moved, 2.0 ** -35, rtol=1e-6)


def test_encode_precondition_at_reference_geometry(orc):
    """The planted message of the encode test: |k| < 2^30 on 1058 fixed columns (rows y = 0 and y = 63 whole, every
    aligned run of 64 hit), zero elsewhere; the oracle's float64 stages land within 0.025 of k + f everywhere."""
    cols = rg.planted_positions()
    assert cols.size >= 1024 and np.all(np.diff(cols) > 0)
    assert set(range(64)) <= set(cols.tolist()) and set(range(4032, 4096)) <= set(cols.tolist())
    assert np.unique(cols // 64).size == 64
    m = rg.planted_message(orc)
    print(f"REFGEOM | encode precondition n=64: |k| < 2^{m['k_bits']} on {cols.size} columns, oracle max "
          f"|delta wc - (k + f)| = {m['pre_err']:.3e} (<= 0.025)")
    assert m["pre_err"] <= 0.025
    rest = np.setdiff1d(np.arange(rg.N2), cols)
    assert not m["k_re"][:, rest].any() and not m["k_im"][:, rest].any()
