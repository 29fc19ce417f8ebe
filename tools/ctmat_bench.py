#!/usr/bin/env python3
"""Ciphertext matrix product timing lines (csrc/ctmat.hip) at N = 2^16, alpha 3 on the 11 + 3 basis of
tools/ctmul_bench.py, all from one run: a 4 x 4 product of ciphertexts with 4 polynomials each (the key switch then
runs on the 64 polynomials DESIGN.md 3.12 measured) at k = 1, 4, 8 and 16 terms.  Lines: ksk_inner_product on 4 digits
and 14 rows (the yardstick, measured here again), ctmat_tensor beside m n calls of ctmul_tensor on the same data, ctmat
with and without CTMUL_RESCALE beside m n calls of ctmul.  Prints one JSON line and writes it to
profiles/ctmat_bench.json.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  GB/s are a call's rate on its bytes model, not a
kernel's share of peak: ctmat_tensor on tensor_model_bytes below, the m n ctmul_tensor calls on m n times
8 N level npoly (4 k + 3), the inner product on 8 N (level + K) (npoly (ndigits + 2) + 2 ndigits).

usage: tools/ctmat_bench.py [--log-n 16] [--m 4] [--n 4] [--npoly 4] [--alpha 3] [--tile 2x2] [--tensor-only]
                            [--min-window 0.3] [--out profiles/ctmat_bench.json]
--tile is the tile the library was built with (mfhe.CTMAT_TILE by default; a tuning build of another tile passes its
own); --tensor-only stops after the tensor lines."""
import argparse
import datetime
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TERMS = (1, 4, 8, 16)


def tensor_model_bytes(n_coeff, level, npoly, m, n, k, tm, tn):
    """Bytes ctmat_tensor moves with a tm x tn tile: per term every entry of A is read once per tile column and every
    entry of B once per tile row (two components each), and the three outputs of every entry are written once."""
    tiles_m, tiles_n = -(-m // tm), -(-n // tn)
    return 8 * n_coeff * level * npoly * (2 * k * (m * tiles_n + n * tiles_m) + 3 * m * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--npoly", type=int, default=4)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--tile", default=None)
    ap.add_argument("--tensor-only", action="store_true")
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ctmat_bench.json"))
    a = ap.parse_args()
    for p in (ROOT / "tools", ROOT, ROOT / "matrix-fhe-gpu_amd"):
        sys.path.insert(0, str(p))
    import torch
    import mfhe
    from bench import gen_moduli
    from bconv_bench import residues, window
    if not torch.cuda.is_available():
        sys.exit("ctmat_bench needs a GPU")
    tm, tn = (int(v) for v in a.tile.split("x")) if a.tile else mfhe.CTMAT_TILE
    N, m, n, P, alpha = 1 << a.log_n, a.m, a.n, a.npoly, a.alpha
    level, K = 11, 3
    rows = level + K
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    batch = m * n * P
    out = {"tool": "ctmat_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "m": m, "n": n,
           "npoly": P, "batch": batch, "tile": f"{tm}x{tn}", "basis": "11 + 3", "alpha": alpha, "ndigits": beta,
           "device": torch.cuda.get_device_name(0)}

    def line(name, model_bytes, fn):
        ms, lo, hi, reps = window(fn, a.min_window)
        out[name] = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps}
        if model_bytes:
            out[name]["model_GB"] = round(model_bytes / 1e9, 4)
            out[name]["GB_s"] = round(model_bytes / 1e9 / (ms * 1e-3), 1)
        return ms

    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    ctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    out["ntt_arith"] = "u64" if ctx.info().arith == mfhe.ARITH_U64 else "f64"
    ctx.ctmat_reserve(m, n, P, level, level, alpha, level, K, mfhe.CTMUL_RESCALE)

    lw = level * N
    ew = P * lw                                                     # one entry, one component
    kmax = max(TERMS)
    # A [m][kmax][P][level][N] and B [kmax][n][P][level][N], dense; a product of k terms reads the first k columns of
    # A and the first k rows of B at these strides
    a_str, b_str = (kmax * ew, ew, lw), (n * ew, ew, lw)
    a0, a1 = (residues(moduli[:level], m * kmax * P, N) for _ in range(2))
    b0, b1 = (residues(moduli[:level], kmax * n * P, N) for _ in range(2))
    rlk = residues(moduli, 2 * beta, N)                             # [beta][2][14][N]
    raised = torch.cat([residues(moduli, batch, N) for _ in range(beta)])
    acc = torch.empty(batch * 2 * rows * N, dtype=torch.int64, device="cuda")
    o01 = torch.empty(2 * batch * lw, dtype=torch.int64, device="cuda")   # out0 then out1: one batch for the rescale
    o0, o1 = o01[:batch * lw], o01[batch * lw:]
    d2 = torch.empty(batch * lw, dtype=torch.int64, device="cuda")

    def separate_tensors(k):
        for i in range(m):
            for j in range(n):
                e = (i * n + j) * ew
                ctx.ctmul_tensor(a0[i * a_str[0]:], a1[i * a_str[0]:], b0[j * b_str[1]:], b1[j * b_str[1]:], o0[e:],
                                 o1[e:], d2[e:], P, level, k, a_term_stride=a_str[1], b_term_stride=b_str[0])

    def separate_products(k, flags):
        for i in range(m):
            for j in range(n):
                e = (i * n + j) * ew
                ctx.ctmul(a0[i * a_str[0]:], a1[i * a_str[0]:], b0[j * b_str[1]:], b1[j * b_str[1]:], rlk,
                          o0[e:e + ew], o1[e:e + ew], P, level, level, alpha, level, K, k, flags,
                          a_term_stride=a_str[1], b_term_stride=b_str[0])

    ip_bytes = 8 * N * rows * (batch * (beta + 2) + 2 * beta)
    line("ksk_inner_product", ip_bytes,
         lambda: ctx.ksk_inner_product(raised, rlk, acc, batch, beta, level, level, level, K))
    ip_rate = out["ksk_inner_product"]["GB_s"]
    for k in TERMS:
        t_mat = line(f"ctmat_tensor_{k}_terms", tensor_model_bytes(N, level, P, m, n, k, tm, tn),
                     lambda k=k: ctx.ctmat_tensor(a0, a1, b0, b1, o0, o1, d2, m, n, k, P, level, a_strides=a_str,
                                                  b_strides=b_str))
        t_sep = line(f"ctmul_tensor_{k}_terms_x{m * n}", m * n * 8 * N * level * P * (4 * k + 3),
                     lambda k=k: separate_tensors(k))
        out[f"ctmat_tensor_{k}_rate_over_inner_product"] = round(out[f"ctmat_tensor_{k}_terms"]["GB_s"] / ip_rate, 3)
        out[f"ctmat_tensor_{k}_time_over_separate"] = round(t_mat / t_sep, 3)
    if not a.tensor_only:
        for k in TERMS:
            for flags, tag in ((0, ""), (mfhe.CTMUL_RESCALE, "_rescale")):
                t_mat = line(f"ctmat_{k}_terms{tag}", 0,
                             lambda k=k, flags=flags: ctx.ctmat(a0, a1, b0, b1, rlk, o0, o1, m, n, k, P, level, level,
                                                                alpha, level, K, flags, a_strides=a_str,
                                                                b_strides=b_str))
                t_sep = line(f"ctmul_{k}_terms{tag}_x{m * n}", 0, lambda k=k, flags=flags: separate_products(k, flags))
                out[f"ctmat_{k}_terms{tag}_time_over_separate"] = round(t_mat / t_sep, 3)
    text = json.dumps(out)
    print(text, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
