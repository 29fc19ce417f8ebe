#!/usr/bin/env python3
"""Plaintext x ciphertext product timing lines (csrc/ptmul.hip) at N = 2^16 on the 11 Q limbs of tools/ctmat_bench.py's
basis, all from one run: Y = W X for a 4 x k matrix of plaintexts and a k x 4 matrix of ciphertexts with 4 polynomials
each at k = 1, 4, 8 and 16 terms, once with per-polynomial plaintexts and once with plaintexts shared by the batch (W's
poly stride 0).  Lines: ksk_inner_product on 4 digits, 14 rows and 64 polynomials (the yardstick, measured here again),
ptmat_tensor beside the m n calls of ptmul_sum on the same data, ptmat with and without PTMUL_RESCALE, and the rescale
alone (ntt_moddown of both components as one batch).  Prints one JSON line and writes it to profiles/ptmat_bench.json.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  GB/s are a call's rate on its bytes model, not a
kernel's share of peak: ptmat_tensor on tensor_model_bytes below, the m n ptmul_sum calls on sum_model_bytes each, the
inner product on 8 N (level + K) (npoly (ndigits + 2) + 2 ndigits).  The models count a shared
plaintext once per polynomial that reads it, as a stream: what the caches save of it is not in them.

usage: tools/ptmat_bench.py [--log-n 16] [--m 4] [--n 4] [--npoly 4] [--tile 2x2] [--tensor-only]
                            [--min-window 0.3] [--out profiles/ptmat_bench.json]
--tile is the tile the library was built with (mfhe.PTMAT_TILE by default; a tuning build of another tile passes its
own, with MFHE_LIB naming its library); --tensor-only stops after the tensor and sum lines."""
import argparse
import datetime
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TERMS = (1, 4, 8, 16)


def tensor_model_bytes(n_coeff, level, npoly, m, n, k, tm, tn, bias=False, add=False):
    """Bytes ptmat_tensor moves with a tm x tn tile (tm on the plaintext side): per term every entry of W is read once
    per tile column and every entry of X, two components, once per tile row; the bias is read once per output, with
    PTMUL_ADD both components of every output are read, and both are written once."""
    tiles_m, tiles_n = -(-m // tm), -(-n // tn)
    words = k * (m * tiles_n + 2 * n * tiles_m) + (m * n if bias else 0) + (2 * m * n if add else 0) + 2 * m * n
    return 8 * n_coeff * level * npoly * words


def sum_model_bytes(n_coeff, level, npoly, nterms, addend=False):
    """Bytes one ptmul_sum moves: per term a plaintext and both components of a source, the addend, two outputs."""
    return 8 * n_coeff * level * npoly * (3 * nterms + (1 if addend else 0) + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--npoly", type=int, default=4)
    ap.add_argument("--tile", default=None)
    ap.add_argument("--tensor-only", action="store_true")
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ptmat_bench.json"))
    a = ap.parse_args()
    for p in (ROOT / "tools", ROOT, ROOT / "matrix-fhe-gpu_amd"):
        sys.path.insert(0, str(p))
    import torch
    import mfhe
    from bench import gen_moduli
    from bconv_bench import residues, window
    if not torch.cuda.is_available():
        sys.exit("ptmat_bench needs a GPU")
    tm, tn = (int(v) for v in a.tile.split("x")) if a.tile else mfhe.PTMAT_TILE
    N, m, n, P = 1 << a.log_n, a.m, a.n, a.npoly
    level, K, alpha = 11, 3, 3
    rows = level + K
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    batch = m * n * P
    out = {"tool": "ptmat_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "m": m, "n": n,
           "npoly": P, "batch": batch, "tile": f"{tm}x{tn}", "basis": "11 Q limbs (yardstick: 11 + 3)",
           "device": torch.cuda.get_device_name(0)}

    def line(name, model_bytes, fn):
        ms, lo, hi, reps = window(fn, a.min_window)
        out[name] = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps}
        if model_bytes:
            out[name]["model_GB"] = round(model_bytes / 1e9, 4)
            out[name]["GB_s"] = round(model_bytes / 1e9 / (ms * 1e-3), 1)
        return out[name]

    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    ctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    out["ntt_arith"] = "u64" if ctx.info().arith == mfhe.ARITH_U64 else "f64"
    ctx.ptmat_reserve(m, n, P, level, mfhe.PTMUL_RESCALE)

    lw = level * N
    ew = P * lw                                                     # one entry of X or of the outputs, one component
    kmax = max(TERMS)
    # W [m][kmax][P][level][N] and X [kmax][n][P][level][N], dense; a product of k terms reads the first k columns of
    # W and the first k rows of X at these strides.  Shared plaintexts: the first polynomial of every entry of W.
    x_str = (n * ew, ew, lw)
    w_strs = {"": (kmax * ew, ew, lw), "_shared": (kmax * ew, ew, 0)}
    w = residues(moduli[:level], m * kmax * P, N)
    x0, x1 = (residues(moduli[:level], kmax * n * P, N) for _ in range(2))
    rlk = residues(moduli, 2 * beta, N)                             # [beta][2][14][N]
    raised = torch.cat([residues(moduli, batch, N) for _ in range(beta)])
    acc = torch.empty(batch * 2 * rows * N, dtype=torch.int64, device="cuda")
    o01 = torch.empty(2 * batch * lw, dtype=torch.int64, device="cuda")   # out0 then out1: one batch for the rescale
    o0, o1 = o01[:batch * lw], o01[batch * lw:]

    def separate_sums(k, w_str):
        terms = list(range(k))
        for i in range(m):
            for j in range(n):
                e = (i * n + j) * ew
                ctx.ptmul_sum(x0[j * x_str[1]:], x1[j * x_str[1]:], w[i * w_str[0]:], o0[e:], o1[e:], terms, terms, P,
                              level, k, k, src_stride=x_str[0], pt_stride=w_str[1], pt_poly_stride=w_str[2])

    ip_bytes = 8 * N * rows * (batch * (beta + 2) + 2 * beta)
    ip_rate = line("ksk_inner_product", ip_bytes,
                   lambda: ctx.ksk_inner_product(raised, rlk, acc, batch, beta, level, level, level, K))["GB_s"]
    for tag, w_str in w_strs.items():
        for k in TERMS:
            mat = line(f"ptmat_tensor_{k}_terms{tag}", tensor_model_bytes(N, level, P, m, n, k, tm, tn),
                       lambda k=k, w_str=w_str: ctx.ptmat_tensor(w, x0, x1, o0, o1, m, n, k, P, level, w_strides=w_str,
                                                                 x_strides=x_str))
            sep = line(f"ptmul_sum_{k}_terms{tag}_x{m * n}", m * n * sum_model_bytes(N, level, P, k),
                       lambda k=k, w_str=w_str: separate_sums(k, w_str))
            out[f"ptmat_tensor_{k}{tag}_rate_over_inner_product"] = round(mat["GB_s"] / ip_rate, 3)
            out[f"ptmul_sum_{k}{tag}_rate_over_inner_product"] = round(sep["GB_s"] / ip_rate, 3)
            out[f"ptmat_tensor_{k}{tag}_time_over_separate"] = round(mat["ms"] / sep["ms"], 3)
            out[f"ptmat_tensor_{k}{tag}_time_over_separate_model"] = round(
                tensor_model_bytes(N, level, P, m, n, k, tm, tn) / (m * n * sum_model_bytes(N, level, P, k)), 3)
            # bar (a): below the separate calls by more than the windows' own spread
            out[f"ptmat_tensor_{k}{tag}_below_separate_beyond_spread"] = bool(mat["ms_max"] < sep["ms_min"])
    if not a.tensor_only:
        w_str = w_strs[""]
        for k in TERMS:
            for flags, tag in ((0, ""), (mfhe.PTMUL_RESCALE, "_rescale")):
                line(f"ptmat_{k}_terms{tag}", 0,
                     lambda k=k, flags=flags: ctx.ptmat(w, x0, x1, o0, o1, m, n, k, P, level, flags=flags,
                                                        w_strides=w_str, x_strides=x_str))
        line("rescale_alone", 0, lambda: ctx.ntt_moddown(o01, o01, 2 * batch, level - 1, level - 1, 1))
    text = json.dumps(out)
    print(text, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
