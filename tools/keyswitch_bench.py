#!/usr/bin/env python3
"""Key-switching timing line (csrc/keyswitch.hip): the digit-by-key inner product alone, the whole mfhe_keyswitch,
and in the same run rns_modup (the streaming yardstick of DESIGN.md §3.8) and the driver's pieces called one by one
(beta x ntt_modup, the inner product, 2 x ntt_moddown) at N = 2^16, batch 64, alpha 3 on an 11 + 3 basis.  Prints one
JSON line.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each,
the median reported with the spread (tools/bconv_bench.py's method).  The inner product's GB/s are on its bytes model
8 N (level + K) (npoly (ndigits + 2) + 2 ndigits) (raised digits read, both accumulators written, the
key counted once), rns_modup's on 8 (3 + 14) npoly N -- a call's rate, not a kernel's share of peak.

The reference's own primes have no 2^17-th root, so the basis is primes of the same bit sizes (45, 10 x 35 | 55, 40,
40) with q = 1 mod 2^17, as tools/bconv_bench.py uses for its NTT-domain lines.

usage: tools/keyswitch_bench.py [--log-n 16] [--batch 64] [--alpha 3] [--min-window 0.3]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-fhe-gpu_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
import mfhe  # noqa: E402
from bench import gen_moduli  # noqa: E402
from bconv_bench import residues, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("keyswitch_bench needs a GPU")
    n, b, alpha = 1 << a.log_n, a.batch, a.alpha
    level, k = 11, 3
    rows = level + k
    digits = [(s, min(alpha, level - s)) for s in range(0, level, alpha)]
    beta = len(digits)
    out = {"tool": "keyswitch_bench", "log_n": a.log_n, "batch": b, "basis": "11 + 3", "alpha": alpha, "ndigits": beta,
           "device": torch.cuda.get_device_name(0)}

    def line(name, model_bytes, fn):
        ms, lo, hi, reps = window(fn, a.min_window)
        out[name] = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps}
        if model_bytes:
            out[name]["model_GB"] = round(model_bytes / 1e9, 4)
            out[name]["GB_s"] = round(model_bytes / 1e9 / (ms * 1e-3), 1)
        return ms

    m2 = 2 << a.log_n
    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    ctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    out["ntt_arith"] = "u64" if ctx.info().arith == mfhe.ARITH_U64 else "f64"
    ctx.rns_modup_reserve(level, alpha, min(alpha, level - alpha), level, k)
    ctx.keyswitch_reserve(b, level, level, alpha, level, k)   # also covers the pieces' own scratch

    e11 = residues(moduli[:level], b, n)
    ksk = residues(moduli, 2 * beta, n)                       # [beta][2][14][N]
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    acc = torch.empty(b * 2 * rows * n, dtype=torch.int64, device="cuda")
    up = torch.empty(b * rows * n, dtype=torch.int64, device="cuda")
    o0 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")

    ds, dc = digits[1] if beta > 1 else digits[0]
    line("rns_modup_3_to_14", 8 * (dc + rows) * b * n, lambda: ctx.rns_modup(e11, up, b, n, level, ds, dc, level, k))
    ip_bytes = 8 * n * rows * (b * (beta + 2) + 2 * beta)
    t_ip = line("ksk_inner_product", ip_bytes,
                lambda: ctx.ksk_inner_product(raised, ksk, acc, b, beta, level, level, level, k))
    t_ks = line("keyswitch", 0, lambda: ctx.keyswitch(e11, ksk, o0, o1, b, level, level, alpha, level, k))
    t_add = line("keyswitch_add", 0,
                 lambda: ctx.keyswitch(e11, ksk, o0, o1, b, level, level, alpha, level, k, mfhe.KS_ADD))
    # the pieces, one by one: each digit's ntt_modup, then ntt_moddown of one component (run twice by the driver's
    # composition); acc viewed as [2 b] polynomials of 14 rows
    t_up = []
    for i, (s, c) in enumerate(digits):
        t_up.append(line(f"ntt_modup_digit{i}", 0,
                         lambda s=s, c=c: ctx.ntt_modup(e11, up, b, level, s, c, level, k)))
    t_down = line("ntt_moddown_14_to_11", 0,
                  lambda: ctx.ntt_moddown(acc, o0, b, level, level, k, in_stride=2 * rows * n))
    pieces = sum(t_up) + t_ip + 2 * t_down
    out["pieces_sum_ms"] = round(pieces, 4)
    out["keyswitch_over_pieces"] = round(t_ks / pieces, 3)
    out["keyswitch_add_over_keyswitch"] = round(t_add / t_ks, 3)
    out["inner_product_over_rns_modup_GB_s"] = round(out["ksk_inner_product"]["GB_s"] / out["rns_modup_3_to_14"]["GB_s"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
