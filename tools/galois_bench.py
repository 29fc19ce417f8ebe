#!/usr/bin/env python3
"""Galois timing lines (csrc/galois.hip, csrc/keyswitch.hip) at N = 2^16, batch 64, alpha 3 on the 11 + 3 basis of
tools/keyswitch_bench.py, all from one run: the automorphism beside a device-to-device copy of the same buffer, the
gathered inner product for three Galois elements beside the plain one on the same buffers, and one rotation
(galois_apply) and eight hoisted rotations (keyswitch_raise + 8 x galois_apply_raised) beside eight key switches, the
lower bound of eight naive rotations.  Prints one JSON line.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  The automorphism's and the copy's GB/s are on
16 N rows npoly bytes (read + write); the inner products' on 8 N (level + K) (npoly (ndigits + 2) + 2 ndigits)
 -- a call's rate, not a kernel's share of peak.

usage: tools/galois_bench.py [--log-n 16] [--batch 64] [--alpha 3] [--rotations 8] [--min-window 0.3]"""
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
    ap.add_argument("--rotations", type=int, default=8)
    ap.add_argument("--min-window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("galois_bench needs a GPU")
    n, b, alpha, nrot = 1 << a.log_n, a.batch, a.alpha, a.rotations
    level, k = 11, 3
    rows = level + k
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    out = {"tool": "galois_bench", "log_n": a.log_n, "batch": b, "basis": "11 + 3", "alpha": alpha, "ndigits": beta,
           "rotations": nrot, "device": torch.cuda.get_device_name(0)}

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
    ctx.keyswitch_reserve(b, level, level, alpha, level, k)
    ctx.galois_reserve(b, level, level, alpha, level, k)

    c0 = residues(moduli[:level], b, n)
    c1 = residues(moduli[:level], b, n)
    gk = residues(moduli, 2 * beta, n)                        # [beta][2][14][N]
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    acc = torch.empty(b * 2 * rows * n, dtype=torch.int64, device="cuda")
    o0 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")
    elts = {"g5": 5, "g5pow1000": pow(5, 1000, m2), "conj": m2 - 1}

    # the automorphism of an 11-row batch beside a device-to-device copy of the same buffer
    au_bytes = 16 * n * level * b
    t_copy = line("d2d_copy_11_rows", au_bytes, lambda: o0.copy_(c0))
    for name, g in elts.items():
        line(f"ntt_automorphism_{name}", au_bytes, lambda g=g: ctx.automorphism(c0, o0, b, level, g))
    out["automorphism_over_copy"] = round(out["ntt_automorphism_g5"]["ms"] / t_copy, 3)

    # the plain inner product (the parent's kernel) and the gathered one, on the same buffers
    ip_bytes = 8 * n * rows * (b * (beta + 2) + 2 * beta)
    t_ip = line("ksk_inner_product", ip_bytes,
                lambda: ctx.ksk_inner_product(raised, gk, acc, b, beta, level, level, level, k))
    for name, g in elts.items():
        t = line(f"ksk_inner_product_galois_{name}", ip_bytes,
                 lambda g=g: ctx.ksk_inner_product_galois(raised, gk, acc, b, beta, level, level, level, k, g))
        out[f"galois_{name}_over_plain"] = round(t / t_ip, 3)

    # one rotation; nrot hoisted rotations; nrot key switches (the lower bound of nrot naive rotations)
    gs = [pow(5, i + 1, m2) for i in range(nrot)]
    t_one = line("galois_apply", 0, lambda: ctx.galois_apply(c0, c1, gk, o0, o1, b, level, level, alpha, level, k, 5))
    t_raise = line("keyswitch_raise", 0, lambda: ctx.keyswitch_raise(c1, raised, b, level, alpha, level, k))
    t_rot = line("galois_apply_raised", 0,
                 lambda: ctx.galois_apply_raised(c0, raised, gk, o0, o1, b, level, level, alpha, level, k, 5))

    def hoisted():
        ctx.keyswitch_raise(c1, raised, b, level, alpha, level, k)
        for g in gs:
            ctx.galois_apply_raised(c0, raised, gk, o0, o1, b, level, level, alpha, level, k, g)

    def switches():
        for _ in gs:
            ctx.keyswitch(c1, gk, o0, o1, b, level, level, alpha, level, k)

    t_h = line(f"hoisted_{nrot}_rotations", 0, hoisted)
    t_ks = line(f"keyswitch_x{nrot}", 0, switches)
    out["hoisted_over_keyswitches"] = round(t_h / t_ks, 3)
    out["galois_apply_over_keyswitch"] = round(t_one / (t_ks / nrot), 3)
    out["raise_plus_rotations_ms"] = round(t_raise + nrot * t_rot, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
