#!/usr/bin/env python3
"""Ciphertext-product timing lines (csrc/ctmul.hip) at N = 2^16, batch 64, alpha 3 on the 11 + 3 basis of
tools/keyswitch_bench.py, all from one run: ctmul_tensor at 1, 2, 4, 8 and 16 terms in the general and the square form
beside ksk_inner_product on 4 digits and 14 rows (the yardstick: the same kind of kernel, measured here again), ctmul
with and without CTMUL_RESCALE at 1 and 8 terms, its pieces (tensor, keyswitch_raise, inner product, ntt_moddown of
both components by the special limbs, the rescale of both outputs), and lazy relinearisation: ctmul at 8 terms against
8 x ctmul at 1 term plus 7 ciphertext additions (each one pass that reads two ciphertexts and writes one, timed as
torch.add on the same buffers).  Prints one JSON line and writes it to profiles/ctmul_bench.json.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  GB/s are a call's rate on its bytes model, not a
kernel's share of peak: ctmul_tensor 8 N level npoly (4 nterms + 3), its square form 8 N level npoly (2 nterms + 3),
the inner product 8 N (level + K) (npoly (ndigits + 2) + 2 ndigits).

usage: tools/ctmul_bench.py [--log-n 16] [--batch 64] [--alpha 3] [--min-window 0.3] [--out profiles/ctmul_bench.json]"""
import argparse
import datetime
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

TERMS = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ctmul_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctmul_bench needs a GPU")
    n, b, alpha = 1 << a.log_n, a.batch, a.alpha
    level, k = 11, 3
    rows = level + k
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    out = {"tool": "ctmul_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "batch": b,
           "basis": "11 + 3", "alpha": alpha, "ndigits": beta, "device": torch.cuda.get_device_name(0)}

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
    ctx.ctmul_reserve(b, level, level, alpha, level, k, mfhe.CTMUL_RESCALE)

    lw = level * n
    tmax = max(TERMS)
    ops = [residues(moduli[:level], tmax * b, n) for _ in range(4)]    # a0, a1, b0, b1: [16][b][11][N]
    rlk = residues(moduli, 2 * beta, n)                                 # [beta][2][14][N]
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    acc = torch.empty(b * 2 * rows * n, dtype=torch.int64, device="cuda")
    o01 = torch.empty(2 * b * lw, dtype=torch.int64, device="cuda")     # out0 then out1: one batch for the rescale
    o0, o1 = o01[:b * lw], o01[b * lw:]
    d2 = torch.empty(b * lw, dtype=torch.int64, device="cuda")

    # the yardstick, then the tensor sum in both forms
    ip_bytes = 8 * n * rows * (b * (beta + 2) + 2 * beta)
    t_ip = line("ksk_inner_product", ip_bytes,
                lambda: ctx.ksk_inner_product(raised, rlk, acc, b, beta, level, level, level, k))
    ip_rate = out["ksk_inner_product"]["GB_s"]
    t_tensor = {}
    for nt in TERMS:
        t_tensor[nt] = line(f"ctmul_tensor_{nt}_terms", 8 * n * level * b * (4 * nt + 3),
                            lambda nt=nt: ctx.ctmul_tensor(ops[0], ops[1], ops[2], ops[3], o0, o1, d2, b, level, nt))
        out[f"ctmul_tensor_{nt}_rate_over_inner_product"] = round(out[f"ctmul_tensor_{nt}_terms"]["GB_s"] / ip_rate, 3)
        line(f"ctmul_tensor_square_{nt}_terms", 8 * n * level * b * (2 * nt + 3),
             lambda nt=nt: ctx.ctmul_tensor(ops[0], ops[1], None, None, o0, o1, d2, b, level, nt))
        out[f"ctmul_tensor_square_{nt}_rate_over_inner_product"] = round(
            out[f"ctmul_tensor_square_{nt}_terms"]["GB_s"] / ip_rate, 3)

    # the pieces of the driver on the public calls
    t_raise = line("keyswitch_raise", 0, lambda: ctx.keyswitch_raise(d2, raised, b, level, alpha, level, k))
    down = torch.empty(2 * b * lw, dtype=torch.int64, device="cuda")
    t_down = line("ntt_moddown_both_components", 0, lambda: ctx.ntt_moddown(acc, down, 2 * b, level, level, k))
    t_resc = line("rescale_both_outputs", 0,
                  lambda: ctx.ntt_moddown(o01, o01, 2 * b, level - 1, level - 1, 1, in_stride=lw, out_stride=lw))
    line("keyswitch_add", 0, lambda: ctx.keyswitch(d2, rlk, o0, o1, b, level, level, alpha, level, k, mfhe.KS_ADD))

    # the driver
    t_mul = {}
    for nt in (1, 8):
        for flags, tag in ((0, ""), (mfhe.CTMUL_RESCALE, "_rescale")):
            t_mul[nt, flags] = line(f"ctmul_{nt}_terms{tag}", 0,
                                    lambda nt=nt, flags=flags: ctx.ctmul(ops[0], ops[1], ops[2], ops[3], rlk, o0, o1,
                                                                         b, level, level, alpha, level, k, nt, flags))
            pieces = {"tensor_ms": round(t_tensor[nt], 4), "raise_ms": round(t_raise, 4),
                      "inner_product_ms": round(t_ip, 4), "moddown_ms": round(t_down, 4),
                      "rescale_ms": round(t_resc if flags else 0.0, 4)}
            pieces["sum_ms"] = round(sum(pieces.values()), 4)
            out[f"ctmul_{nt}_terms{tag}_pieces"] = pieces

    # lazy relinearisation: one 8-term product against eight 1-term products summed by 7 ciphertext additions
    e01 = torch.empty_like(o01)
    s01 = torch.empty_like(o01)
    o01.zero_()
    e01.zero_()
    t_add = line("ciphertext_addition_pass", 3 * 8 * 2 * b * lw, lambda: torch.add(o01, e01, out=s01))
    for flags, tag in ((0, ""), (mfhe.CTMUL_RESCALE, "_rescale")):
        eager = 8 * t_mul[1, flags] + 7 * t_add
        out[f"lazy_relin_8_terms{tag}"] = {"ctmul_8_terms_ms": round(t_mul[8, flags], 4),
                                           "eight_products_plus_seven_additions_ms": round(eager, 4),
                                           "ratio": round(t_mul[8, flags] / eager, 3)}
    text = json.dumps(out)
    print(text, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
