#!/usr/bin/env python3
"""Slot encoder timing lines (csrc/slot.hip) at N = 2^16, 64 polynomials on the 11 + 3 basis of
tools/keyswitch_bench.py, all from one run: slot_encode onto 14 rows and onto 11 rows in the coefficient form, ntt_fwd
of those rows alone, slot_encode in the evaluation form, the SLOT_REAL form, slot_decode in both forms, beside
ksk_inner_product on 4 digits and 14 rows (the yardstick, measured here again).  Prints one JSON line and writes it to
profiles/slot_bench.json.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  Every line has two byte counts: the algorithmic
bytes (encode_bytes / decode_bytes below: slots in, residues out, or the d rows in and the slots out) and the moved
bytes, which add the two-pass intermediate's write and read (two_pass_bytes; log_n >= 14, see WHOLE_MAX_LOG).  GB/s and the rate over
the yardstick's are given on both.

usage: tools/slot_bench.py [--log-n 16] [--batch 64] [--min-window 0.3] [--out profiles/slot_bench.json]"""
import argparse
import datetime
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def encode_bytes(n, npoly, rows, real=False):
    """Algorithmic bytes of slot_encode: N doubles of slots in (N / 2 with SLOT_REAL), rows x N words out."""
    return 8 * n * npoly * ((0.5 if real else 1) + rows)


def decode_bytes(n, npoly, d):
    """Algorithmic bytes of slot_decode: d rows of N words in, N doubles of slots out."""
    return 8 * n * npoly * (d + 1)


# csrc/slot.hpp kSlotWholeMaxLog: up to N / 2 = 2^12 points a transform is one launch with no intermediate.  A mirror
# of the library's constant, not read from it; tests/test_slot_cpu.py fails if the two part.
WHOLE_MAX_LOG = 12


def two_pass_bytes(log_n, npoly):
    """What the two-launch form also moves: the [npoly][N / 2] complex intermediate written and read once."""
    return 2 * 8 * (1 << log_n) * npoly if log_n - 1 > WHOLE_MAX_LOG else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "slot_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT / "matrix-fhe-gpu_amd"))
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tools"))
    import torch
    import mfhe
    from bench import gen_moduli
    from bconv_bench import residues, window
    if not torch.cuda.is_available():
        sys.exit("slot_bench needs a GPU")
    n, b = 1 << a.log_n, a.batch
    level, k = 11, 3
    rows, beta = level + k, 4
    m2 = 2 << a.log_n
    scale = 2.0 ** 40
    out = {"tool": "slot_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "batch": b,
           "basis": "11 + 3", "scale": "2^40", "device": torch.cuda.get_device_name(0)}
    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    ctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    out["ntt_arith"] = "u64" if ctx.info().arith == mfhe.ARITH_U64 else "f64"
    ctx.slot_reserve(b, level, level, k)
    extra = two_pass_bytes(a.log_n, b)
    ip_rate = [None]

    def line(name, model_bytes, fn, moved=None):
        ms, lo, hi, reps = window(fn, a.min_window)
        e = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps}
        if model_bytes:
            moved = model_bytes if moved is None else moved
            e["model_GB"] = round(model_bytes / 1e9, 4)
            e["moved_GB"] = round(moved / 1e9, 4)
            e["GB_s"] = round(model_bytes / 1e9 / (ms * 1e-3), 1)
            e["moved_GB_s"] = round(moved / 1e9 / (ms * 1e-3), 1)
            if ip_rate[0]:
                e["rate_over_inner_product"] = round(e["GB_s"] / ip_rate[0], 3)
                e["moved_rate_over_inner_product"] = round(e["moved_GB_s"] / ip_rate[0], 3)
        out[name] = e
        return ms

    # the yardstick
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    rlk = residues(moduli, 2 * beta, n)
    acc = torch.empty(b * 2 * rows * n, dtype=torch.int64, device="cuda")
    line("ksk_inner_product", 8 * n * rows * (b * (beta + 2) + 2 * beta),
         lambda: ctx.ksk_inner_product(raised, rlk, acc, b, beta, level, level, level, k))
    ip_rate[0] = out["ksk_inner_product"]["GB_s"]
    del raised, rlk, acc

    z = torch.rand(b * n, dtype=torch.float64, device="cuda").view(torch.complex128)       # [b][n / 2] complex
    zr = torch.rand(b * n // 2, dtype=torch.float64, device="cuda")
    r14 = torch.empty(b * rows * n, dtype=torch.int64, device="cuda")
    r11 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")
    back = torch.empty_like(z)
    C = mfhe.SLOT_COEFF
    line("encode_14_rows_coeff", encode_bytes(n, b, rows), lambda: ctx.slot_encode(z, r14, b, level, scale, level, k, C),
         encode_bytes(n, b, rows) + extra)
    line("encode_11_rows_coeff", encode_bytes(n, b, level), lambda: ctx.slot_encode(z, r11, b, level, scale, flags=C),
         encode_bytes(n, b, level) + extra)
    sp_rows = r14[:b * k * n]

    def ntt14():
        ctx.ntt_fwd(r11, b, 0, level)
        ctx.ntt_fwd(sp_rows, b, level, k)

    line("ntt_fwd_14_rows", 2 * 8 * n * b * rows, ntt14)
    line("ntt_fwd_11_rows", 2 * 8 * n * b * level, lambda: ctx.ntt_fwd(r11, b, 0, level))
    # the evaluation form: 14 rows go through the dense blocks (two-pass NTTs: 4 row passes, the copies: 2); 11 dense
    # rows are transformed in place (4 row passes)
    line("encode_14_rows_eval", encode_bytes(n, b, rows), lambda: ctx.slot_encode(z, r14, b, level, scale, level, k),
         encode_bytes(n, b, rows) + extra + 6 * 8 * n * b * rows)
    line("encode_11_rows_eval", encode_bytes(n, b, level), lambda: ctx.slot_encode(z, r11, b, level, scale),
         encode_bytes(n, b, level) + extra + 4 * 8 * n * b * level)
    line("encode_14_rows_coeff_real", encode_bytes(n, b, rows, True),
         lambda: ctx.slot_encode(zr, r14, b, level, scale, level, k, C | mfhe.SLOT_REAL),
         encode_bytes(n, b, rows, True) + extra)
    ctx.slot_encode(z, r11, b, level, scale, flags=C)
    line("decode_coeff", decode_bytes(n, b, 2), lambda: ctx.slot_decode(r11, back, b, level, scale, C),
         decode_bytes(n, b, 2) + extra)
    ctx.slot_encode(z, r11, b, level, scale)
    # the evaluation form copies the two rows out (2 row passes) and inverse-transforms them (4)
    line("decode_eval", decode_bytes(n, b, 2), lambda: ctx.slot_decode(r11, back, b, level, scale),
         decode_bytes(n, b, 2) + extra + 6 * 8 * n * b * 2)
    torch.cuda.synchronize()
    out["round_trip_max_error"] = float((back - z).abs().max())
    text = json.dumps(out)
    print(text, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
