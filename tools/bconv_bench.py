#!/usr/bin/env python3
"""RNS basis conversion timing line (csrc/bconv.hip): rns_modup (3-limb digit into 14 rows), rns_moddown (14 rows to
11) and the NTT-domain pair at N = 2^16, batch 64 on the reference's 11 + 3 basis, with mfhe_crt_compose_f64 and
mfhe_rns_decompose on the same number of coefficients as the yardstick (the project's other per-coefficient
memory-bound kernels).  Prints one JSON line.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each,
the median reported with the spread.  GB/s are on the bytes the algorithm needs, 8 * (rows read + rows written) *
npoly * ncoeff, over the event time per call -- a call's rate, not a kernel's share of peak.

The reference's own primes have 2-adic order 8 .. 12 (no 2^17-th root), so the NTT-domain pair runs on primes of
the same bit sizes (45, 10 x 35 | 55, 40, 40) with q = 1 mod 2^17; the rns_* calls use the reference's primes.

usage: tools/bconv_bench.py [--log-n 16] [--batch 64] [--min-window 0.3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-fhe-gpu_amd"))
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import mfhe  # noqa: E402
from bench import gen_moduli  # noqa: E402


def window(fn, min_window):
    """ms per call: median and (min, max) of three event-timed windows of >= min_window seconds."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def timed(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    est = timed(10)
    reps = max(10, int(min_window * 1e3 / max(est, 1e-3)) + 1)
    ms = [timed(reps) for _ in range(3)]
    return statistics.median(ms), min(ms), max(ms), reps


def residues(moduli, batch, n):
    qt = torch.tensor(moduli, dtype=torch.int64, device="cuda").repeat_interleave(n).repeat(batch)
    d = torch.empty(batch * len(moduli) * n, dtype=torch.int64, device="cuda")
    d.random_(0, 2 ** 62).remainder_(qt)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--min-window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bconv_bench needs a GPU")
    n, b = 1 << a.log_n, a.batch
    out = {"tool": "bconv_bench", "log_n": a.log_n, "batch": b, "basis": "11 + 3", "device": torch.cuda.get_device_name(0)}

    def line(name, rows, fn):
        ms, lo, hi, reps = window(fn, a.min_window)
        gb = 8 * rows * b * n / 1e9
        out[name] = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps,
                     "model_GB": round(gb, 4), "GB_s": round(gb / (ms * 1e-3), 1)}

    # coefficient-domain calls on the reference's primes (no NTT tables needed; log_n only sizes them)
    ctx = mfhe.Context(mfhe.RNS_MODULI + mfhe.P_MODULI, 6, 0)
    ctx.rns_modup_reserve(11, 3, 3, 11, 3)
    ctx.rns_moddown_reserve(11, 11, 3)
    q11 = residues(mfhe.RNS_MODULI, b, n)
    r14 = residues(mfhe.RNS_MODULI + mfhe.P_MODULI, b, n)
    up = torch.empty(b * 14 * n, dtype=torch.int64, device="cuda")
    down = torch.empty(b * 11 * n, dtype=torch.int64, device="cuda")
    line("rns_modup_3_to_14", 3 + 14, lambda: ctx.rns_modup(q11, up, b, n, 11, 3, 3, 11, 3))
    line("rns_moddown_14_to_11", 14 + 11, lambda: ctx.rns_moddown(r14, down, b, n, 11, 11, 3))
    # yardsticks: the same b * n coefficients through the reference's 11-limb Q context (every q < 2^50: the FP64
    # compose, the product's default path); the 14-limb context (a 55-bit prime: the integer compose) beside it
    f = torch.empty(b * n, dtype=torch.float64, device="cuda")
    z = (torch.rand(b * n, dtype=torch.float64, device="cuda") - 0.5) * 1000.0
    qctx = mfhe.Context(mfhe.RNS_MODULI, 6, 0)
    line("crt_compose_f64_L11", 11 + 1, lambda: qctx.crt_compose_f64(q11, f, b, n))
    line("rns_decompose_L11", 1 + 11, lambda: qctx.rns_decompose(z, down, b, n))
    line("crt_compose_f64_L14", 14 + 1, lambda: ctx.crt_compose_f64(r14, f, b, n))
    line("rns_decompose_L14", 1 + 14, lambda: ctx.rns_decompose(z, up, b, n))
    del ctx, qctx
    # NTT-domain pair: same bit sizes, q = 1 mod 2N
    m2 = 2 << a.log_n
    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    nctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    nctx.rns_modup_reserve(11, 3, 3, 11, 3)
    nctx.rns_moddown_reserve(11, 11, 3)
    nctx.ntt_bconv_reserve(b, 14)
    e11 = residues(moduli[:11], b, n)
    e14 = residues(moduli, b, n)
    line("ntt_modup_3_to_14", 3 + 14, lambda: nctx.ntt_modup(e11, up, b, 11, 3, 3, 11, 3))
    line("ntt_moddown_14_to_11", 14 + 11, lambda: nctx.ntt_moddown(e14, down, b, 11, 11, 3))
    out["ntt_arith"] = "u64" if nctx.info().arith == mfhe.ARITH_U64 else "f64"
    y = min(out["crt_compose_f64_L11"]["GB_s"], out["rns_decompose_L11"]["GB_s"])
    out["yardstick_GB_s"] = y
    out["modup_over_yardstick"] = round(out["rns_modup_3_to_14"]["GB_s"] / y, 3)
    out["moddown_over_yardstick"] = round(out["rns_moddown_14_to_11"]["GB_s"] / y, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
