#!/usr/bin/env python3
"""RLWE client-side timing lines (csrc/rlwe.hip) at N = 2^16, alpha 3 on the 11 + 3 basis of tools/keyswitch_bench.py,
all from one run: sample_uniform, sample_small, encrypt_sk, encrypt_pk and decrypt at 64 polynomials, beside
ksk_inner_product on 4 digits and 14 rows (the yardstick, measured here again); then rlwe_ksk_gen beside
Context.gen_switch_key at the same shape, their windows alternating.  Prints one JSON line and writes it to
profiles/rlwe_bench.json.

The bar: rlwe_ksk_gen draws a in registers and makes one pass over the key where gen_switch_key makes a dozen, so it
must not be slower; the margin is the run's own spread, the largest difference among the three windows of either call
(ksk_gen_vs_gen_switch_key: bar_met).

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  GB/s are a call's rate on its bytes model, not a
kernel's share of peak, in words of 8 bytes per residue: sample_uniform 1 (a written), sample_small 5 (written, the
NTT's read and write, the copy out), encrypt_sk 7 (e written, the NTT's read and write, e and m read, c0 and c1
written), encrypt_pk 13 (three small polynomials written, transformed and read, m read, c0 and c1 written), decrypt 3,
ksk_gen 6 per key-row residue (e written, transformed and read, both components written); the inner product
8 N (level + K) (npoly (ndigits + 2) + 2 ndigits).  A mask residue costs a quarter of a ChaCha20
block, about 250 integer operations, so sample_uniform's rate against the yardstick's says whether the mask kernel is
bound by the ALUs or by memory (alu_or_hbm).

usage: tools/rlwe_bench.py [--log-n 16] [--batch 64] [--alpha 3] [--min-window 0.3] [--out profiles/rlwe_bench.json]"""
import argparse
import datetime
import json
import statistics
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


def alternating(fa, fb, min_window):
    """(median, min, max, reps) of fa and of fb, three windows each, a window of one following a window of the other."""
    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = []
    for fn in (fa, fb):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps.append(max(3, int(min_window * 1e3 / max(timed(fn, 3), 1e-3)) + 1))
    ms = ([], [])
    for _ in range(3):
        ms[0].append(timed(fa, reps[0]))
        ms[1].append(timed(fb, reps[1]))
    return [(statistics.median(m), min(m), max(m), r) for m, r in zip(ms, reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rlwe_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rlwe_bench needs a GPU")
    n, b, alpha = 1 << a.log_n, a.batch, a.alpha
    level, k = 11, 3
    rows = level + k
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    out = {"tool": "rlwe_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "batch": b,
           "basis": "11 + 3", "alpha": alpha, "ndigits": beta, "device": torch.cuda.get_device_name(0)}

    def record(name, res, model_bytes):
        ms, lo, hi, reps = res
        out[name] = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps,
                     "model_GB": round(model_bytes / 1e9, 4), "GB_s": round(model_bytes / 1e9 / (ms * 1e-3), 1)}
        print(name, out[name], file=sys.stderr, flush=True)
        return ms

    def line(name, model_bytes, fn):
        return record(name, window(fn, a.min_window), model_bytes)

    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    ctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    out["ntt_arith"] = "u64" if ctx.info().arith == mfhe.ARITH_U64 else "f64"
    seed = mfhe.Seed(bytes(range(32)))
    empty = lambda words: torch.empty(words, dtype=torch.int64, device="cuda")

    # the yardstick
    rlk = residues(moduli, 2 * beta, n)                                 # [beta][2][14][N]
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    acc = empty(b * 2 * rows * n)
    line("ksk_inner_product", 8 * n * rows * (b * (beta + 2) + 2 * beta),
         lambda: ctx.ksk_inner_product(raised, rlk, acc, b, beta, level, level, level, k))
    ip_rate = out["ksk_inner_product"]["GB_s"]
    del raised, acc

    ctx.rlwe_reserve(b, level, level, k)
    res = 8 * n * rows * b                                              # the bytes of one word per residue
    s = ctx.rlwe_sample_small(seed, mfhe.RLWE_SECRET, 0, empty(rows * n), 1, level, level, k)
    m = residues(moduli, b, n)
    c0, c1 = empty(b * rows * n), empty(b * rows * n)
    t_uni = line("sample_uniform", res, lambda: ctx.rlwe_sample_uniform(seed, 1, c1, b, level, level, k))
    line("sample_small_noise", 5 * res, lambda: ctx.rlwe_sample_small(seed, mfhe.RLWE_NOISE, 1, c0, b, level, level, k))
    line("encrypt_sk", 7 * res, lambda: ctx.rlwe_encrypt_sk(seed, 1, s, m, c0, c1, b, level, level, k))
    resq = 8 * n * level * b
    pk0, pk1 = ctx.rlwe_encrypt_sk(seed, 0, s, None, empty(level * n), empty(level * n), 1, level)
    mq = residues(moduli[:level], b, n)
    q0, q1, dq = empty(b * level * n), empty(b * level * n), empty(b * level * n)
    line("encrypt_pk", 13 * resq, lambda: ctx.rlwe_encrypt_pk(seed, 1, pk0, pk1, mq, q0, q1, b, level))
    line("decrypt", 3 * resq, lambda: ctx.rlwe_decrypt(q0, q1, s, dq, b, level))
    # 4 residues and ~1000 integer operations to a block: the ALUs' time for sample_uniform against the memory's
    uni = out["sample_uniform"]
    out["alu_or_hbm"] = {"sample_uniform_rate_over_inner_product": round(uni["GB_s"] / ip_rate, 3),
                         "mask_kernel_bound": "ALU" if uni["GB_s"] < 0.5 * ip_rate else "HBM",
                         "encrypt_sk_minus_noise_ms": round(out["encrypt_sk"]["ms"] - out["sample_small_noise"]["ms"], 4),
                         "sample_uniform_ms": round(t_uni, 4)}

    # the key: one fused call beside the Python layer's dozen passes, windows alternating
    s2 = residues(moduli, 1, n)
    ksk = empty(beta * 2 * rows * n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    ra, rb = alternating(lambda: ctx.rlwe_ksk_gen(seed, 1, mfhe.RLWE_KEY_SWITCH, s, ksk, level, alpha, level, k, s_from=s2),
                         lambda: ctx.gen_switch_key(s2, s, level, alpha, level, k, generator=gen), a.min_window)
    t_new = record("ksk_gen", ra, 6 * 8 * n * rows * beta)
    t_old = record("gen_switch_key", rb, 6 * 8 * n * rows * beta)
    new, old = out["ksk_gen"], out["gen_switch_key"]
    spread = max(new["ms_max"] - new["ms_min"], old["ms_max"] - old["ms_min"])
    out["ksk_gen_vs_gen_switch_key"] = {"time_ratio": round(t_new / t_old, 3), "spread_ms": round(spread, 4),
                                        "bar_met": bool(t_new <= t_old + spread)}
    line("ksk_gen_relin", 6 * 8 * n * rows * beta,
         lambda: ctx.rlwe_ksk_gen(seed, 1, mfhe.RLWE_KEY_RELIN, s, ksk, level, alpha, level, k))
    line("ksk_gen_galois", 6 * 8 * n * rows * beta,
         lambda: ctx.rlwe_ksk_gen(seed, 1, mfhe.RLWE_KEY_GALOIS, s, ksk, level, alpha, level, k, galois_elt=5))
    text = json.dumps(out)
    print(text, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
