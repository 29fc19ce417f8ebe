#!/usr/bin/env python3
"""Polynomial-evaluation timing lines (csrc/lincomb.hip, csrc/poly.hip) at N = 2^16, batch 64, alpha 3 on the 11 + 3
basis of tools/keyswitch_bench.py, all from one run: ct_lincomb at 2, 8 and 32 terms (level 11, with the addend) beside
lt_pt_mac fed the same sums -- the same source buffer, constant-filled plaintexts, on the narrowest geometry it accepts
(one special row, so 12 rows where ct_lincomb reads and writes 11) -- and beside ksk_inner_product on 4 digits and 14
rows (the yardstick, measured here again); then poly_apply at Chebyshev degrees 7, 15 and 31 with its share in
products, sums and rescales, each node's three pieces timed on the public calls at the node's own level and term
count.  Prints one JSON line and writes it to profiles/poly_bench.json.

The bar: ct_lincomb moves the ciphertext bytes of lt_pt_mac (fewer here, by the special row) and no plaintext rows, so
it must not be slower; the margin is the run's own spread, the largest difference among the three windows of either
call (lincomb_N_terms_vs_pt_mac: bar_met).

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  GB/s are a call's rate on its bytes model, not a
kernel's share of peak: ct_lincomb 8 N npoly 2 level (nterms + 1), lt_pt_mac 8 N (level + K) (2 npoly (nterms + 1) +
nterms), the inner product 8 N (level + K) (npoly (ndigits + 2) + 2 ndigits).

usage: tools/poly_bench.py [--log-n 16] [--batch 64] [--alpha 3] [--min-window 0.3] [--out profiles/poly_bench.json]"""
import argparse
import datetime
import json
import random
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

TERMS = (2, 8, 32)
DEGREES = (7, 15, 31)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "poly_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("poly_bench needs a GPU")
    n, b, alpha = 1 << a.log_n, a.batch, a.alpha
    level, k = 11, 3
    rows = level + k
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    out = {"tool": "poly_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "batch": b,
           "basis": "11 + 3", "alpha": alpha, "ndigits": beta, "device": torch.cuda.get_device_name(0)}

    def line(name, model_bytes, fn):
        ms, lo, hi, reps = window(fn, a.min_window)
        out[name] = {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps}
        if model_bytes:
            out[name]["model_GB"] = round(model_bytes / 1e9, 4)
            out[name]["GB_s"] = round(model_bytes / 1e9 / (ms * 1e-3), 1)
        print(name, out[name], file=sys.stderr, flush=True)
        return ms

    moduli = gen_moduli(45, m2, 1) + gen_moduli(35, m2, 10) + gen_moduli(55, m2, 1) + gen_moduli(40, m2, 2)
    ctx = mfhe.Context(moduli, a.log_n, mfhe.CONV_PHANTOM)
    out["ntt_arith"] = "u64" if ctx.info().arith == mfhe.ARITH_U64 else "f64"
    lw = level * n

    # the yardstick
    rlk = residues(moduli, 2 * beta, n)                                 # [beta][2][14][N]
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    acc = torch.empty(b * 2 * rows * n, dtype=torch.int64, device="cuda")
    line("ksk_inner_product", 8 * n * rows * (b * (beta + 2) + 2 * beta),
         lambda: ctx.ksk_inner_product(raised, rlk, acc, b, beta, level, level, level, k))
    ip_rate = out["ksk_inner_product"]["GB_s"]
    del raised

    # the same sums through both kernels: u [32][b][2][12][N], one special row
    kk, prow, nk = 1, level + 1, 8
    nslots = max(TERMS)
    slot = b * 2 * prow * n
    pmod = moduli[:level] + moduli[level:level + kk]
    u = torch.empty(nslots * slot, dtype=torch.int64, device="cuda")
    for s in range(nslots):
        u[s * slot:(s + 1) * slot].copy_(residues(pmod, 2 * b, n))
    rnd = random.Random(5)
    K = [[rnd.randrange(q) for q in pmod] for _ in range(nk)]
    d_k = mfhe.to_device_u64([v for row in K for v in row])
    pt = mfhe.to_device_u64([v for row in K for v in row]).repeat_interleave(n)          # [nk][12][N], constant rows
    macc = torch.empty(b * 2 * prow * n, dtype=torch.int64, device="cuda")
    l0 = torch.empty(b * lw, dtype=torch.int64, device="cuda")
    l1 = torch.empty(b * lw, dtype=torch.int64, device="cuda")
    for nt in TERMS:
        tx, tk = list(range(nt)), [t % nk for t in range(nt)]
        t_lin = line(f"ct_lincomb_{nt}_terms", 8 * n * b * 2 * level * (nt + 1),
                     lambda: ctx.ct_lincomb(u, u[prow * n:], d_k, l0, l1, tx, tk, b, level, nslots, nk, nk - 1,
                                            src_stride=slot, x_poly_stride=2 * prow * n, k_stride=prow))
        t_mac = line(f"lt_pt_mac_{nt}_terms", 8 * n * prow * (2 * b * (nt + 1) + nt),
                     lambda: ctx.lt_pt_mac(u, pt, macc, tx, tk, b, level, level, kk, nslots, nk))
        lin, mac = out[f"ct_lincomb_{nt}_terms"], out[f"lt_pt_mac_{nt}_terms"]
        spread = max(lin["ms_max"] - lin["ms_min"], mac["ms_max"] - mac["ms_min"])
        out[f"lincomb_{nt}_terms_vs_pt_mac"] = {"time_ratio": round(t_lin / t_mac, 3), "spread_ms": round(spread, 4),
                                                "bar_met": bool(t_lin <= t_mac + spread),
                                                "rate_over_pt_mac": round(lin["GB_s"] / mac["GB_s"], 3),
                                                "rate_over_inner_product": round(lin["GB_s"] / ip_rate, 3)}
    del u, pt, macc

    # the driver, and every node's pieces on the public calls at the node's level
    c0, c1 = residues(moduli[:level], b, n), residues(moduli[:level], b, n)
    x01 = torch.cat([residues(moduli[:level], 2 * b, n) for _ in range(3)])    # three ciphertexts, components adjacent
    y01 = torch.empty(2 * b * lw, dtype=torch.int64, device="cuda")
    pieces = {}

    def piece(kind, lv, nt):
        if (kind, lv, nt) not in pieces:
            if kind == "product":
                fn = lambda: ctx.ctmul(x01, x01[b * lw:], x01[2 * b * lw:], x01[3 * b * lw:], rlk, y01, y01[b * lw:], b, lv,
                                       level, alpha, level, k, 1, 0, a_poly_stride=lw, b_poly_stride=lw, out_stride=lw)
            elif kind == "sum":
                fn = lambda: ctx.ct_lincomb(x01, x01[b * lw:], d_k, y01, y01[b * lw:], [t % 3 for t in range(nt)],
                                            [t % nk for t in range(nt)], b, lv, 3, nk, nk - 1, src_stride=2 * b * lw,
                                            x_poly_stride=lw, k_stride=prow, out_stride=lw)
            else:
                fn = lambda: ctx.ntt_moddown(y01, y01, 2 * b, lv - 1, lv - 1, 1, in_stride=lw, out_stride=lw)
            pieces[kind, lv, nt] = window(fn, a.min_window)[0]
        return pieces[kind, lv, nt]

    for d in DEGREES:
        coeffs = [rnd.uniform(-1, 1) for _ in range(d + 1)]
        plan = ctx.poly_plan(coeffs, mfhe.POLY_CHEBYSHEV, 2.0 ** 35, level)
        info = plan.info()
        ctx.poly_reserve(plan, b, level, alpha, level, k)
        o0 = torch.empty(b * info.out_level * n, dtype=torch.int64, device="cuda")
        o1 = torch.empty(b * info.out_level * n, dtype=torch.int64, device="cuda")
        t_apply = line(f"poly_apply_degree_{d}", 0,
                       lambda: ctx.poly_apply(plan, c0, c1, rlk, o0, o1, b, level, alpha, level, k))
        t_mul = t_sum = t_res = 0.0
        for nd in plan.nodes():
            if nd["mul_a"] >= 0:
                t_mul += piece("product", nd["level"], 1)
            t_sum += piece("sum", nd["level"], len(nd["terms"]) + (nd["mul_a"] >= 0))
            t_res += piece("rescale", nd["level"], 0)
        total = t_mul + t_sum + t_res
        out[f"poly_apply_degree_{d}"].update({
            "nodes": info.nnodes, "products": info.nmul, "registers": info.nreg, "depth": info.depth,
            "products_ms": round(t_mul, 4), "sums_ms": round(t_sum, 4), "rescales_ms": round(t_res, 4),
            "pieces_sum_ms": round(total, 4), "products_share": round(t_mul / total, 3),
            "sums_share": round(t_sum / total, 3), "rescales_share": round(t_res / total, 3)})
        plan.close()
    text = json.dumps(out)
    print(text, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
