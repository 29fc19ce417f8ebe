#!/usr/bin/env python3
"""Linear-transform timing lines (csrc/lintrans.hip) at N = 2^16, batch 64, alpha 3 on the 11 + 3 basis of
tools/keyswitch_bench.py, all from one run: lt_pt_mac at 4, 8 and 16 terms beside ksk_inner_product on the same rows
(the yardstick: the same kind of kernel, measured here again), lt_baby_step, lt_apply for 64 diagonals split as
(n1, n2) = (16, 4) and (8, 8), and on the parent's code paths keyswitch_raise + 64 x galois_apply_raised, the lower
bound of a transform done diagonal by diagonal (its plaintext products left out); ntt_moddown of both components of
one accumulator is timed too.  Prints one JSON line.

Timing: HIP events around a window of calls sized to >= 0.3 s after a warm-up of every shape, three windows each, the
median reported with the spread (tools/bconv_bench.py's method).  GB/s are a call's rate on its bytes model, not a
kernel's share of peak: lt_pt_mac 8 N (level + K) (2 npoly (nterms + 1) + nterms), the inner product
8 N (level + K) (npoly (ndigits + 2) + 2 ndigits), lt_baby_step the inner product's plus
24 N level npoly for the c0 term (read c0, read and write component 0 of the Q rows).

usage: tools/lintrans_bench.py [--log-n 16] [--batch 64] [--alpha 3] [--diagonals 64] [--min-window 0.3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--diagonals", type=int, default=64)
    ap.add_argument("--min-window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lintrans_bench needs a GPU")
    n, b, alpha, nd = 1 << a.log_n, a.batch, a.alpha, a.diagonals
    level, k = 11, 3
    rows = level + k
    beta = -(-level // alpha)
    m2 = 2 << a.log_n
    out = {"tool": "lintrans_bench", "date": datetime.date.today().isoformat(), "log_n": a.log_n, "batch": b,
           "basis": "11 + 3", "alpha": alpha, "ndigits": beta, "diagonals": nd,
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
    splits = [(16, nd // 16), (8, nd // 8)]
    max_baby = max(n1 for n1, _ in splits)
    ctx.lt_reserve(b, level, level, alpha, level, k, max_baby)

    c0 = residues(moduli[:level], b, n)
    c1 = residues(moduli[:level], b, n)
    nkeys = max(n1 - 1 + n2 - 1 for n1, n2 in splits)
    keys = [residues(moduli, 2 * beta, n) for _ in range(nkeys)]   # each [beta][2][14][N]
    raised = torch.cat([residues(moduli, b, n) for _ in range(beta)])
    acc = torch.empty(b * 2 * rows * n, dtype=torch.int64, device="cuda")
    o0 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")
    o1 = torch.empty(b * level * n, dtype=torch.int64, device="cuda")
    pt = residues(moduli, nd, n)                                   # [nd][14][N], pt_level = level
    slot_words = b * 2 * rows * n
    U = torch.empty(16 * slot_words, dtype=torch.int64, device="cuda")
    for s in range(16):                                            # canonical residues in every slot
        U[s * slot_words:(s + 1) * slot_words].copy_(residues(moduli, 2 * b, n))

    # the multiply-accumulate beside the inner product on the same rows
    ip_bytes = 8 * n * rows * (b * (beta + 2) + 2 * beta)
    t_ip = line("ksk_inner_product", ip_bytes,
                lambda: ctx.ksk_inner_product(raised, keys[0], acc, b, beta, level, level, level, k))
    ip_rate = out["ksk_inner_product"]["GB_s"]
    t_mac = {}
    for nt in (4, 8, 16):
        terms = list(range(nt))
        mac_bytes = 8 * n * rows * (2 * b * (nt + 1) + nt)
        t_mac[nt] = line(f"lt_pt_mac_{nt}_terms", mac_bytes,
                         lambda terms=terms: ctx.lt_pt_mac(U, pt, acc, terms, terms, b, level, level, k, 16, nd))
        out[f"lt_pt_mac_{nt}_rate_over_inner_product"] = round(out[f"lt_pt_mac_{nt}_terms"]["GB_s"] / ip_rate, 3)

    # one keyed baby step; the unrotated one
    bs_bytes = ip_bytes + 24 * n * level * b
    u0 = U[:slot_words]
    t_bs = line("lt_baby_step", bs_bytes,
                lambda: ctx.lt_baby_step(c0, raised, keys[0], u0, b, level, level, alpha, level, k, 5))
    line("lt_baby_step_keyless", 0, lambda: ctx.lt_baby_step(c0, c1, None, u0, b, level, level, alpha, level, k, 1))
    out["lt_baby_step_over_inner_product"] = round(t_bs / t_ip, 3)
    del U, u0
    torch.cuda.empty_cache()

    # the parent's pieces, and the transform diagonal by diagonal on them (plaintext products left out)
    t_raise = line("keyswitch_raise", 0, lambda: ctx.keyswitch_raise(c1, raised, b, level, alpha, level, k))
    t_rot = line("galois_apply_raised", 0,
                 lambda: ctx.galois_apply_raised(c0, raised, keys[0], o0, o1, b, level, level, alpha, level, k, 5))
    t_fresh = line("galois_apply", 0,
                   lambda: ctx.galois_apply(c0, c1, keys[0], o0, o1, b, level, level, alpha, level, k, 5))
    down = torch.empty(2 * b * level * n, dtype=torch.int64, device="cuda")
    t_down = line("ntt_moddown_both_components", 0, lambda: ctx.ntt_moddown(acc, down, 2 * b, level, level, k))
    gs = [pow(5, i + 1, m2) for i in range(nd)]

    def by_diagonal():
        ctx.keyswitch_raise(c1, raised, b, level, alpha, level, k)
        for i, g in enumerate(gs):
            ctx.galois_apply_raised(c0, raised, keys[i % nkeys], o0, o1, b, level, level, alpha, level, k, g)

    t_diag = line(f"raise_plus_{nd}_hoisted_rotations", 0, by_diagonal)

    # the transform
    for n1, n2 in splits:
        plan = mfhe.bsgs_plan(range(nd), n1, a.log_n)
        assert len(plan["baby_elt"]) == n1 and len(plan["giant_elt"]) == n2 and len(plan["term_step"]) == nd
        kb = [None] + keys[:n1 - 1]
        kg = [None] + keys[n1 - 1:n1 + n2 - 2]
        t = line(f"lt_apply_{n1}x{n2}", 0,
                 lambda plan=plan, kb=kb, kg=kg: ctx.lt_apply(c0, c1, pt, o0, o1, b, level, level, alpha, level, k,
                                                              plan["baby_elt"], plan["giant_elt"], kb, kg,
                                                              plan["term_giant"], plan["term_baby"]))
        out[f"lt_apply_{n1}x{n2}_over_by_diagonal"] = round(t / t_diag, 3)
        # this run's pieces of the same sum, for DESIGN.md 3.11's comparison with its estimate
        out[f"lt_apply_{n1}x{n2}_pieces"] = {"raise_ms": round(t_raise, 4), "baby_steps_ms": round((n1 - 1) * t_bs, 4),
                                             "pt_macs_ms": round(n2 * t_mac[n1], 4),
                                             "moddowns_ms": round(n2 * t_down, 4),
                                             "rotations_ms": round((n2 - 1) * t_fresh, 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
