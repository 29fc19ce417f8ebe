#!/usr/bin/env python3
"""The launches of the key switch and its four drivers, for comparing two builds of the library (MFHE_LIB picks the
build): one call each of keyswitch, galois_apply, lt_apply (a 2 x 2 baby-step / giant-step plan), ctmul with
CTMUL_RESCALE and ctmat (2 x 3 by 3 x 2) at N = 16, level 5, K = 2, alpha 2, npoly 3.  Launches do not depend on the
data, so the operands are random residues.

  rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/ks_launch_trace.py run
  python tools/ks_launch_trace.py list DIR > profiles/ks_launch_trace_<build>.txt

The `he` scenario does the same for the pipelines of he.hip: one call each of keygen, encode, encrypt_pair,
decrypt_to_eval and decrypt_and_decode at n = 8, L = 3 (the first three reference moduli), under the default options
and again with MFHE_OPT_HE_STREAMS 0, HE_STREAMS 2, HE_FUSED 0 and WCRT_MFMA 0 (run `he` in place of `run`;
profiles/he_launch_trace_<build>.txt).

`list` prints the tool's name and then one line per dispatch, in dispatch order: kernel name, grid and workgroup size
in threads.  Two builds launch alike when their lists are equal."""
import csv
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LOG_N, LEVEL, K, ALPHA, NPOLY = 4, 5, 2, 2, 3


def run():
    sys.path.insert(0, str(ROOT / "matrix-fhe-gpu_amd"))
    sys.path.insert(0, str(ROOT))
    import torch
    import mfhe
    from bench import gen_moduli

    n, m2 = 1 << LOG_N, 2 << LOG_N
    moduli = gen_moduli(50, m2, LEVEL + K)
    ctx = mfhe.Context(moduli, LOG_N, mfhe.CONV_PHANTOM)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(rows_moduli, count):   # [count][len(rows_moduli)][n] residues
        q = torch.tensor(rows_moduli, dtype=torch.int64, device="cuda")[None, :, None]
        x = torch.randint(0, 1 << 49, (count, len(rows_moduli), n), generator=gen, device="cuda", dtype=torch.int64)
        return (x % q).reshape(-1).contiguous()

    def empty(count):
        return torch.empty(count * LEVEL * n, dtype=torch.int64, device="cuda")

    beta = -(-LEVEL // ALPHA)
    geom = (LEVEL, LEVEL, ALPHA, LEVEL, K)
    key = lambda: rnd(moduli, 2 * beta)   # noqa: E731  [beta][2][level + K][n]
    q = moduli[:LEVEL]
    c0, c1 = rnd(q, NPOLY), rnd(q, NPOLY)
    ctx.keyswitch(c1, key(), empty(NPOLY), empty(NPOLY), NPOLY, *geom)
    ctx.galois_apply(c0, c1, key(), empty(NPOLY), empty(NPOLY), NPOLY, *geom, mfhe.galois_elt(1, LOG_N))
    # diagonals 0 .. 3 as 2 baby steps by 2 giant steps
    baby, giant = [1, mfhe.galois_elt(1, LOG_N)], [1, mfhe.galois_elt(2, LOG_N)]
    ctx.lt_apply(c0, c1, rnd(moduli, 4), empty(NPOLY), empty(NPOLY), NPOLY, *geom, baby, giant, [None, key()],
                 [None, key()], [0, 0, 1, 1], [0, 1, 0, 1])
    ctx.ctmul(c0, c1, rnd(q, NPOLY), rnd(q, NPOLY), key(), empty(NPOLY), empty(NPOLY), NPOLY, *geom,
              flags=mfhe.CTMUL_RESCALE)
    a0, a1, b0, b1 = (rnd(q, 6 * NPOLY) for _ in range(4))
    ctx.ctmat(a0, a1, b0, b1, key(), empty(4 * NPOLY), empty(4 * NPOLY), 2, 2, 3, NPOLY, *geom)
    torch.cuda.synchronize()


def run_he():
    sys.path.insert(0, str(ROOT / "matrix-fhe-gpu_amd"))
    import torch
    import mfhe

    log_n, L = 3, 3
    n2 = 1 << (2 * log_n)
    words = 512 * L * n2
    ctx = mfhe.Context(mfhe.RNS_MODULI[:L], log_n, mfhe.CONV_PHANTOM | mfhe.CONV_WCRT)
    gen = torch.Generator(device="cuda").manual_seed(1)
    msg = torch.rand(2 * 512 * n2, generator=gen, device="cuda", dtype=torch.float64)
    sk = torch.empty(512 * L << log_n, dtype=torch.int64, device="cuda")
    re, im, ev = (torch.empty(words, dtype=torch.int64, device="cuda") for _ in range(3))
    cre, cim = (torch.empty(2 * words, dtype=torch.int64, device="cuda") for _ in range(2))
    out = torch.empty_like(msg)
    defaults = {o: ctx.get_option(o) for o in (mfhe.OPT_HE_STREAMS, mfhe.OPT_HE_FUSED, mfhe.OPT_WCRT_MFMA)}
    for opt, value in ((None, None), (mfhe.OPT_HE_STREAMS, 0), (mfhe.OPT_HE_STREAMS, 2), (mfhe.OPT_HE_FUSED, 0),
                       (mfhe.OPT_WCRT_MFMA, 0)):
        for o, v in defaults.items():
            ctx.set_option(o, value if o == opt else v)
        ctx.keygen(sk)
        ctx.encode(msg, re, im)
        ctx.encrypt_pair(re, im, sk, cre, cim)
        ctx.decrypt_to_eval(cre, sk, ev)
        ctx.decrypt_and_decode(cre, cim, sk, out)
        torch.cuda.synchronize()


def listing(d):
    files = sorted(Path(d).rglob("*kernel_trace.csv"))
    if len(files) != 1:
        sys.exit(f"expected one kernel trace under {d}, found {len(files)}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Dispatch_Id"]))
    print("# tools/ks_launch_trace.py: kernel, grid (threads), workgroup")
    for r in rows:
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        print(f'{r["Kernel_Name"]} {grid} {wg}')


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 2 and sys.argv[1] == "he":
        run_he()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
