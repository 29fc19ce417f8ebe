"""mfhe -- Python host layer over libmfhe.so (include/mfhe.h), the MI355X backend for the
Matrix-FHE-GPU hot path (batched NTT/INTT, wide RNS CRT encode/decode).

The reference exposes this path through C++ (include/core/*.cuh) and phantom-fhe; this
module mirrors that surface for tests and benchmarks.  PyTorch is used only for device
memory and streams: every tensor is handed to the native library as a raw pointer.
There is no CPU or PyTorch fallback -- if libmfhe.so is missing or fails to load, import
raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from pathlib import Path

_PKG_DIR = Path(__file__).resolve().parent.parent          # matrix-fhe-gpu_amd/
REPO_ROOT = _PKG_DIR.parent
# MFHE_LIB: load a tuning-variant build instead (tools only; the product path is libmfhe.so)
LIB_PATH = Path(os.environ["MFHE_LIB"]) if os.environ.get("MFHE_LIB") else _PKG_DIR / "libmfhe.so"
HEADER = REPO_ROOT / "include" / "mfhe.h"

OK, EINVAL, EUNSUPPORTED, EHIP, ENOMEM, ENOTREADY = 0, 1, 2, 3, 4, 5
CONV_PHANTOM, CONV_GL, CONV_WCRT = 1, 2, 4
ARITH_AUTO, ARITH_F64, ARITH_U64 = 0, 1, 2
OPT_NTT_CHUNK_BYTES, OPT_NTT_PLAN, OPT_CRT_WORDS, OPT_NTT_WG_PER_CU, OPT_NTT_PREFETCH = 1, 2, 3, 4, 5
OPT_NTT_FUSED, OPT_WCRT_MFMA = 6, 9   # OPT_NTT_FUSED: removed in r04, only 0 accepted
OPT_CGEMM_MFMA, OPT_HE_FUSED, OPT_TRACE_SPLIT = 10, 11, 12
XCHG_ALLGATHER, XCHG_ALLTOALL = 0, 1
BCONV_FAST, BCONV_CENTERED = 0, 1
KS_ADD = 1                      # keyswitch: add the results to what out0 / out1 hold (relinearisation)
CTMUL_RESCALE = 1               # ctmul: after relinearising, ModDown both outputs by limb level - 1
PTMUL_RESCALE = 1               # ptmat: after the product, ModDown both outputs by limb level - 1
PTMUL_ADD = 2                   # ptmat_tensor / ptmat: the outputs' present contents are added into the sums
POLY_MONOMIAL = 0               # PolyPlan: sum a_i x^i
POLY_CHEBYSHEV = 1              # PolyPlan: sum a_i T_i(x), slots in [-1, 1]
SLOT_REAL = 1                   # slot_encode / slot_decode: real slots, N / 2 doubles per polynomial
SLOT_COEFF = 2                  # slot_encode / slot_decode: residues in the coefficient domain (no NTT)
RLWE_MASK, RLWE_NOISE, RLWE_SECRET, RLWE_EPHEMERAL, RLWE_NOISE0, RLWE_NOISE1 = 1, 2, 3, 4, 5, 6   # rlwe_*: streams
RLWE_COEFF = 1                  # rlwe_sample_small / rlwe_lift_small: coefficient domain (no forward NTT)
RLWE_KEY_SWITCH, RLWE_KEY_RELIN, RLWE_KEY_GALOIS = 0, 1, 2   # rlwe_ksk_gen: where s_from comes from
RECOMBINE_ROWS_GLOBAL = 1
RECOMBINE_EXCHANGE_ONLY = 2     # measurement: exchanges only, composes skipped (out untouched)
RECOMBINE_AFTER_PREV = 4        # the shard was complete when the previous chunked call on the comm was entered
RECOMBINE_AGREE = 8             # end with an all-rank status agreement (host wait)
RECOMBINE_COMPOSE_ONLY = 16     # measurement: composes only, out of the receive halves' last exchanged chunks
RECOMBINE_SELF_EXCHANGE = 32    # test hook: world 1 runs the exchange pipeline (RCCL self-exchange) anyway
RECOMBINE_DEBUG_FAIL = 256      # test hook: the compose of chunk 1 (or 0) fails
OPT_NTT_PACK = 13
OPT_WCRT_PIPE = 14
OPT_NTT_PLAN_EFFECTIVE = 15   # read-only: 4 pipelined single pass (2^14 FP64), 1 single pass, 2 two passes
OPT_NTT_U60 = 17              # U64 NTTs with every modulus < 2^60: 1 = lazy U60 schedules (default), 0 = Harvey
OPT_HE_STREAMS = 18           # encode / encrypt_pair / decrypt_and_decode re/im chains: 3 = encode pairs + decode side stream (default), 2 = pairs, 1 = side stream, 0 = one stream
OPT_ENC_A_DIRECT = 19         # encrypt (fused ring): 1 = the GEMM writes a into both ciphertexts (default), 0 = ring kernel copies it
OPT_ENC_E_SMALL = 21          # encrypt: 1 = the noise's W-CRT as the dense product with its one digit (default), 0 = factored
OPT_DEC_MM = 20               # removed in r06 (the decrypt's ring product on the matrix cores): only 0 accepted; was FP64 X-NTT rows (default)
COMM_ID_BYTES = 128

#: reference parameters (include/core/config.h:7-52)
RNS_MODULI = [
    17592186435073, 17182765057, 17184541441, 17186120449, 17186515201, 17186909953,
    17188883713, 17190462721, 17190857473, 17191844353, 17192831233,
]
P_MODULI = [18014398515156481, 549757491457, 549759662593]
MATRIX_N = 64
BATCH_SIZE = 512
BATCH_PRIME_P = 771
SCALING_FACTOR = 2.0 ** 35


class MfheError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mfhe error {code}: {msg}")
        self.code = code


def _load() -> ctypes.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} not built; run `make -C {_PKG_DIR}` (or __graft_entry__.build())")
    return ctypes.CDLL(str(LIB_PATH), mode=ctypes.RTLD_GLOBAL)


lib = _load()

_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


class CtxInfo(ctypes.Structure):
    _fields_ = [
        ("num_limbs", ctypes.c_int), ("log_n", ctypes.c_int), ("crt_words", ctypes.c_int),
        ("arith", ctypes.c_int), ("conventions", ctypes.c_int), ("phi", ctypes.c_int),
        ("delta", ctypes.c_double),
    ]


def _sig(name, argtypes, restype=ctypes.c_int):
    f = getattr(lib, name)
    f.argtypes = argtypes
    f.restype = restype
    return f


_sig("mfhe_ctx_create", [_u64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(_vp)])
_sig("mfhe_ctx_destroy", [_vp])
_sig("mfhe_ctx_get_info", [_vp, ctypes.POINTER(CtxInfo)])
_sig("mfhe_ctx_set_arith", [_vp, ctypes.c_int])
_sig("mfhe_ctx_get_moduli", [_vp, _u64p, ctypes.c_int])
_sig("mfhe_ctx_set_option", [_vp, ctypes.c_int, ctypes.c_int64])
_sig("mfhe_ctx_get_option", [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)])
for _n in ("mfhe_ntt_fwd", "mfhe_ntt_inv", "mfhe_gl_ntt_fwd", "mfhe_gl_ntt_inv", "mfhe_cyclic_ntt_fwd",
           "mfhe_cyclic_ntt_inv"):
    _sig(_n, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _vp])
_sig("mfhe_gl_perm", [_vp, _vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _vp])
_sig("mfhe_ntt_tables", [_vp] + [ctypes.POINTER(_vp)] * 6)
_sig("mfhe_ntt_dmodulus", [_vp, ctypes.POINTER(_vp)])
_sig("mfhe_fnwt_1d", [_vp, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp])
_sig("mfhe_inwt_1d", [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp])
_sig("mfhe_rns_decompose", [_vp, _vp, _sz, _sz, _sz, _vp, _vp])
_sig("mfhe_crt_compose", [_vp, _vp, _sz, _sz, _vp, _vp, _vp])
_sig("mfhe_crt_to_f64", [_vp, _vp, _vp, _sz, _vp, _sz, _vp])
_sig("mfhe_crt_compose_i64", [_vp, _vp, _sz, _sz, _vp, _vp])
_sig("mfhe_crt_compose_f64", [_vp, _vp, _sz, _sz, _vp, _sz, _vp])
_sig("mfhe_crt_compose_f64_sharded", [_vp, _vp, ctypes.c_int, _sz, _sz, _sz, _vp, _sz, _vp])
_int = ctypes.c_int
_sig("mfhe_rns_bconv_reserve", [_vp, _int, _int, _int, _int])
_sig("mfhe_rns_bconv", [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_rns_moddown", [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _int, _int, _int, _vp])
_sig("mfhe_rns_modup", [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_ntt_bconv_reserve", [_vp, _sz, _int])
_sig("mfhe_ntt_modup", [_vp, _vp, _sz, _vp, _sz, _sz, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_ntt_moddown", [_vp, _vp, _sz, _vp, _sz, _sz, _int, _int, _int, _vp])
_sig("mfhe_ksk_assemble", [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _vp])
_sig("mfhe_ksk_inner_product", [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_keyswitch_reserve", [_vp, _sz, _int, _int, _int, _int, _int])
_sig("mfhe_keyswitch", [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_ntt_automorphism", [_vp, _vp, _sz, _vp, _sz, _sz, _int, _int, _vp])
_sig("mfhe_ksk_inner_product_galois",
     [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_keyswitch_raise", [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _int, _int, _int, _int, _vp])
_sig("mfhe_galois_apply_raised",
     [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_galois_apply", [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_galois_reserve", [_vp, _sz, _int, _int, _int, _int, _int])


class LtPlan(ctypes.Structure):
    """mfhe_lt_plan (include/mfhe.h): host arrays, read during the call only."""
    _fields_ = [
        ("n_baby", _int), ("n_giant", _int), ("nterms", _int),
        ("baby_elt", ctypes.POINTER(_int)), ("giant_elt", ctypes.POINTER(_int)),
        ("d_gk_baby", ctypes.POINTER(_vp)), ("d_gk_giant", ctypes.POINTER(_vp)),
        ("term_giant", ctypes.POINTER(_int)), ("term_baby", ctypes.POINTER(_int)),
    ]


LT_MAX_TERMS = 64               # lt_pt_mac: most terms of one sum (one giant step of a plan)
_intp = ctypes.POINTER(_int)
_sig("mfhe_lt_baby_step", [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _int, _vp])
_sig("mfhe_lt_pt_mac",
     [_vp, _vp, _sz, _sz, _int, _vp, _sz, _int, _int, _vp, _sz, _intp, _intp, _int, _sz, _int, _int, _int, _vp])
_sig("mfhe_lt_reserve", [_vp, _sz, _int, _int, _int, _int, _int, _int])
_sig("mfhe_lt_apply", [_vp, ctypes.POINTER(LtPlan), _vp, _vp, _sz, _vp, _sz, _int, _vp, _vp, _sz, _sz, _int, _int, _int,
                       _int, _int, _vp])
CTMUL_MAX_TERMS = 64            # ctmul_tensor / ctmul: most terms of one sum
_sig("mfhe_ctmul_tensor", [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _int, _vp, _vp, _sz, _vp, _sz, _sz, _int, _vp])
_sig("mfhe_ctmul_reserve", [_vp, _sz, _int, _int, _int, _int, _int, _int])
_sig("mfhe_ctmul_apply", [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _int, _vp, _vp, _vp, _sz, _sz, _int, _int, _int,
                          _int, _int, _int, _vp])
CTMAT_TILE = (2, 2)             # ctmat_tensor: outputs one thread owns (csrc/ctmat.hip kCtmatTM x kCtmatTN)
_sig("mfhe_ctmat_tensor", [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _sz, _sz, _sz, _int, _int, _int, _vp, _vp, _sz, _sz,
                           _sz, _vp, _sz, _sz, _sz, _sz, _int, _vp])
_sig("mfhe_ctmat_reserve", [_vp, _int, _int, _sz, _int, _int, _int, _int, _int, _int])
_sig("mfhe_ctmat_apply", [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _sz, _sz, _sz, _int, _int, _int, _vp, _vp, _vp, _sz,
                          _sz, _int, _int, _int, _int, _int, _int, _vp])
PTMUL_MAX_TERMS = 64            # ptmul_sum / ptmat_tensor / ptmat: most terms of one sum
_sig("mfhe_ptmat_tile", [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)])


def _ptmat_tile():
    tm, tn = ctypes.c_int(), ctypes.c_int()
    if lib.mfhe_ptmat_tile(ctypes.byref(tm), ctypes.byref(tn)) != OK:
        raise ImportError("mfhe_ptmat_tile failed")
    return tm.value, tn.value


PTMAT_TILE = _ptmat_tile()      # ptmat_tensor: outputs one thread owns in the loaded build (kPtmatTM x kPtmatTN)
_sig("mfhe_ptmul_sum", [_vp, _vp, _vp, _sz, _sz, _int, _vp, _sz, _sz, _int, ctypes.POINTER(_int), ctypes.POINTER(_int),
                        _int, _int, _vp, _vp, _sz, _sz, _int, _vp])
_sig("mfhe_ptmat_tensor", [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _sz, _sz, _sz, _int, _int, _int, _vp, _sz, _sz, _sz, _vp,
                           _vp, _sz, _sz, _sz, _sz, _int, _int, _vp])
_sig("mfhe_ptmat_reserve", [_vp, _int, _int, _sz, _int, _int])
_sig("mfhe_ptmat_apply", [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _sz, _sz, _sz, _int, _int, _int, _vp, _sz, _sz, _sz, _vp,
                          _vp, _sz, _sz, _int, _int, _vp])
_dbl = ctypes.c_double
LINCOMB_MAX_TERMS = 64          # ct_lincomb: most terms of one sum (a node of a PolyPlan among them)


class PolyInfo(ctypes.Structure):
    _fields_ = [("basis", _int), ("degree", _int), ("level", _int), ("nnodes", _int), ("nreg", _int),
                ("nconst", _int), ("nmul", _int), ("depth", _int), ("out_level", _int), ("out_reg", _int),
                ("in_scale", _dbl), ("out_scale", _dbl)]


class PolyNode(ctypes.Structure):
    _fields_ = [("dst", _int), ("level", _int), ("mul_a", _int), ("mul_b", _int), ("k_mul", _int), ("nterms", _int),
                ("addend_k", _int), ("term_src", _int * LINCOMB_MAX_TERMS), ("term_k", _int * LINCOMB_MAX_TERMS),
                ("term_coef", _dbl * LINCOMB_MAX_TERMS), ("addend_coef", _dbl), ("scale_in", _dbl), ("scale_out", _dbl)]


_sig("mfhe_ct_lincomb", [_vp, _vp, _vp, _sz, _sz, _int, _vp, _sz, _int, ctypes.POINTER(_int), ctypes.POINTER(_int), _int,
                         _int, _vp, _vp, _sz, _sz, _int, _vp])
_sig("mfhe_poly_plan_create", [_vp, ctypes.POINTER(_dbl), _int, _int, _dbl, _int, ctypes.POINTER(_vp)])
_sig("mfhe_poly_plan_destroy", [_vp])
_sig("mfhe_poly_plan_info", [_vp, ctypes.POINTER(PolyInfo)])
_sig("mfhe_poly_plan_node", [_vp, _int, ctypes.POINTER(PolyNode)])
_sig("mfhe_poly_plan_constant", [_vp, _int, ctypes.POINTER(_int), _u64p, _u64p])
_sig("mfhe_poly_plan_table", [_vp, ctypes.POINTER(_vp)])
_sig("mfhe_poly_reserve", [_vp, _vp, _sz, _int, _int, _int, _int])
_sig("mfhe_poly_apply", [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _vp])
_sig("mfhe_slot_reserve", [_vp, _sz, _int, _int, _int])
_sig("mfhe_slot_encode", [_vp, _vp, _sz, _dbl, _vp, _sz, _sz, _int, _int, _int, _int, _vp])
_sig("mfhe_slot_decode", [_vp, _vp, _sz, _dbl, _vp, _sz, _sz, _int, _int, _vp])
_seedp = ctypes.POINTER(ctypes.c_uint32)
_u64 = ctypes.c_uint64
_sig("mfhe_rlwe_reserve", [_vp, _sz, _int, _int, _int])
_sig("mfhe_rlwe_sample_uniform", [_vp, _seedp, _u64, _vp, _sz, _sz, _int, _int, _int, _vp])
_sig("mfhe_rlwe_sample_small", [_vp, _seedp, _int, _u64, _vp, _sz, _sz, _int, _int, _int, _int, _vp])
_sig("mfhe_rlwe_lift_small", [_vp, _vp, _sz, _vp, _sz, _sz, _int, _int, _int, _int, _vp])
_sig("mfhe_rlwe_encrypt_sk", [_vp, _seedp, _u64, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _int, _int, _int, _vp])
_sig("mfhe_rlwe_ksk_gen", [_vp, _seedp, _u64, _int, _int, _vp, _vp, _vp, _int, _int, _int, _int, _vp])
_sig("mfhe_rlwe_encrypt_pk", [_vp, _seedp, _u64, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _int, _vp])
_sig("mfhe_rlwe_decrypt", [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _int, _vp])
for _n in ("mfhe_wcrt_fwd", "mfhe_wcrt_inv", "mfhe_wcrt_fwd_vector", "mfhe_wcrt_fwd_centered",
           "mfhe_wcrt_inv_centered", "mfhe_wdft_fwd", "mfhe_wdft_inv", "mfhe_matrix_to_poly", "mfhe_poly_to_matrix",
           "mfhe_keygen"):
    _sig(_n, [_vp, _vp, _vp, _vp] if _n != "mfhe_keygen" else [_vp, _vp, _vp])
_sig("mfhe_xy_idft", [_vp, _vp, _vp, _sz, _vp])
_sig("mfhe_xy_dft", [_vp, _vp, _vp, _sz, _vp])
_sig("mfhe_wdft_fwd_pair_i64", [_vp] * 6)
_sig("mfhe_wdft_inv_pair", [_vp] * 6)
_sig("mfhe_ct_add", [_vp] * 5)
_sig("mfhe_ct_mul_tensor", [_vp] * 7)
_sig("mfhe_trace_map_bprime", [_vp] * 5 + [ctypes.c_int, ctypes.c_int, _sz, _vp])
_sig("mfhe_trace_gemm", [_vp] * 7 + [ctypes.c_int, ctypes.c_int, _sz, _vp])
_sig("mfhe_trace_rescale", [_vp] * 3 + [ctypes.c_int, ctypes.c_int, _sz, _u64p, _vp])
_sig("mfhe_trace_product", [_vp] * 7 + [ctypes.c_int, ctypes.c_int, _sz, _u64p, _vp])
_sig("mfhe_ctx_reserve_workspace", [_vp])
_sig("mfhe_encode", [_vp, _vp, _vp, _vp, _vp])
_sig("mfhe_decode", [_vp, _vp, _vp, _vp, _vp])
_sig("mfhe_encrypt", [_vp, _vp, _vp, _vp, _vp])
_sig("mfhe_encrypt_pair", [_vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("mfhe_decrypt_to_eval", [_vp, _vp, _vp, _vp, _vp])
_sig("mfhe_decrypt_and_decode", [_vp, _vp, _vp, _vp, _vp, _vp])
_sig("mfhe_comm_unique_id", [_vp])
_sig("mfhe_comm_init", [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)])
_sig("mfhe_comm_wrap", [_vp, ctypes.POINTER(_vp)])
_sig("mfhe_comm_destroy", [_vp])
_sig("mfhe_comm_info", [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)])
_sig("mfhe_allgather_limbs", [_vp, _vp, _sz, _vp, _vp])
_sig("mfhe_crt_recombine_sharded", [_vp, _vp, ctypes.c_int, _vp, _sz, _sz, _vp, _sz, _vp])
_sig("mfhe_crt_recombine_reserve", [_vp, _vp, ctypes.c_int, _sz, _sz])
_sig("mfhe_crt_recombine_chunked", [_vp, _vp, ctypes.c_int, _vp, _sz, _sz, _sz, _vp, _sz, ctypes.c_int, _vp])
_sig("mfhe_crt_recombine_chunked_reserve", [_vp, _vp, ctypes.c_int, _sz, _sz])
_sig("mfhe_ctx_set_limb_shard", [_vp, ctypes.c_int, ctypes.c_int])
_sig("mfhe_decode_sharded", [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp])
_sig("mfhe_decrypt_and_decode_sharded", [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("mfhe_last_error", [], ctypes.c_char_p)
_sig("mfhe_version", [], ctypes.c_char_p)


def declared_symbols(header: Path = None) -> list[str]:
    """Every function name declared in include/*.h (the C-ABI surface)."""
    hdrs = [header] if header else sorted((REPO_ROOT / "include").glob("*.h"))
    names = []
    for h in hdrs:
        text = re.sub(r"/\*.*?\*/", "", h.read_text(), flags=re.S)
        names += re.findall(r"\b(mfhe_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        raise MfheError(rc, f"{what}: {lib.mfhe_last_error().decode()}")


_XCHG = {"allgather": XCHG_ALLGATHER, "alltoall": XCHG_ALLTOALL}


def _need(t, words, what):
    """Host-side size check before a raw pointer crosses the C ABI (an undersized tensor would otherwise be
    an out-of-bounds device access)."""
    if t.numel() * t.element_size() < 8 * words:
        raise ValueError(f"{what}: {t.numel()} elements of {t.element_size()} B < {words} words needed")


def _need_strided(t, count, stride, what):
    """An output written at t[i * stride], i < count: (count - 1) * stride + 1 words."""
    if stride < 1:
        raise ValueError(f"{what}: stride must be >= 1")
    _need(t, (count - 1) * stride + 1 if count else 0, what)


class _stdout_to_stderr:
    """RCCL's initialisation banner goes to fd 1; keep a caller's stdout (bench.py's one JSON line) clean."""

    def __enter__(self):
        import sys
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        os.dup2(self._saved, 1)
        os.close(self._saved)


class Comm:
    """An RCCL communicator owned by libmfhe (include/mfhe.h mfhe_comm_*): one per process/GPU.

    `Comm.create(rank, world, group)` makes rank 0 draw the unique id and broadcasts it over an existing
    torch.distributed process group (any backend) -- the side channel only; the data path is RCCL."""

    def __init__(self, handle, size, rank):
        self._h, self.size, self.rank = handle, size, rank

    @classmethod
    def from_id(cls, uid: bytes, world: int, rank: int) -> "Comm":
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        h = _vp()
        with _stdout_to_stderr():
            rc = lib.mfhe_comm_init(ctypes.addressof(buf), world, rank, ctypes.byref(h))
        check(rc, "comm_init")
        return cls(h, world, rank)

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
        with _stdout_to_stderr():
            rc = lib.mfhe_comm_unique_id(ctypes.addressof(buf))
        check(rc, "comm_unique_id")
        return bytes(buf)

    @classmethod
    def create(cls, group=None) -> "Comm":
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        uid = cls.unique_id() if rank == 0 else bytes(COMM_ID_BYTES)
        t = torch.tensor(list(uid), dtype=torch.uint8)
        if dist.get_backend(group) == "nccl":
            t = t.cuda()
        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return cls.from_id(bytes(t.cpu().tolist()), world, rank)

    def allgather_limbs(self, shard, recv, stream=None):
        _need(recv, shard.numel() * self.size, "recv")
        check(lib.mfhe_allgather_limbs(self._h, _ptr(shard), shard.numel(), _ptr(recv), _stream_ptr(stream)),
              "allgather_limbs")
        return recv

    def close(self):
        if self._h:
            check(lib.mfhe_comm_destroy(self._h), "comm_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream_ptr(stream) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _ptr(t) -> int:
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("mfhe operates on device tensors")
    if not t.is_contiguous():
        raise ValueError("mfhe needs contiguous tensors")
    return t.data_ptr()


class Seed:
    """The 256-bit seed of the rlwe_* draws (32 bytes, from os.urandom by default) with a counter of polynomial ids:
    take(n) returns the first of n ids never handed out before, so calls that share a Seed never reuse a
    (seed, stream, id).  The library itself obtains no entropy and keeps no state."""

    def __init__(self, key: bytes = None, next_id: int = 0):
        key = os.urandom(32) if key is None else bytes(key)
        if len(key) != 32:
            raise ValueError("a Seed is 32 bytes")
        self.key, self.next_id = key, int(next_id)
        self.words = (ctypes.c_uint32 * 8)(*[int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)])

    def take(self, n: int = 1) -> int:
        if n < 0 or self.next_id + n > 1 << 64:
            raise ValueError("Seed: the 64-bit id space is exhausted")
        first, self.next_id = self.next_id, self.next_id + n
        return first


def _seed_words(seed):
    if isinstance(seed, Seed):
        return seed.words
    if seed is None:
        return None
    return Seed(seed).words


class Context:
    """One parameter set + device tables (mfhe_ctx).  Mirrors init_he_backend /
    PhantomContext / Encoder table setup of the reference."""

    def __init__(self, moduli, log_n: int, conventions: int = CONV_PHANTOM, delta: float = SCALING_FACTOR):
        arr = (ctypes.c_uint64 * len(moduli))(*[int(m) for m in moduli])
        h = _vp()
        check(lib.mfhe_ctx_create(arr, len(moduli), int(log_n), int(conventions), float(delta), ctypes.byref(h)),
              "mfhe_ctx_create")
        self._h = h
        self.moduli = [int(m) for m in moduli]
        self.L = len(self.moduli)
        self.log_n = int(log_n)
        self.N = 1 << self.log_n
        self.delta = float(delta)
        info = self.info()
        self.crt_words = info.crt_words
        self.phi = info.phi

    @property
    def handle(self):
        return self._h

    def info(self) -> CtxInfo:
        inf = CtxInfo()
        check(lib.mfhe_ctx_get_info(self._h, ctypes.byref(inf)), "get_info")
        return inf

    def set_arith(self, arith: int) -> None:
        check(lib.mfhe_ctx_set_arith(self._h, arith), "set_arith")

    def set_option(self, opt: int, value: int) -> None:
        check(lib.mfhe_ctx_set_option(self._h, opt, int(value)), "set_option")

    def get_option(self, opt: int) -> int:
        v = ctypes.c_int64()
        check(lib.mfhe_ctx_get_option(self._h, opt, ctypes.byref(v)), "get_option")
        return v.value

    def close(self):
        if getattr(self, "_h", None):
            lib.mfhe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- NTT ----
    def _ntt(self, fn, data, batch, start_limb, nlimbs, stream):
        nl = self.L - start_limb if nlimbs is None else nlimbs
        if batch is None:
            batch = data.numel() // (nl * self.N)
        if data.numel() < batch * nl * self.N:
            raise ValueError("tensor smaller than batch * nlimbs * N")
        check(fn(self._h, _ptr(data), batch, start_limb, nl, _stream_ptr(stream)), fn.__name__)
        return data

    def ntt_fwd(self, data, batch=None, start_limb=0, nlimbs=None, stream=None):
        return self._ntt(lib.mfhe_ntt_fwd, data, batch, start_limb, nlimbs, stream)

    def ntt_inv(self, data, batch=None, start_limb=0, nlimbs=None, stream=None):
        return self._ntt(lib.mfhe_ntt_inv, data, batch, start_limb, nlimbs, stream)

    def gl_ntt_fwd(self, data, batch=None, start_limb=0, nlimbs=None, stream=None):
        return self._ntt(lib.mfhe_gl_ntt_fwd, data, batch, start_limb, nlimbs, stream)

    def gl_ntt_inv(self, data, batch=None, start_limb=0, nlimbs=None, stream=None):
        return self._ntt(lib.mfhe_gl_ntt_inv, data, batch, start_limb, nlimbs, stream)

    def cyclic_ntt_fwd(self, data, batch=None, start_limb=0, nlimbs=None, stream=None):
        return self._ntt(lib.mfhe_cyclic_ntt_fwd, data, batch, start_limb, nlimbs, stream)

    def cyclic_ntt_inv(self, data, batch=None, start_limb=0, nlimbs=None, stream=None):
        return self._ntt(lib.mfhe_cyclic_ntt_inv, data, batch, start_limb, nlimbs, stream)

    def gl_perm(self, src, dst, batch, nlimbs=None, inverse=False, stream=None):
        nl = self.L if nlimbs is None else nlimbs
        check(lib.mfhe_gl_perm(self._h, _ptr(src), _ptr(dst), batch, nl, int(inverse), _stream_ptr(stream)), "gl_perm")
        return dst

    def ntt_tables(self):
        ps = [_vp() for _ in range(6)]
        check(lib.mfhe_ntt_tables(self._h, *[ctypes.byref(p) for p in ps]), "ntt_tables")
        dm = _vp()
        check(lib.mfhe_ntt_dmodulus(self._h, ctypes.byref(dm)), "ntt_dmodulus")
        return [p.value for p in ps] + [dm.value]

    # ---- wide CRT ----
    def rns_decompose(self, src, dst, npoly, ncoeff, in_stride=1, stream=None):
        check(lib.mfhe_rns_decompose(self._h, _ptr(src), in_stride, npoly, ncoeff, _ptr(dst), _stream_ptr(stream)),
              "rns_decompose")
        return dst

    def crt_compose(self, src, mag, neg, npoly, ncoeff, stream=None):
        check(lib.mfhe_crt_compose(self._h, _ptr(src), npoly, ncoeff, _ptr(mag), _ptr(neg), _stream_ptr(stream)),
              "crt_compose")

    def crt_compose_i64(self, src, out, npoly, ncoeff, stream=None):
        """Centred CRT value truncated to int64 (crt_compose_centerlift_kernel, encoder.cu:152-189)."""
        _need(src, npoly * self.L * ncoeff, "crt_compose_i64 src")
        _need(out, npoly * ncoeff, "crt_compose_i64 out")
        check(lib.mfhe_crt_compose_i64(self._h, _ptr(src), npoly, ncoeff, _ptr(out), _stream_ptr(stream)),
              "crt_compose_i64")
        return out

    def crt_to_f64(self, mag, neg, out, count, out_stride=1, stream=None):
        _need(mag, count * self.info().crt_words, "crt_to_f64 mag")
        _need_strided(out, count, out_stride, "crt_to_f64 out")
        check(lib.mfhe_crt_to_f64(self._h, _ptr(mag), _ptr(neg), count, _ptr(out), out_stride, _stream_ptr(stream)),
              "crt_to_f64")
        return out

    def crt_compose_f64(self, src, out, npoly, ncoeff, out_stride=1, stream=None):
        _need(src, npoly * self.L * ncoeff, "crt_compose_f64 src")
        _need_strided(out, npoly * ncoeff, out_stride, "crt_compose_f64 out")
        check(lib.mfhe_crt_compose_f64(self._h, _ptr(src), npoly, ncoeff, _ptr(out), out_stride, _stream_ptr(stream)),
              "crt_compose_f64")
        return out


    def crt_compose_f64_sharded(self, src, out, nshards, shard_stride, npoly, ncoeff, out_stride=1, stream=None,
                                src_offset=0):
        """Compose residue shards gathered from `nshards` GPUs in place (see include/mfhe.h)."""
        _need(src, src_offset + (nshards - 1) * shard_stride + npoly * (self.L // max(nshards, 1)) * ncoeff,
              "crt_compose_f64_sharded src")
        _need_strided(out, npoly * ncoeff, out_stride, "crt_compose_f64_sharded out")
        check(lib.mfhe_crt_compose_f64_sharded(self._h, _ptr(src) + 8 * src_offset, nshards, shard_stride, npoly,
                                               ncoeff, _ptr(out), out_stride, _stream_ptr(stream)),
              "crt_compose_f64_sharded")
        return out

    # ---- RNS basis conversion (include/mfhe.h): residues [npoly][rows][ncoeff], poly strides in words ----
    @staticmethod
    def _need_polys(t, npoly, stride, rows, ncoeff, what):
        """npoly blocks of rows * ncoeff words, `stride` words apart."""
        _need(t, (npoly - 1) * stride + rows * ncoeff if npoly and ncoeff else 0, what)

    def rns_bconv_reserve(self, src_start, src_count, dst_start, dst_count):
        check(lib.mfhe_rns_bconv_reserve(self._h, src_start, src_count, dst_start, dst_count), "rns_bconv_reserve")

    def rns_bconv(self, src, dst, npoly, ncoeff, src_start, src_count, dst_start, dst_count, mode=BCONV_FAST,
                  in_stride=None, out_stride=None, stream=None):
        """dst rows = limbs [dst_start, +dst_count) converted from src rows = limbs [src_start, +src_count)."""
        ist = src_count * ncoeff if in_stride is None else in_stride
        ost = dst_count * ncoeff if out_stride is None else out_stride
        self._need_polys(src, npoly, ist, src_count, ncoeff, "rns_bconv src")
        self._need_polys(dst, npoly, ost, dst_count, ncoeff, "rns_bconv dst")
        check(lib.mfhe_rns_bconv(self._h, _ptr(src), ist, _ptr(dst), ost, npoly, ncoeff, src_start, src_count,
                                 dst_start, dst_count, mode, _stream_ptr(stream)), "rns_bconv")
        return dst

    def rns_moddown_reserve(self, keep_count, drop_start, drop_count):
        self.rns_bconv_reserve(drop_start, drop_count, 0, keep_count)

    def rns_moddown(self, src, dst, npoly, ncoeff, keep_count, drop_start, drop_count, in_stride=None,
                    out_stride=None, stream=None):
        """src rows: limbs [0, keep_count) then [drop_start, +drop_count); dst rows [0, keep_count) =
        round(x / prod(dropped)).  dst may be src (in place, equal strides)."""
        ist = (keep_count + drop_count) * ncoeff if in_stride is None else in_stride
        ost = (ist if dst is src else keep_count * ncoeff) if out_stride is None else out_stride
        self._need_polys(src, npoly, ist, keep_count + drop_count, ncoeff, "rns_moddown src")
        self._need_polys(dst, npoly, ost, keep_count, ncoeff, "rns_moddown dst")
        check(lib.mfhe_rns_moddown(self._h, _ptr(src), ist, _ptr(dst), ost, npoly, ncoeff, keep_count, drop_start,
                                   drop_count, _stream_ptr(stream)), "rns_moddown")
        return dst

    def rns_rescale(self, src, dst, npoly, ncoeff, level, in_stride=None, out_stride=None, stream=None):
        """Drop limb level - 1 of a level-limb polynomial: dst rows [0, level - 1) = round(x / q_(level-1))."""
        return self.rns_moddown(src, dst, npoly, ncoeff, level - 1, level - 1, 1, in_stride, out_stride, stream)

    def _modup_ranges(self, level, digit_start, digit_count, special_start, nspecial):
        rs = [(0, digit_start), (digit_start + digit_count, level - digit_start - digit_count),
              (special_start, nspecial)]
        return [(a, n) for a, n in rs if n > 0]

    def rns_modup_reserve(self, level, digit_start, digit_count, special_start, nspecial):
        for a, n in self._modup_ranges(level, digit_start, digit_count, special_start, nspecial):
            self.rns_bconv_reserve(digit_start, digit_count, a, n)

    def rns_modup(self, src, dst, npoly, ncoeff, level, digit_start, digit_count, special_start, nspecial,
                  in_stride=None, out_stride=None, stream=None):
        """src rows: limbs [0, level); dst rows: [0, level) then [special_start, +nspecial): the digit's rows
        copied, every other row its FAST conversion.  One launch."""
        ist = level * ncoeff if in_stride is None else in_stride
        ost = (level + nspecial) * ncoeff if out_stride is None else out_stride
        self._need_polys(src, npoly, ist, level, ncoeff, "rns_modup src")
        self._need_polys(dst, npoly, ost, level + nspecial, ncoeff, "rns_modup dst")
        check(lib.mfhe_rns_modup(self._h, _ptr(src), ist, _ptr(dst), ost, npoly, ncoeff, level, digit_start,
                                 digit_count, special_start, nspecial, _stream_ptr(stream)), "rns_modup")
        return dst

    def ntt_bconv_reserve(self, npoly, rows):
        check(lib.mfhe_ntt_bconv_reserve(self._h, npoly, rows), "ntt_bconv_reserve")

    def ntt_modup(self, src, dst, npoly, level, digit_start, digit_count, special_start, nspecial, in_stride=None,
                  out_stride=None, stream=None):
        """rns_modup on evaluation-domain rows (phantom NTT, ncoeff = N)."""
        ist = level * self.N if in_stride is None else in_stride
        ost = (level + nspecial) * self.N if out_stride is None else out_stride
        self._need_polys(src, npoly, ist, level, self.N, "ntt_modup src")
        self._need_polys(dst, npoly, ost, level + nspecial, self.N, "ntt_modup dst")
        check(lib.mfhe_ntt_modup(self._h, _ptr(src), ist, _ptr(dst), ost, npoly, level, digit_start, digit_count,
                                 special_start, nspecial, _stream_ptr(stream)), "ntt_modup")
        return dst

    def ntt_moddown(self, src, dst, npoly, keep_count, drop_start, drop_count, in_stride=None, out_stride=None,
                    stream=None):
        """rns_moddown on evaluation-domain rows (phantom NTT, ncoeff = N)."""
        ist = (keep_count + drop_count) * self.N if in_stride is None else in_stride
        ost = (ist if dst is src else keep_count * self.N) if out_stride is None else out_stride
        self._need_polys(src, npoly, ist, keep_count + drop_count, self.N, "ntt_moddown src")
        self._need_polys(dst, npoly, ost, keep_count, self.N, "ntt_moddown dst")
        check(lib.mfhe_ntt_moddown(self._h, _ptr(src), ist, _ptr(dst), ost, npoly, keep_count, drop_start,
                                   drop_count, _stream_ptr(stream)), "ntt_moddown")
        return dst

    # ---- hybrid key switching (include/mfhe.h): evaluation domain, Q limbs [0, level), K special limbs from
    # special_start (>= key_level); a (level + K)-row block has limb r on row r < level, else special_start + r - level
    def ksk_assemble(self, s_from, s_to, a, e, ksk, key_level, alpha, special_start, nspecial, stream=None):
        """ksk [beta][2][key_level + K][N] from s_from, s_to [key_level + K][N] and a, e [beta][key_level + K][N]:
        component 1 = a_j, component 0 = e_j - a_j s_to + F s_from (F = P mod q_r on the rows of digit j, else 0)."""
        rows, beta = key_level + nspecial, -(-key_level // max(alpha, 1))
        for t, what in ((s_from, "s_from"), (s_to, "s_to")):
            self._need_polys(t, 1, rows * self.N, rows, self.N, f"ksk_assemble {what}")
        for t, what in ((a, "a"), (e, "e")):
            self._need_polys(t, beta, rows * self.N, rows, self.N, f"ksk_assemble {what}")
        self._need_polys(ksk, beta, 2 * rows * self.N, 2 * rows, self.N, "ksk_assemble ksk")
        check(lib.mfhe_ksk_assemble(self._h, _ptr(s_from), _ptr(s_to), _ptr(a), _ptr(e), _ptr(ksk), key_level, alpha,
                                    special_start, nspecial, _stream_ptr(stream)), "ksk_assemble")
        return ksk

    def ksk_inner_product(self, raised, ksk, acc, npoly, ndigits, level, key_level, special_start, nspecial,
                          digit_stride=None, poly_stride=None, acc_stride=None, stream=None):
        """acc [npoly][2][level + K][N] = sum over the digits of raised [ndigits][npoly][level + K][N] times
        ksk [ndigits][2][key_level + K][N] (key rows [0, level) and the special rows).  One launch."""
        rows = level + nspecial
        pst = rows * self.N if poly_stride is None else poly_stride
        dst = npoly * pst if digit_stride is None else digit_stride
        ast = 2 * rows * self.N if acc_stride is None else acc_stride
        self._need_polys(raised, npoly, pst, rows, self.N, "ksk_inner_product raised (one digit)")
        _need(raised, (ndigits - 1) * dst + (npoly - 1) * pst + rows * self.N if npoly and ndigits > 0 else 0,
              "ksk_inner_product raised")
        self._need_polys(ksk, ndigits, 2 * (key_level + nspecial) * self.N, 2 * (key_level + nspecial), self.N,
                         "ksk_inner_product ksk")
        self._need_polys(acc, npoly, ast, 2 * rows, self.N, "ksk_inner_product acc")
        check(lib.mfhe_ksk_inner_product(self._h, _ptr(raised), dst, pst, _ptr(ksk), _ptr(acc), ast, npoly, ndigits,
                                         level, key_level, special_start, nspecial, _stream_ptr(stream)),
              "ksk_inner_product")
        return acc

    def keyswitch_reserve(self, npoly, level, key_level, alpha, special_start, nspecial):
        """Grow the workspace and build every table of this geometry: keyswitch then allocates nothing."""
        check(lib.mfhe_keyswitch_reserve(self._h, npoly, level, key_level, alpha, special_start, nspecial),
              "keyswitch_reserve")

    def keyswitch(self, src, ksk, out0, out1, npoly, level, key_level, alpha, special_start, nspecial, flags=0,
                  in_stride=None, out_stride=None, stream=None):
        """src [npoly][level][N] -> out0, out1 [npoly][level][N] with out0 + out1 s_to ~ src s_from for the key's
        (s_from, s_to): ModUp of every digit, inner product, ModDown.  flags: KS_ADD adds to out0 / out1."""
        ist = level * self.N if in_stride is None else in_stride
        ost = level * self.N if out_stride is None else out_stride
        beta = -(-key_level // max(alpha, 1))
        self._need_polys(src, npoly, ist, level, self.N, "keyswitch src")
        self._need_polys(out0, npoly, ost, level, self.N, "keyswitch out0")
        self._need_polys(out1, npoly, ost, level, self.N, "keyswitch out1")
        self._need_polys(ksk, beta, 2 * (key_level + nspecial) * self.N, 2 * (key_level + nspecial), self.N,
                         "keyswitch ksk")
        check(lib.mfhe_keyswitch(self._h, _ptr(src), ist, _ptr(ksk), _ptr(out0), _ptr(out1), ost, npoly, level,
                                 key_level, alpha, special_start, nspecial, flags, _stream_ptr(stream)), "keyswitch")
        return out0, out1

    def relinearize(self, d2, rlk, d0, d1, npoly, level, key_level, alpha, special_start, nspecial, in_stride=None,
                    out_stride=None, stream=None):
        """(d0, d1) += keyswitch(d2) with the relinearisation key rlk (s_from = s^2, s_to = s): a degree-2
        ciphertext (d0, d1, d2) becomes the degree-1 ciphertext (d0, d1) of the same message."""
        return self.keyswitch(d2, rlk, d0, d1, npoly, level, key_level, alpha, special_start, nspecial, KS_ADD,
                              in_stride, out_stride, stream)

    def gen_switch_key(self, s_from, s_to, key_level, alpha, special_start, nspecial, generator=None, sigma=3.2):
        """A switching key [beta][2][key_level + K][N] from s_from to s_to (both [key_level + K][N], evaluation
        domain).  The randomness lives in PyTorch: a uniform per limb, e a rounded Gaussian of width sigma clipped
        at 6 sigma, its residues taken on every row and forward-transformed; the arithmetic is mfhe_ksk_assemble."""
        import torch
        rows, beta, n = key_level + nspecial, -(-key_level // alpha), self.N
        dev = s_from.device
        limbs = list(range(key_level)) + list(range(special_start, special_start + nspecial))
        a = torch.empty((beta, rows, n), dtype=torch.int64, device=dev)
        for r, l in enumerate(limbs):
            a[:, r, :] = torch.randint(0, self.moduli[l], (beta, n), generator=generator, device=dev, dtype=torch.int64)
        g = torch.randn((beta, n), generator=generator, device=dev, dtype=torch.float64) * sigma
        ei = torch.round(g.clamp(-6.0 * sigma, 6.0 * sigma)).to(torch.int64)
        q = torch.tensor([self.moduli[l] for l in limbs], dtype=torch.int64, device=dev)
        e = torch.remainder(ei[:, None, :], q[None, :, None])          # [beta][rows][N], coefficient domain
        eq, ep = e[:, :key_level].contiguous(), e[:, key_level:].contiguous()
        self.ntt_fwd(eq, beta, 0, key_level)
        self.ntt_fwd(ep, beta, special_start, nspecial)
        e = torch.cat((eq, ep), dim=1).contiguous()
        ksk = torch.empty(beta * 2 * rows * n, dtype=torch.int64, device=dev)
        return self.ksk_assemble(s_from, s_to, a, e, ksk, key_level, alpha, special_start, nspecial)

    # ---- Galois automorphisms and hoisted rotations (include/mfhe.h): the geometry of the key switch; a Galois
    # element is an odd integer in [1, 2N) (galois_elt / galois_conj below)
    def automorphism(self, src, dst, npoly, rows, galois_elt, in_stride=None, out_stride=None, stream=None):
        """dst [npoly][rows][N] = sigma_g(src) in the evaluation domain: dst[p][r][i] = src[p][r][pi_g(i)].  Out of
        place, one launch."""
        ist = rows * self.N if in_stride is None else in_stride
        ost = rows * self.N if out_stride is None else out_stride
        self._need_polys(src, npoly, ist, rows, self.N, "automorphism src")
        self._need_polys(dst, npoly, ost, rows, self.N, "automorphism dst")
        check(lib.mfhe_ntt_automorphism(self._h, _ptr(src), ist, _ptr(dst), ost, npoly, rows, galois_elt,
                                        _stream_ptr(stream)), "automorphism")
        return dst

    def _need_raised(self, raised, npoly, ndigits, rows, dst, pst, what):
        self._need_polys(raised, npoly, pst, rows, self.N, f"{what} raised (one digit)")
        _need(raised, (ndigits - 1) * dst + (npoly - 1) * pst + rows * self.N if npoly and ndigits > 0 else 0,
              f"{what} raised")

    def ksk_inner_product_galois(self, raised, ksk, acc, npoly, ndigits, level, key_level, special_start, nspecial,
                                 galois_elt, digit_stride=None, poly_stride=None, acc_stride=None, stream=None):
        """ksk_inner_product with the raised digits read through the gather of sigma_g:
        acc[p][c][r][i] = sum_j raised[j][p][r][pi_g(i)] ksk[j][c][keyrow(r)][i].  One launch."""
        rows = level + nspecial
        pst = rows * self.N if poly_stride is None else poly_stride
        dst = npoly * pst if digit_stride is None else digit_stride
        ast = 2 * rows * self.N if acc_stride is None else acc_stride
        self._need_raised(raised, npoly, ndigits, rows, dst, pst, "ksk_inner_product_galois")
        self._need_polys(ksk, ndigits, 2 * (key_level + nspecial) * self.N, 2 * (key_level + nspecial), self.N,
                         "ksk_inner_product_galois ksk")
        self._need_polys(acc, npoly, ast, 2 * rows, self.N, "ksk_inner_product_galois acc")
        check(lib.mfhe_ksk_inner_product_galois(self._h, _ptr(raised), dst, pst, _ptr(ksk), _ptr(acc), ast, npoly,
                                                ndigits, level, key_level, special_start, nspecial, galois_elt,
                                                _stream_ptr(stream)), "ksk_inner_product_galois")
        return acc

    def galois_reserve(self, npoly, level, key_level, alpha, special_start, nspecial):
        """Grow the workspace and build every table of this geometry: keyswitch_raise, galois_apply_raised and
        galois_apply then allocate nothing."""
        check(lib.mfhe_galois_reserve(self._h, npoly, level, key_level, alpha, special_start, nspecial),
              "galois_reserve")

    def keyswitch_raise(self, src, raised, npoly, level, alpha, special_start, nspecial, in_stride=None,
                        digit_stride=None, poly_stride=None, stream=None):
        """The hoisted part of a rotation: raised [beta][npoly][level + K][N] = the ModUp of every digit of src
        [npoly][level][N], as keyswitch raises them.  No key, no Galois element."""
        rows, beta = level + nspecial, -(-level // max(alpha, 1))
        ist = level * self.N if in_stride is None else in_stride
        pst = rows * self.N if poly_stride is None else poly_stride
        dst = npoly * pst if digit_stride is None else digit_stride
        self._need_polys(src, npoly, ist, level, self.N, "keyswitch_raise src")
        self._need_raised(raised, npoly, beta, rows, dst, pst, "keyswitch_raise")
        check(lib.mfhe_keyswitch_raise(self._h, _ptr(src), ist, _ptr(raised), dst, pst, npoly, level, alpha,
                                       special_start, nspecial, _stream_ptr(stream)), "keyswitch_raise")
        return raised

    def galois_apply_raised(self, c0, raised, gk, out0, out1, npoly, level, key_level, alpha, special_start, nspecial,
                            galois_elt, in_stride=None, digit_stride=None, poly_stride=None, out_stride=None,
                            stream=None):
        """(out0, out1) = (sigma_g(c0) + k0, k1) from c0 [npoly][level][N], the raised digits of c1 (keyswitch_raise)
        and the Galois key gk of g: out0 + out1 s ~ sigma_g(c0 + c1 s).  raised is only read."""
        rows, beta = level + nspecial, -(-level // max(alpha, 1))
        ist = level * self.N if in_stride is None else in_stride
        ost = level * self.N if out_stride is None else out_stride
        pst = rows * self.N if poly_stride is None else poly_stride
        dst = npoly * pst if digit_stride is None else digit_stride
        self._need_polys(c0, npoly, ist, level, self.N, "galois_apply_raised c0")
        self._need_raised(raised, npoly, beta, rows, dst, pst, "galois_apply_raised")
        self._need_polys(out0, npoly, ost, level, self.N, "galois_apply_raised out0")
        self._need_polys(out1, npoly, ost, level, self.N, "galois_apply_raised out1")
        self._need_polys(gk, -(-key_level // max(alpha, 1)), 2 * (key_level + nspecial) * self.N,
                         2 * (key_level + nspecial), self.N, "galois_apply_raised gk")
        check(lib.mfhe_galois_apply_raised(self._h, _ptr(c0), ist, _ptr(raised), dst, pst, _ptr(gk), _ptr(out0),
                                           _ptr(out1), ost, npoly, level, key_level, alpha, special_start, nspecial,
                                           galois_elt, _stream_ptr(stream)), "galois_apply_raised")
        return out0, out1

    def galois_apply(self, c0, c1, gk, out0, out1, npoly, level, key_level, alpha, special_start, nspecial, galois_elt,
                     in_stride=None, out_stride=None, stream=None):
        """One rotation or conjugation of the ciphertext (c0, c1), each [npoly][level][N], with the Galois key gk of
        g: keyswitch_raise(c1) into the workspace, then galois_apply_raised."""
        ist = level * self.N if in_stride is None else in_stride
        ost = level * self.N if out_stride is None else out_stride
        beta = -(-key_level // max(alpha, 1))
        for t, what in ((c0, "c0"), (c1, "c1")):
            self._need_polys(t, npoly, ist, level, self.N, f"galois_apply {what}")
        for t, what in ((out0, "out0"), (out1, "out1")):
            self._need_polys(t, npoly, ost, level, self.N, f"galois_apply {what}")
        self._need_polys(gk, beta, 2 * (key_level + nspecial) * self.N, 2 * (key_level + nspecial), self.N,
                         "galois_apply gk")
        check(lib.mfhe_galois_apply(self._h, _ptr(c0), _ptr(c1), ist, _ptr(gk), _ptr(out0), _ptr(out1), ost, npoly,
                                    level, key_level, alpha, special_start, nspecial, galois_elt,
                                    _stream_ptr(stream)), "galois_apply")
        return out0, out1

    def gen_galois_key(self, s, galois_elt, key_level, alpha, special_start, nspecial, generator=None, sigma=3.2):
        """The Galois key of g for the secret s [key_level + K][N] (evaluation domain): a switching key from
        sigma_g(s) to s (gen_switch_key)."""
        import torch
        rows = key_level + nspecial
        s_from = torch.empty(rows * self.N, dtype=torch.int64, device=s.device)
        self.automorphism(s, s_from, 1, rows, galois_elt)
        return self.gen_switch_key(s_from, s, key_level, alpha, special_start, nspecial, generator, sigma)

    # ---- encrypted linear transforms by baby-step giant-step (include/mfhe.h): the geometry of the key switch;
    # bsgs_plan below splits rotation indices into the steps and terms these calls take
    def lt_baby_step(self, c0, raised, gk, u, npoly, level, key_level, alpha, special_start, nspecial, galois_elt=1,
                     in_stride=None, digit_stride=None, poly_stride=None, u_stride=None, stream=None):
        """u [npoly][2][level + K][N] = the rotation of (c0, c1) by the Galois key gk of g, left in Q u P and scaled
        by P (no ModDown): c0 [npoly][level][N], raised the raised digits of c1 (keyswitch_raise).  gk None with
        galois_elt 1 is the unrotated term: `raised` is then c1 itself, laid out as c0."""
        rows, beta = level + nspecial, -(-level // max(alpha, 1))
        ist = level * self.N if in_stride is None else in_stride
        pst = rows * self.N if poly_stride is None else poly_stride
        dst = npoly * pst if digit_stride is None else digit_stride
        ust = 2 * rows * self.N if u_stride is None else u_stride
        self._need_polys(c0, npoly, ist, level, self.N, "lt_baby_step c0")
        if gk is None:
            self._need_polys(raised, npoly, ist, level, self.N, "lt_baby_step c1")
        else:
            self._need_raised(raised, npoly, beta, rows, dst, pst, "lt_baby_step")
            self._need_polys(gk, -(-key_level // max(alpha, 1)), 2 * (key_level + nspecial) * self.N,
                             2 * (key_level + nspecial), self.N, "lt_baby_step gk")
        self._need_polys(u, npoly, ust, 2 * rows, self.N, "lt_baby_step u")
        check(lib.mfhe_lt_baby_step(self._h, _ptr(c0), ist, _ptr(raised), dst, pst, _ptr(gk), _ptr(u), ust, npoly,
                                    level, key_level, alpha, special_start, nspecial, galois_elt,
                                    _stream_ptr(stream)), "lt_baby_step")
        return u

    def lt_pt_mac(self, u, pt, acc, term_u, term_pt, npoly, level, special_start, nspecial, nslots, npt,
                  pt_level=None, slot_stride=None, poly_stride=None, pt_stride=None, acc_stride=None, stream=None):
        """acc[p][c][r] = sum_t pt[term_pt[t]][ptrow(r)] u[term_u[t]][p][c][r] mod q_r: u [nslots][npoly][2][level + K][N],
        pt [npt][pt_level + K][N] shared by the batch, acc [npoly][2][level + K][N]; term_u, term_pt Python lists of
        1 .. 64 entries.  One launch."""
        rows = level + nspecial
        pt_level = level if pt_level is None else pt_level
        pst = 2 * rows * self.N if poly_stride is None else poly_stride
        sst = npoly * pst if slot_stride is None else slot_stride
        tst = (pt_level + nspecial) * self.N if pt_stride is None else pt_stride
        ast = 2 * rows * self.N if acc_stride is None else acc_stride
        if len(term_u) != len(term_pt):
            raise ValueError("lt_pt_mac: term_u and term_pt differ in length")
        self._need_polys(u, npoly, pst, 2 * rows, self.N, "lt_pt_mac u (one slot)")
        _need(u, (nslots - 1) * sst + (npoly - 1) * pst + 2 * rows * self.N if npoly and nslots > 0 else 0,
              "lt_pt_mac u")
        self._need_polys(pt, npt, tst, pt_level + nspecial, self.N, "lt_pt_mac pt")
        self._need_polys(acc, npoly, ast, 2 * rows, self.N, "lt_pt_mac acc")
        nt = len(term_u)
        tu, tp = (_int * max(nt, 1))(*term_u), (_int * max(nt, 1))(*term_pt)
        check(lib.mfhe_lt_pt_mac(self._h, _ptr(u), sst, pst, nslots, _ptr(pt), tst, npt, pt_level, _ptr(acc), ast, tu,
                                 tp, nt, npoly, level, special_start, nspecial, _stream_ptr(stream)), "lt_pt_mac")
        return acc

    def lt_reserve(self, npoly, level, key_level, alpha, special_start, nspecial, n_baby):
        """Grow the workspace and build every table of this geometry: lt_apply with up to n_baby baby steps then
        allocates nothing and copies nothing to the device."""
        check(lib.mfhe_lt_reserve(self._h, npoly, level, key_level, alpha, special_start, nspecial, n_baby),
              "lt_reserve")

    def lt_apply(self, c0, c1, pt, out0, out1, npoly, level, key_level, alpha, special_start, nspecial, baby_elt,
                 giant_elt, gk_baby, gk_giant, term_giant, term_baby, pt_level=None, in_stride=None, pt_stride=None,
                 out_stride=None, stream=None):
        """(out0, out1) = the linear transform of the ciphertext (c0, c1), each [npoly][level][N], by the plaintexts pt
        [nterms][pt_level + K][N]: term t multiplies plaintext t by baby step term_baby[t] inside giant step
        term_giant[t] (non-decreasing).  baby_elt, giant_elt: Galois elements, entry 0 is 1; gk_baby, gk_giant: lists
        of Galois keys (device tensors, entry 0 and unused steps may be None).  bsgs_plan gives the lists."""
        pt_level = level if pt_level is None else pt_level
        ist = level * self.N if in_stride is None else in_stride
        ost = level * self.N if out_stride is None else out_stride
        tst = (pt_level + nspecial) * self.N if pt_stride is None else pt_stride
        nb, ng, nt = len(baby_elt), len(giant_elt), len(term_giant)
        if len(gk_baby) != nb or len(gk_giant) != ng or len(term_baby) != nt:
            raise ValueError("lt_apply: list lengths differ")
        for t, what in ((c0, "c0"), (c1, "c1")):
            self._need_polys(t, npoly, ist, level, self.N, f"lt_apply {what}")
        for t, what in ((out0, "out0"), (out1, "out1")):
            self._need_polys(t, npoly, ost, level, self.N, f"lt_apply {what}")
        self._need_polys(pt, nt, tst, pt_level + nspecial, self.N, "lt_apply pt")
        kbeta, kw = -(-key_level // max(alpha, 1)), 2 * (key_level + nspecial) * self.N
        for k in list(gk_baby) + list(gk_giant):
            if k is not None:
                self._need_polys(k, kbeta, kw, 2 * (key_level + nspecial), self.N, "lt_apply key")
        # the ctypes arrays stay referenced by these locals across the call
        a_be, a_ge = (_int * max(nb, 1))(*baby_elt), (_int * max(ng, 1))(*giant_elt)
        a_kb = (_vp * max(nb, 1))(*[_ptr(k) for k in gk_baby])
        a_kg = (_vp * max(ng, 1))(*[_ptr(k) for k in gk_giant])
        a_tg, a_tb = (_int * max(nt, 1))(*term_giant), (_int * max(nt, 1))(*term_baby)
        plan = LtPlan(nb, ng, nt, a_be, a_ge, a_kb, a_kg, a_tg, a_tb)
        check(lib.mfhe_lt_apply(self._h, ctypes.byref(plan), _ptr(c0), _ptr(c1), ist, _ptr(pt), tst, pt_level,
                                _ptr(out0), _ptr(out1), ost, npoly, level, key_level, alpha, special_start, nspecial,
                                _stream_ptr(stream)), "lt_apply")
        return out0, out1

    # ---- ciphertext products (include/mfhe.h): the geometry of the key switch; a ciphertext is a pair of
    # [level][N] polynomials, a product a sum over nterms pairs of ciphertexts relinearised once
    def _ctmul_operands(self, a0, a1, b0, b1, nterms, npoly, level, a_term_stride, a_poly_stride, b_term_stride,
                        b_poly_stride, what):
        """Dense strides by default, the operand buffers size-checked: (a_term, a_poly, b_term, b_poly)."""
        if (b0 is None) != (b1 is None):
            raise ValueError(f"{what}: b0 and b1 are both given or both None (the square form)")
        lw = level * self.N
        apst = lw if a_poly_stride is None else a_poly_stride
        atst = npoly * apst if a_term_stride is None else a_term_stride
        bpst = lw if b_poly_stride is None else b_poly_stride
        btst = npoly * bpst if b_term_stride is None else b_term_stride
        ops = [(a0, "a0", atst, apst), (a1, "a1", atst, apst)]
        if b0 is not None:
            ops += [(b0, "b0", btst, bpst), (b1, "b1", btst, bpst)]
        for t, name, tst, pst in ops:
            self._need_polys(t, npoly, pst, level, self.N, f"{what} {name} (one term)")
            _need(t, (nterms - 1) * tst + (npoly - 1) * pst + lw if npoly and nterms > 0 else 0, f"{what} {name}")
        return atst, apst, btst, bpst

    def ctmul_tensor(self, a0, a1, b0, b1, d0, d1, d2, npoly, level, nterms=1, a_term_stride=None,
                     a_poly_stride=None, b_term_stride=None, b_poly_stride=None, d01_stride=None, d2_stride=None,
                     stream=None):
        """(d0, d1, d2), each [npoly][level][N] = sum_t (a0 b0, a0 b1 + a1 b0, a1 b1)[t] mod q_r for the ciphertexts
        (a0, a1) and (b0, b1), each pointer [nterms][npoly][level][N] with a term stride and a poly stride.
        b0 = b1 = None is the square form: (sum a0^2, 2 sum a0 a1, sum a1^2).  One launch."""
        atst, apst, btst, bpst = self._ctmul_operands(a0, a1, b0, b1, nterms, npoly, level, a_term_stride,
                                                      a_poly_stride, b_term_stride, b_poly_stride, "ctmul_tensor")
        ost = level * self.N if d01_stride is None else d01_stride
        o2st = level * self.N if d2_stride is None else d2_stride
        self._need_polys(d0, npoly, ost, level, self.N, "ctmul_tensor d0")
        self._need_polys(d1, npoly, ost, level, self.N, "ctmul_tensor d1")
        self._need_polys(d2, npoly, o2st, level, self.N, "ctmul_tensor d2")
        check(lib.mfhe_ctmul_tensor(self._h, _ptr(a0), _ptr(a1), atst, apst, _ptr(b0), _ptr(b1), btst, bpst, nterms,
                                    _ptr(d0), _ptr(d1), ost, _ptr(d2), o2st, npoly, level, _stream_ptr(stream)),
              "ctmul_tensor")
        return d0, d1, d2

    def ctmul_reserve(self, npoly, level, key_level, alpha, special_start, nspecial, flags=0):
        """Grow the workspace and build every table of this geometry (the rescale's with CTMUL_RESCALE): ctmul then
        allocates nothing and copies nothing to the device."""
        check(lib.mfhe_ctmul_reserve(self._h, npoly, level, key_level, alpha, special_start, nspecial, flags),
              "ctmul_reserve")

    def ctmul(self, a0, a1, b0, b1, rlk, out0, out1, npoly, level, key_level, alpha, special_start, nspecial,
              nterms=1, flags=0, a_term_stride=None, a_poly_stride=None, b_term_stride=None, b_poly_stride=None,
              out_stride=None, stream=None):
        """(out0, out1), each [npoly][level][N] = the relinearised sum of the nterms products of the ciphertexts
        (a0, a1) and (b0, b1) (b0 = b1 = None: the squares of (a0, a1)) with the relinearisation key rlk:
        ctmul_tensor, then keyswitch(KS_ADD) of d2.  flags: CTMUL_RESCALE also divides by q_(level-1); rows
        [0, level - 1) of the outputs then hold the result at level - 1."""
        atst, apst, btst, bpst = self._ctmul_operands(a0, a1, b0, b1, nterms, npoly, level, a_term_stride,
                                                      a_poly_stride, b_term_stride, b_poly_stride, "ctmul")
        ost = level * self.N if out_stride is None else out_stride
        self._need_polys(out0, npoly, ost, level, self.N, "ctmul out0")
        self._need_polys(out1, npoly, ost, level, self.N, "ctmul out1")
        if rlk is not None:
            self._need_polys(rlk, -(-key_level // max(alpha, 1)), 2 * (key_level + nspecial) * self.N,
                             2 * (key_level + nspecial), self.N, "ctmul rlk")
        check(lib.mfhe_ctmul_apply(self._h, _ptr(a0), _ptr(a1), atst, apst, _ptr(b0), _ptr(b1), btst, bpst, nterms,
                                   _ptr(rlk), _ptr(out0), _ptr(out1), ost, npoly, level, key_level, alpha,
                                   special_start, nspecial, flags, _stream_ptr(stream)), "ctmul")
        return out0, out1

    # ---- products of matrices of ciphertexts (include/mfhe.h): C = A B, A m x k and B k x n ciphertexts of npoly
    # polynomials per component; one tiled launch where m n ctmul_tensor calls stream A n times and B m times
    def _ctmat_need(self, t, rows, cols, npoly, level, row, col, poly, what):
        """The buffer holds a rows x cols matrix of entries at these strides."""
        lw = level * self.N
        last = (rows - 1) * row + (cols - 1) * col + (npoly - 1) * poly + lw
        _need(t, last if npoly and rows > 0 and cols > 0 else 0, what)

    def _ctmat_operands(self, a0, a1, b0, b1, m, n, k, npoly, level, a_strides, b_strides, what):
        """Dense strides [m][k][npoly][level][N] and [k][n][npoly][level][N] by default, the operand buffers
        size-checked: ((a_row, a_col, a_poly), (b_row, b_col, b_poly))."""
        lw = level * self.N
        a = (k * npoly * lw, npoly * lw, lw) if a_strides is None else tuple(a_strides)
        b = (n * npoly * lw, npoly * lw, lw) if b_strides is None else tuple(b_strides)
        for t, name in ((a0, "a0"), (a1, "a1")):
            self._ctmat_need(t, m, k, npoly, level, *a, f"{what} {name}")
        for t, name in ((b0, "b0"), (b1, "b1")):
            self._ctmat_need(t, k, n, npoly, level, *b, f"{what} {name}")
        return a, b

    def ctmat_tensor(self, a0, a1, b0, b1, d0, d1, d2, m, n, k, npoly, level, a_strides=None, b_strides=None,
                     d01_strides=None, d2_strides=None, stream=None):
        """(d0, d1, d2)[i][j] = sum_t (a0 b0, a0 b1 + a1 b0, a1 b1) of a[i][t] and b[t][j] mod q_r for the m x k matrix
        (a0, a1) and the k x n matrix (b0, b1) of ciphertexts, npoly polynomials [level][N] per entry and component.  Every
        *_strides is (row, col, poly) in words, dense by default: [m][k], [k][n] and [m][n] entries of
        [npoly][level][N]; a transposed operand is the same memory with row and col swapped.  One launch, bit-identical
        to m n ctmul_tensor calls."""
        a, b = self._ctmat_operands(a0, a1, b0, b1, m, n, k, npoly, level, a_strides, b_strides, "ctmat_tensor")
        lw = level * self.N
        o = (n * npoly * lw, npoly * lw, lw) if d01_strides is None else tuple(d01_strides)
        o2 = (n * npoly * lw, npoly * lw, lw) if d2_strides is None else tuple(d2_strides)
        self._ctmat_need(d0, m, n, npoly, level, *o, "ctmat_tensor d0")
        self._ctmat_need(d1, m, n, npoly, level, *o, "ctmat_tensor d1")
        self._ctmat_need(d2, m, n, npoly, level, *o2, "ctmat_tensor d2")
        check(lib.mfhe_ctmat_tensor(self._h, _ptr(a0), _ptr(a1), *a, _ptr(b0), _ptr(b1), *b, m, n, k, _ptr(d0),
                                    _ptr(d1), *o, _ptr(d2), *o2, npoly, level, _stream_ptr(stream)), "ctmat_tensor")
        return d0, d1, d2

    def ctmat_reserve(self, m, n, npoly, level, key_level, alpha, special_start, nspecial, flags=0):
        """Grow the workspace and build every table of this geometry (the rescale's with CTMUL_RESCALE): ctmat then
        allocates nothing and copies nothing to the device."""
        check(lib.mfhe_ctmat_reserve(self._h, m, n, npoly, level, key_level, alpha, special_start, nspecial, flags),
              "ctmat_reserve")

    def ctmat(self, a0, a1, b0, b1, rlk, out0, out1, m, n, k, npoly, level, key_level, alpha, special_start, nspecial,
              flags=0, a_strides=None, b_strides=None, out_stride=None, stream=None):
        """(out0, out1), each [m][n][npoly][level][N] at one poly stride = the relinearised product of the m x k matrix
        (a0, a1) and the k x n matrix (b0, b1) of ciphertexts with the relinearisation key rlk: ctmat_tensor, then one
        keyswitch(KS_ADD) of d2 over all m n npoly polynomials.  flags: CTMUL_RESCALE also divides by q_(level-1).
        Bit-identical to m n ctmul calls, one per entry."""
        a, b = self._ctmat_operands(a0, a1, b0, b1, m, n, k, npoly, level, a_strides, b_strides, "ctmat")
        ost = level * self.N if out_stride is None else out_stride
        batch = max(m, 0) * max(n, 0) * npoly
        self._need_polys(out0, batch, ost, level, self.N, "ctmat out0")
        self._need_polys(out1, batch, ost, level, self.N, "ctmat out1")
        if rlk is not None:
            self._need_polys(rlk, -(-key_level // max(alpha, 1)), 2 * (key_level + nspecial) * self.N,
                             2 * (key_level + nspecial), self.N, "ctmat rlk")
        check(lib.mfhe_ctmat_apply(self._h, _ptr(a0), _ptr(a1), *a, _ptr(b0), _ptr(b1), *b, m, n, k, _ptr(rlk),
                                   _ptr(out0), _ptr(out1), ost, npoly, level, key_level, alpha, special_start,
                                   nspecial, flags, _stream_ptr(stream)), "ctmat")
        return out0, out1

    # ---- plaintext x ciphertext products (include/mfhe.h): the plaintext-weighted sum, and Y = W X + B for an m x k
    # matrix W of plaintexts and a k x n matrix X of ciphertexts in one tiled launch, with one rescale per product
    def ptmul_sum(self, x0, x1, pt, out0, out1, term_x, term_pt, npoly, level, nsrc, npt, addend_pt=-1,
                  src_stride=None, x_poly_stride=None, pt_stride=None, pt_poly_stride=None, out_stride=None,
                  stream=None):
        """(out0, out1), each [npoly][level][N] = sum_t pt[term_pt[t]] (x0, x1)[term_x[t]] + (pt[addend_pt], 0) mod
        q_r: x0, x1 the components of nsrc ciphertexts, each [nsrc][npoly][>= level rows][N] with a source stride and a
        poly stride; pt npt plaintexts [npt][npoly][>= level rows][N] with a pt stride and a pt poly stride, or with
        pt_poly_stride = 0 one plaintext per index shared by the batch, [npt][>= level rows][N]; term_x, term_pt Python
        lists of 1 .. 64 entries.  One launch."""
        lw = level * self.N
        pst = lw if x_poly_stride is None else x_poly_stride
        sst = npoly * pst if src_stride is None else src_stride
        ppst = lw if pt_poly_stride is None else pt_poly_stride
        ptst = (npoly * ppst if ppst else lw) if pt_stride is None else pt_stride
        ost = lw if out_stride is None else out_stride
        if len(term_x) != len(term_pt):
            raise ValueError("ptmul_sum: term_x and term_pt differ in length")
        for t, what in ((x0, "x0"), (x1, "x1")):
            self._need_polys(t, npoly, pst, level, self.N, f"ptmul_sum {what} (one source)")
            _need(t, (nsrc - 1) * sst + (npoly - 1) * pst + lw if npoly and nsrc > 0 else 0, f"ptmul_sum {what}")
        _need(pt, (npt - 1) * ptst + (npoly - 1) * ppst + lw if npoly and npt > 0 else 0, "ptmul_sum pt")
        self._need_polys(out0, npoly, ost, level, self.N, "ptmul_sum out0")
        self._need_polys(out1, npoly, ost, level, self.N, "ptmul_sum out1")
        nt = len(term_x)
        tx, tp = (_int * max(nt, 1))(*term_x), (_int * max(nt, 1))(*term_pt)
        check(lib.mfhe_ptmul_sum(self._h, _ptr(x0), _ptr(x1), sst, pst, nsrc, _ptr(pt), ptst, ppst, npt, tx, tp, nt,
                                 addend_pt, _ptr(out0), _ptr(out1), ost, npoly, level, _stream_ptr(stream)),
              "ptmul_sum")
        return out0, out1

    def _ptmat_operands(self, w, x0, x1, bias, m, n, k, npoly, level, w_strides, x_strides, bias_strides, what):
        """Dense strides [m][k][npoly][level][N], [k][n][npoly][level][N] and [m][n][npoly][level][N] by default, the
        operand buffers size-checked: ((w_row, w_col, w_poly), (x_row, x_col, x_poly), (b_row, b_col, b_poly))."""
        lw = level * self.N
        ws = (k * npoly * lw, npoly * lw, lw) if w_strides is None else tuple(w_strides)
        xs = (n * npoly * lw, npoly * lw, lw) if x_strides is None else tuple(x_strides)
        bs = (n * npoly * lw, npoly * lw, lw) if bias_strides is None else tuple(bias_strides)
        self._ctmat_need(w, m, k, npoly, level, *ws, f"{what} w")
        for t, name in ((x0, "x0"), (x1, "x1")):
            self._ctmat_need(t, k, n, npoly, level, *xs, f"{what} {name}")
        if bias is not None:
            self._ctmat_need(bias, m, n, npoly, level, *bs, f"{what} bias")
        return ws, xs, bs

    def ptmat_tensor(self, w, x0, x1, out0, out1, m, n, k, npoly, level, bias=None, flags=0, w_strides=None,
                     x_strides=None, bias_strides=None, out_strides=None, stream=None):
        """(out0, out1)[i][j] = sum_t w[i][t] (x0, x1)[t][j] + (bias[i][j], 0) mod q_r for the m x k matrix w of
        plaintexts and the k x n matrix (x0, x1) of ciphertexts, npoly polynomials [level][N] per entry (and component).
        Every *_strides is (row, col, poly) in words, dense by default; a transposed operand is the same memory with
        row and col swapped.  w's poly stride may be 0 (one plaintext per entry for the whole batch); each of the bias'
        three strides may be 0 (one row, one column, one polynomial of bias broadcast).  flags: PTMUL_ADD adds what the
        outputs hold into the sums.  One launch, bit-identical to m n ptmul_sum calls."""
        ws, xs, bs = self._ptmat_operands(w, x0, x1, bias, m, n, k, npoly, level, w_strides, x_strides, bias_strides,
                                          "ptmat_tensor")
        lw = level * self.N
        o = (n * npoly * lw, npoly * lw, lw) if out_strides is None else tuple(out_strides)
        self._ctmat_need(out0, m, n, npoly, level, *o, "ptmat_tensor out0")
        self._ctmat_need(out1, m, n, npoly, level, *o, "ptmat_tensor out1")
        check(lib.mfhe_ptmat_tensor(self._h, _ptr(w), *ws, _ptr(x0), _ptr(x1), *xs, m, n, k, _ptr(bias), *bs,
                                    _ptr(out0), _ptr(out1), *o, npoly, level, flags, _stream_ptr(stream)),
              "ptmat_tensor")
        return out0, out1

    def ptmat_reserve(self, m, n, npoly, level, flags=0):
        """Grow the workspace and build the rescale's table (with PTMUL_RESCALE; nothing is needed without): ptmat then
        allocates nothing and copies nothing to the device."""
        check(lib.mfhe_ptmat_reserve(self._h, m, n, npoly, level, flags), "ptmat_reserve")

    def ptmat(self, w, x0, x1, out0, out1, m, n, k, npoly, level, bias=None, flags=0, w_strides=None, x_strides=None,
              bias_strides=None, out_stride=None, stream=None):
        """(out0, out1), each [m][n][npoly][level][N] at one poly stride = w (x0, x1) + (bias, 0) as ptmat_tensor
        computes it.  flags: PTMUL_ADD as there; PTMUL_RESCALE also divides by q_(level-1) in one ModDown over all
        m n npoly polynomials, and rows [0, level - 1) of the outputs then hold the result at level - 1."""
        ws, xs, bs = self._ptmat_operands(w, x0, x1, bias, m, n, k, npoly, level, w_strides, x_strides, bias_strides,
                                          "ptmat")
        ost = level * self.N if out_stride is None else out_stride
        batch = max(m, 0) * max(n, 0) * npoly
        self._need_polys(out0, batch, ost, level, self.N, "ptmat out0")
        self._need_polys(out1, batch, ost, level, self.N, "ptmat out1")
        check(lib.mfhe_ptmat_apply(self._h, _ptr(w), *ws, _ptr(x0), _ptr(x1), *xs, m, n, k, _ptr(bias), *bs,
                                   _ptr(out0), _ptr(out1), ost, npoly, level, flags, _stream_ptr(stream)), "ptmat")
        return out0, out1

    # ---- encrypted polynomial evaluation (include/mfhe.h): scalar sums of ciphertexts and the plans built on them
    def ct_lincomb(self, x0, x1, k, out0, out1, term_x, term_k, npoly, level, nsrc, nk, addend_k=-1, src_stride=None,
                   x_poly_stride=None, k_stride=None, out_stride=None, stream=None):
        """(out0, out1), each [npoly][level][N] = sum_t k[term_k[t]] (x0, x1)[term_x[t]] + (k[addend_k], 0) mod q_r: x0,
        x1 the components of nsrc ciphertexts, each [nsrc][npoly][>= level rows][N] with a source stride and a poly
        stride, k [nk][>= level] residues of the constants (or a PolyPlan: its table; nk and k_stride are then the
        plan's); term_x, term_k Python lists of 1 .. 64 entries.  One launch."""
        lw = level * self.N
        pst = lw if x_poly_stride is None else x_poly_stride
        sst = npoly * pst if src_stride is None else src_stride
        if isinstance(k, PolyPlan):   # the plan's own table, by its device address
            kinfo = k.info()
            kptr, nk, kst = k.table_ptr(), kinfo.nconst, kinfo.level
        else:
            kst = level if k_stride is None else k_stride
            _need(k, (nk - 1) * kst + level if nk > 0 else 0, "ct_lincomb k")
            kptr = _ptr(k)
        ost = lw if out_stride is None else out_stride
        if len(term_x) != len(term_k):
            raise ValueError("ct_lincomb: term_x and term_k differ in length")
        for t, what in ((x0, "x0"), (x1, "x1")):
            self._need_polys(t, npoly, pst, level, self.N, f"ct_lincomb {what} (one source)")
            _need(t, (nsrc - 1) * sst + (npoly - 1) * pst + lw if npoly and nsrc > 0 else 0, f"ct_lincomb {what}")
        self._need_polys(out0, npoly, ost, level, self.N, "ct_lincomb out0")
        self._need_polys(out1, npoly, ost, level, self.N, "ct_lincomb out1")
        nt = len(term_x)
        tx, tk = (_int * max(nt, 1))(*term_x), (_int * max(nt, 1))(*term_k)
        check(lib.mfhe_ct_lincomb(self._h, _ptr(x0), _ptr(x1), sst, pst, nsrc, kptr, kst, nk, tx, tk, nt, addend_k,
                                  _ptr(out0), _ptr(out1), ost, npoly, level, _stream_ptr(stream)), "ct_lincomb")
        return out0, out1

    def poly_plan(self, coeffs, basis, in_scale, level) -> "PolyPlan":
        """The baby-step giant-step plan of sum_i coeffs[i] x^i (POLY_MONOMIAL) or sum_i coeffs[i] T_i(x)
        (POLY_CHEBYSHEV) for an input at `level` and scale in_scale."""
        return PolyPlan(self, coeffs, basis, in_scale, level)

    def poly_reserve(self, plan, npoly, key_level, alpha, special_start, nspecial):
        """Grow the workspace and build every table of every level the plan touches: poly_apply then allocates nothing
        and copies nothing to the device."""
        check(lib.mfhe_poly_reserve(self._h, plan.handle, npoly, key_level, alpha, special_start, nspecial),
              "poly_reserve")

    def poly_apply(self, plan, c0, c1, rlk, out0, out1, npoly, key_level, alpha, special_start, nspecial,
                   in_stride=None, out_stride=None, stream=None):
        """(out0, out1), each [npoly][out_level][N] = the plan's polynomial of the ciphertexts (c0, c1), each
        [npoly][level][N] at the plan's level, with the relinearisation key rlk; the result is at plan.info().out_level
        and out_scale."""
        info = plan.info()
        ist = info.level * self.N if in_stride is None else in_stride
        ost = info.out_level * self.N if out_stride is None else out_stride
        self._need_polys(c0, npoly, ist, info.level, self.N, "poly_apply c0")
        self._need_polys(c1, npoly, ist, info.level, self.N, "poly_apply c1")
        self._need_polys(out0, npoly, ost, info.out_level, self.N, "poly_apply out0")
        self._need_polys(out1, npoly, ost, info.out_level, self.N, "poly_apply out1")
        if rlk is not None:
            self._need_polys(rlk, -(-key_level // max(alpha, 1)), 2 * (key_level + nspecial) * self.N,
                             2 * (key_level + nspecial), self.N, "poly_apply rlk")
        check(lib.mfhe_poly_apply(self._h, plan.handle, _ptr(c0), _ptr(c1), ist, _ptr(rlk), _ptr(out0), _ptr(out1),
                                  ost, npoly, key_level, alpha, special_start, nspecial, _stream_ptr(stream)),
              "poly_apply")
        return out0, out1

    # ---- CKKS slots (include/mfhe.h mfhe_slot_*): slot j of a polynomial m is m(zeta^(5^j)), zeta = e^(i pi / N) ----
    def _slot_words(self, t, npoly, stride, flags, what):
        """Checks a slot tensor (float64, interleaved (re, im) unless SLOT_REAL, or complex128) and returns the stride
        in doubles: npoly blocks of N (N / 2 with SLOT_REAL) doubles."""
        import torch
        if t.dtype == torch.complex128:
            if flags & SLOT_REAL:
                raise ValueError(f"{what}: SLOT_REAL takes a float64 tensor")
        elif t.dtype != torch.float64:
            raise ValueError(f"{what}: slots are float64 or complex128, not {t.dtype}")
        width = self.N // 2 if flags & SLOT_REAL else self.N
        st = width if stride is None else stride
        self._need_polys(t, npoly, st, 1, width, what)
        return st

    def slot_reserve(self, npoly, level, special_start=0, nspecial=0):
        """Grow the workspace and build the table of this geometry: slot_encode and slot_decode of up to npoly
        polynomials then allocate nothing and copy nothing to the device."""
        check(lib.mfhe_slot_reserve(self._h, npoly, level, special_start, nspecial), "slot_reserve")

    def slot_encode(self, slots, out, npoly, level, scale, special_start=0, nspecial=0, flags=0, slot_stride=None,
                    out_stride=None, stream=None):
        """out [npoly][level + nspecial][N] = the residues of rint(scale c), c the real polynomial whose slots are
        `slots` ([npoly][N / 2] complex128, the same as [npoly][N] float64 interleaved; [npoly][N / 2] float64 with
        SLOT_REAL), in the evaluation domain unless SLOT_COEFF.  Row r >= level is special limb special_start + r -
        level.  slot_stride in doubles, out_stride in words."""
        sst = self._slot_words(slots, npoly, slot_stride, flags, "slot_encode slots")
        rows = level + nspecial
        ost = rows * self.N if out_stride is None else out_stride
        self._need_polys(out, npoly, ost, rows, self.N, "slot_encode out")
        check(lib.mfhe_slot_encode(self._h, _ptr(slots), sst, float(scale), _ptr(out), ost, npoly, level,
                                   special_start, nspecial, flags, _stream_ptr(stream)), "slot_encode")
        return out

    def slot_decode(self, src, slots, npoly, level, scale, flags=0, in_stride=None, slot_stride=None, stream=None):
        """slots = the slot values of the polynomials src [npoly][level][N] (limbs [0, min(level, 2)) are read,
        composed, centred and converted to f64), divided by scale.  Evaluation domain unless SLOT_COEFF."""
        sst = self._slot_words(slots, npoly, slot_stride, flags, "slot_decode slots")
        ist = level * self.N if in_stride is None else in_stride
        self._need_polys(src, npoly, ist, min(level, 2), self.N, "slot_decode src")
        check(lib.mfhe_slot_decode(self._h, _ptr(src), ist, float(scale), _ptr(slots), sst, npoly, level, flags,
                                   _stream_ptr(stream)), "slot_decode")
        return slots

    # ---- RLWE keys, encryption, decryption (include/mfhe.h mfhe_rlwe_*): seeded ChaCha20 draws on the key switch's
    # layout; `seed` is a Seed (or 32 bytes), `first_id` the first polynomial id of the call (Seed.take hands out ranges)
    def rlwe_reserve(self, npoly, level, special_start=0, nspecial=0):
        """Grow the workspace for every rlwe_* call at this geometry: they then allocate nothing and copy nothing to
        the device (rlwe_ksk_gen at key_level = level: npoly >= beta)."""
        check(lib.mfhe_rlwe_reserve(self._h, npoly, level, special_start, nspecial), "rlwe_reserve")

    def rlwe_sample_uniform(self, seed, first_id, out, npoly, level, special_start=0, nspecial=0, out_stride=None,
                            stream=None):
        """out [npoly][level + nspecial][N] = the mask residues of ids first_id .. first_id + npoly - 1."""
        rows = level + nspecial
        ost = rows * self.N if out_stride is None else out_stride
        self._need_polys(out, npoly, ost, rows, self.N, "rlwe_sample_uniform out")
        check(lib.mfhe_rlwe_sample_uniform(self._h, _seed_words(seed), first_id, _ptr(out), ost, npoly, level,
                                           special_start, nspecial, _stream_ptr(stream)), "rlwe_sample_uniform")
        return out

    def rlwe_sample_small(self, seed, stream_id, first_id, out, npoly, level, special_start=0, nspecial=0, flags=0,
                          out_stride=None, stream=None):
        """out [npoly][level + nspecial][N] = the residues of the small integers of stream `stream_id` (RLWE_NOISE ..
        RLWE_NOISE1), in the evaluation domain unless RLWE_COEFF.  A secret key: RLWE_SECRET at key_level + K rows."""
        rows = level + nspecial
        ost = rows * self.N if out_stride is None else out_stride
        self._need_polys(out, npoly, ost, rows, self.N, "rlwe_sample_small out")
        check(lib.mfhe_rlwe_sample_small(self._h, _seed_words(seed), stream_id, first_id, _ptr(out), ost, npoly, level,
                                         special_start, nspecial, flags, _stream_ptr(stream)), "rlwe_sample_small")
        return out

    def rlwe_lift_small(self, coeffs, out, npoly, level, special_start=0, nspecial=0, flags=0, coeff_stride=None,
                        out_stride=None, stream=None):
        """out [npoly][level + nspecial][N] = the residues of the int32 coefficients [npoly][N] (coeff_stride in
        int32), in the evaluation domain unless RLWE_COEFF: the caller's own small polynomials."""
        import torch
        if coeffs.dtype != torch.int32:
            raise ValueError(f"rlwe_lift_small: coefficients are int32, not {coeffs.dtype}")
        rows = level + nspecial
        cst = self.N if coeff_stride is None else coeff_stride
        ost = rows * self.N if out_stride is None else out_stride
        if cst < self.N:
            raise ValueError("rlwe_lift_small: coefficient stride smaller than N")
        if npoly and coeffs.numel() < (npoly - 1) * cst + self.N:
            raise ValueError("rlwe_lift_small coeffs: tensor smaller than the polynomials it holds")
        self._need_polys(out, npoly, ost, rows, self.N, "rlwe_lift_small out")
        check(lib.mfhe_rlwe_lift_small(self._h, _ptr(coeffs), cst, _ptr(out), ost, npoly, level, special_start,
                                       nspecial, flags, _stream_ptr(stream)), "rlwe_lift_small")
        return out

    def rlwe_encrypt_sk(self, seed, first_id, s, m, c0, c1, npoly, level, special_start=0, nspecial=0, m_stride=None,
                        out_stride=None, stream=None):
        """(c0, c1) [npoly][level + nspecial][N] with c1 = a, c0 = m + e - a s under the secret s [level + nspecial][N];
        m None encrypts zero (a public key is that call with npoly = 1)."""
        rows = level + nspecial
        mst = rows * self.N if m_stride is None else m_stride
        ost = rows * self.N if out_stride is None else out_stride
        self._need_polys(s, 1, rows * self.N, rows, self.N, "rlwe_encrypt_sk s")
        if m is not None:
            self._need_polys(m, npoly, mst, rows, self.N, "rlwe_encrypt_sk m")
        self._need_polys(c0, npoly, ost, rows, self.N, "rlwe_encrypt_sk c0")
        self._need_polys(c1, npoly, ost, rows, self.N, "rlwe_encrypt_sk c1")
        check(lib.mfhe_rlwe_encrypt_sk(self._h, _seed_words(seed), first_id, _ptr(s), _ptr(m), mst, _ptr(c0), _ptr(c1),
                                       ost, npoly, level, special_start, nspecial, _stream_ptr(stream)),
              "rlwe_encrypt_sk")
        return c0, c1

    def rlwe_ksk_gen(self, seed, first_id, kind, s_to, ksk, key_level, alpha, special_start, nspecial, s_from=None,
                     galois_elt=1, stream=None):
        """ksk [beta][2][key_level + K][N]: a switching key to s_to from s_from (RLWE_KEY_SWITCH), from s_to^2
        (RLWE_KEY_RELIN) or from sigma_g(s_to) (RLWE_KEY_GALOIS); digit j draws at id first_id + j."""
        rows, beta = key_level + nspecial, -(-key_level // max(alpha, 1))
        self._need_polys(s_to, 1, rows * self.N, rows, self.N, "rlwe_ksk_gen s_to")
        if s_from is not None:
            self._need_polys(s_from, 1, rows * self.N, rows, self.N, "rlwe_ksk_gen s_from")
        self._need_polys(ksk, beta, 2 * rows * self.N, 2 * rows, self.N, "rlwe_ksk_gen ksk")
        check(lib.mfhe_rlwe_ksk_gen(self._h, _seed_words(seed), first_id, kind, galois_elt, _ptr(s_from), _ptr(s_to),
                                    _ptr(ksk), key_level, alpha, special_start, nspecial, _stream_ptr(stream)),
              "rlwe_ksk_gen")
        return ksk

    def rlwe_encrypt_pk(self, seed, first_id, pk0, pk1, m, c0, c1, npoly, level, m_stride=None, out_stride=None,
                        stream=None):
        """(c0, c1) [npoly][level][N] = (pk0 u + e0 + m, pk1 u + e1) on rows [0, level) of the public key; m None
        encrypts zero."""
        mst = level * self.N if m_stride is None else m_stride
        ost = level * self.N if out_stride is None else out_stride
        self._need_polys(pk0, 1, level * self.N, level, self.N, "rlwe_encrypt_pk pk0")
        self._need_polys(pk1, 1, level * self.N, level, self.N, "rlwe_encrypt_pk pk1")
        if m is not None:
            self._need_polys(m, npoly, mst, level, self.N, "rlwe_encrypt_pk m")
        self._need_polys(c0, npoly, ost, level, self.N, "rlwe_encrypt_pk c0")
        self._need_polys(c1, npoly, ost, level, self.N, "rlwe_encrypt_pk c1")
        check(lib.mfhe_rlwe_encrypt_pk(self._h, _seed_words(seed), first_id, _ptr(pk0), _ptr(pk1), _ptr(m), mst,
                                       _ptr(c0), _ptr(c1), ost, npoly, level, _stream_ptr(stream)), "rlwe_encrypt_pk")
        return c0, c1

    def rlwe_decrypt(self, c0, c1, s, out, npoly, rows, in_stride=None, out_stride=None, stream=None):
        """out [npoly][rows][N] = c0 + c1 s on rows [0, rows); rows = min(level, 2) is all slot_decode reads."""
        ist = rows * self.N if in_stride is None else in_stride
        ost = rows * self.N if out_stride is None else out_stride
        self._need_polys(c0, npoly, ist, rows, self.N, "rlwe_decrypt c0")
        self._need_polys(c1, npoly, ist, rows, self.N, "rlwe_decrypt c1")
        self._need_polys(s, 1, rows * self.N, rows, self.N, "rlwe_decrypt s")
        self._need_polys(out, npoly, ost, rows, self.N, "rlwe_decrypt out")
        check(lib.mfhe_rlwe_decrypt(self._h, _ptr(c0), _ptr(c1), ist, _ptr(s), _ptr(out), ost, npoly, rows,
                                    _stream_ptr(stream)), "rlwe_decrypt")
        return out

    def crt_recombine_sharded(self, comm: "Comm", mode, shard, npoly, ncoeff, out, out_stride=1, stream=None):
        """RCCL exchange of this rank's [npoly][L/G][ncoeff] residue shard + compose of its polynomial slice
        (include/mfhe.h mfhe_crt_recombine_sharded); out: npoly/G * ncoeff f64."""
        m = _XCHG[mode] if isinstance(mode, str) else mode
        g = comm.size
        lg = self.info().num_limbs // g if g else 0
        _need(shard, npoly * lg * ncoeff, "shard")
        # the kernel writes out[i * out_stride] for i < npoly / G * ncoeff
        _need_strided(out, (npoly // g) * ncoeff if g else 0, out_stride, "out")
        check(lib.mfhe_crt_recombine_sharded(self._h, comm._h, m, _ptr(shard), npoly, ncoeff, _ptr(out), out_stride,
                                             _stream_ptr(stream)), "crt_recombine_sharded")
        return out

    def crt_recombine_reserve(self, comm: "Comm", mode, npoly, ncoeff):
        m = _XCHG[mode] if isinstance(mode, str) else mode
        check(lib.mfhe_crt_recombine_reserve(self._h, comm._h, m, npoly, ncoeff), "crt_recombine_reserve")

    def crt_recombine_chunked(self, comm: "Comm", mode, shard, npoly, ncoeff, chunk_polys, out, out_stride=1,
                              rows_global=False, stream=None, flags=0):
        """Chunked, pipelined RCCL recombine (include/mfhe.h mfhe_crt_recombine_chunked): exchange of chunk k + 1
        on the communicator's stream beside the compose of chunk k on `stream`.  out rows: owned_polys order
        (npoly/G rows), or the global poly index with rows_global (npoly rows, only this rank's written).
        flags: further MFHE_RECOMBINE_* bits (RECOMBINE_EXCHANGE_ONLY: out may be None)."""
        m = _XCHG[mode] if isinstance(mode, str) else mode
        g = comm.size
        lg = self.info().num_limbs // g if g else 0
        _need(shard, npoly * lg * ncoeff, "shard")
        rows = npoly if rows_global else (npoly // g if g else 0)
        if out is not None or not flags & RECOMBINE_EXCHANGE_ONLY:
            _need_strided(out, rows * ncoeff, out_stride, "out")
        check(lib.mfhe_crt_recombine_chunked(self._h, comm._h, m, _ptr(shard), npoly, ncoeff, chunk_polys,
                                             _ptr(out) if out is not None else None, out_stride,
                                             (RECOMBINE_ROWS_GLOBAL if rows_global else 0) | flags,
                                             _stream_ptr(stream)), "crt_recombine_chunked")
        return out

    def crt_recombine_chunked_reserve(self, comm: "Comm", mode, chunk_polys, ncoeff):
        m = _XCHG[mode] if isinstance(mode, str) else mode
        check(lib.mfhe_crt_recombine_chunked_reserve(self._h, comm._h, m, chunk_polys, ncoeff),
              "crt_recombine_chunked_reserve")

    # ---- W axis / encoder / pipelines (reference geometry, CONV_WCRT) ----
    def _call(self, name, *ptrs, stream=None):
        fn = getattr(lib, name)
        check(fn(self._h, *ptrs, _stream_ptr(stream)), name)

    # host-side sizes of the fixed-geometry buffers (phi = 512 W-lanes), checked before raw pointers cross
    def _mat(self):   # one matrix-major [phi][L][n*n] (or poly-major [phi*n][L][n]) residue array
        return 512 * self.L * self.N * self.N

    def _msg(self):   # one [phi][n*n] complex message, interleaved doubles
        return 2 * 512 * self.N * self.N

    def _sk(self):    # secret key [phi][L][n]
        return 512 * self.L * self.N

    def _sizes(self, what, *pairs):
        for t, words in pairs:
            _need(t, words, what)

    def wcrt_fwd(self, src, dst, stream=None):
        self._sizes("wcrt_fwd", (src, self._mat()), (dst, self._mat()))
        self._call("mfhe_wcrt_fwd", _ptr(src), _ptr(dst), stream=stream); return dst
    def wcrt_inv(self, src, dst, stream=None):
        self._sizes("wcrt_inv", (src, self._mat()), (dst, self._mat()))
        self._call("mfhe_wcrt_inv", _ptr(src), _ptr(dst), stream=stream); return dst
    def wcrt_fwd_vector(self, src, dst, stream=None):
        self._call("mfhe_wcrt_fwd_vector", _ptr(src), _ptr(dst), stream=stream); return dst
    def wcrt_fwd_centered(self, src, dst, stream=None):
        self._call("mfhe_wcrt_fwd_centered", _ptr(src), _ptr(dst), stream=stream); return dst
    def wcrt_inv_centered(self, src, dst, stream=None):
        self._call("mfhe_wcrt_inv_centered", _ptr(src), _ptr(dst), stream=stream); return dst
    def wdft_fwd(self, src, dst, stream=None): self._call("mfhe_wdft_fwd", _ptr(src), _ptr(dst), stream=stream); return dst
    def wdft_inv(self, src, dst, stream=None): self._call("mfhe_wdft_inv", _ptr(src), _ptr(dst), stream=stream); return dst
    def wdft_fwd_pair_i64(self, re, im, out_re, out_im, stream=None):
        self._call("mfhe_wdft_fwd_pair_i64", _ptr(re), _ptr(im), _ptr(out_re), _ptr(out_im), stream=stream)
    def wdft_inv_pair(self, re, im, out_re, out_im, stream=None):
        self._call("mfhe_wdft_inv_pair", _ptr(re), _ptr(im), _ptr(out_re), _ptr(out_im), stream=stream)
    def ct_add(self, ct1, ct2, res, stream=None):
        self._sizes("ct_add", *[(t, 2 * self._mat()) for t in (ct1, ct2, res)])
        self._call("mfhe_ct_add", _ptr(ct1), _ptr(ct2), _ptr(res), stream=stream); return res
    def ct_mul_tensor(self, ct1, ct2, d0, d1, d2, stream=None):
        self._sizes("ct_mul_tensor", (ct1, 2 * self._mat()), (ct2, 2 * self._mat()),
                    *[(t, self._mat()) for t in (d0, d1, d2)])
        self._call("mfhe_ct_mul_tensor", _ptr(ct1), _ptr(ct2), _ptr(d0), _ptr(d1), _ptr(d2), stream=stream)
    # ---- trace GEMM, planes [batch][nlimbs][n][n] (batched_trace.cu) ----
    @staticmethod
    def _trace_need(tensors, n, nlimbs, batch, what):
        """Every plane must hold batch * nlimbs * n * n int64/uint64 words (checked before raw pointers cross)."""
        import torch
        words = batch * nlimbs * n * n
        for t in tensors:
            if t.dtype not in (torch.int64, torch.uint64):
                raise ValueError(f"{what}: planes must be int64/uint64, got {t.dtype}")
            _need(t, words, what)

    def trace_map_bprime(self, b_re, b_im, bp_re, bp_im, n, nlimbs, batch, stream=None):
        self._trace_need((b_re, b_im, bp_re, bp_im), n, nlimbs, batch, "trace_map_bprime")
        check(lib.mfhe_trace_map_bprime(self._h, _ptr(b_re), _ptr(b_im), _ptr(bp_re), _ptr(bp_im), n, nlimbs, batch,
                                        _stream_ptr(stream)), "trace_map_bprime")
    def trace_gemm(self, a_re, a_im, bp_re, bp_im, c_re, c_im, n, nlimbs, batch, stream=None):
        self._trace_need((a_re, a_im, bp_re, bp_im, c_re, c_im), n, nlimbs, batch, "trace_gemm")
        check(lib.mfhe_trace_gemm(self._h, _ptr(a_re), _ptr(a_im), _ptr(bp_re), _ptr(bp_im), _ptr(c_re), _ptr(c_im),
                                  n, nlimbs, batch, _stream_ptr(stream)), "trace_gemm")
    def trace_rescale(self, c_re, c_im, n, nlimbs, batch, inv, stream=None):
        self._trace_need((c_re, c_im), n, nlimbs, batch, "trace_rescale")
        arr = (ctypes.c_uint64 * nlimbs)(*[int(v) for v in inv[:nlimbs]])
        check(lib.mfhe_trace_rescale(self._h, _ptr(c_re), _ptr(c_im), n, nlimbs, batch, arr, _stream_ptr(stream)),
              "trace_rescale")
    def trace_product(self, a_re, a_im, b_re, b_im, c_re, c_im, n, nlimbs, batch, inv=None, stream=None):
        self._trace_need((a_re, a_im, b_re, b_im, c_re, c_im), n, nlimbs, batch, "trace_product")
        arr = (ctypes.c_uint64 * nlimbs)(*[int(v) for v in inv[:nlimbs]]) if inv is not None else None
        check(lib.mfhe_trace_product(self._h, _ptr(a_re), _ptr(a_im), _ptr(b_re), _ptr(b_im), _ptr(c_re), _ptr(c_im),
                                     n, nlimbs, batch, arr, _stream_ptr(stream)), "trace_product")
    def xy_dft(self, src, dst, lanes, stream=None):
        check(lib.mfhe_xy_dft(self._h, _ptr(src), _ptr(dst), lanes, _stream_ptr(stream)), "xy_dft"); return dst
    def xy_idft(self, src, dst, lanes, stream=None):
        check(lib.mfhe_xy_idft(self._h, _ptr(src), _ptr(dst), lanes, _stream_ptr(stream)), "xy_idft"); return dst
    def matrix_to_poly(self, src, dst, stream=None):
        self._sizes("matrix_to_poly", (src, self._mat()), (dst, self._mat()))
        self._call("mfhe_matrix_to_poly", _ptr(src), _ptr(dst), stream=stream); return dst
    def poly_to_matrix(self, src, dst, stream=None):
        self._sizes("poly_to_matrix", (src, self._mat()), (dst, self._mat()))
        self._call("mfhe_poly_to_matrix", _ptr(src), _ptr(dst), stream=stream); return dst
    def reserve_workspace(self): check(lib.mfhe_ctx_reserve_workspace(self._h), "reserve_workspace")
    def encode(self, msg, out_re, out_im, stream=None):
        self._sizes("encode", (msg, self._msg()), (out_re, self._mat()), (out_im, self._mat()))
        self._call("mfhe_encode", _ptr(msg), _ptr(out_re), _ptr(out_im), stream=stream)
    def decode(self, ev_re, ev_im, msg, stream=None):
        self._sizes("decode", (ev_re, self._mat()), (ev_im, self._mat()), (msg, self._msg()))
        self._call("mfhe_decode", _ptr(ev_re), _ptr(ev_im), _ptr(msg), stream=stream); return msg
    def keygen(self, sk, stream=None):
        self._sizes("keygen", (sk, self._sk()))
        self._call("mfhe_keygen", _ptr(sk), stream=stream); return sk
    def encrypt(self, m, sk, ct, stream=None):
        self._sizes("encrypt", (m, self._mat()), (sk, self._sk()), (ct, 2 * self._mat()))
        self._call("mfhe_encrypt", _ptr(m), _ptr(sk), _ptr(ct), stream=stream)
    def encrypt_pair(self, m_re, m_im, sk, ct_re, ct_im, stream=None):
        self._sizes("encrypt_pair", (m_re, self._mat()), (m_im, self._mat()), (sk, self._sk()),
                    (ct_re, 2 * self._mat()), (ct_im, 2 * self._mat()))
        self._call("mfhe_encrypt_pair", _ptr(m_re), _ptr(m_im), _ptr(sk), _ptr(ct_re), _ptr(ct_im), stream=stream)
    def decrypt_to_eval(self, ct, sk, out, stream=None):
        self._sizes("decrypt_to_eval", (ct, 2 * self._mat()), (sk, self._sk()), (out, self._mat()))
        self._call("mfhe_decrypt_to_eval", _ptr(ct), _ptr(sk), _ptr(out), stream=stream); return out
    def decrypt_and_decode(self, ct_re, ct_im, sk, msg, stream=None):
        self._sizes("decrypt_and_decode", (ct_re, 2 * self._mat()), (ct_im, 2 * self._mat()), (sk, self._sk()),
                    (msg, self._msg()))
        self._call("mfhe_decrypt_and_decode", _ptr(ct_re), _ptr(ct_im), _ptr(sk), _ptr(msg), stream=stream); return msg

    # ---- residue sharding across GPUs (BASELINE C4, include/mfhe.h) ----
    def set_limb_shard(self, limb_base: int, limbs_total: int):
        """This context holds limbs [limb_base, limb_base + L) of a limbs_total-modulus parameter set."""
        check(lib.mfhe_ctx_set_limb_shard(self._h, limb_base, limbs_total), "set_limb_shard")

    def decode_sharded(self, ctx_all: "Context", comm: "Comm", mode, ev_re, ev_im, msg, stream=None):
        m = _XCHG[mode] if isinstance(mode, str) else mode
        self._sizes("decode_sharded", (ev_re, self._mat()), (ev_im, self._mat()), (msg, self._msg()))
        check(lib.mfhe_decode_sharded(self._h, ctx_all._h, comm._h, m, _ptr(ev_re), _ptr(ev_im), _ptr(msg),
                                      _stream_ptr(stream)), "decode_sharded")
        return msg

    def decrypt_and_decode_sharded(self, ctx_all: "Context", comm: "Comm", mode, ct_re, ct_im, sk, msg, stream=None):
        m = _XCHG[mode] if isinstance(mode, str) else mode
        self._sizes("decrypt_and_decode_sharded", (ct_re, 2 * self._mat()), (ct_im, 2 * self._mat()),
                    (sk, self._sk()), (msg, self._msg()))
        check(lib.mfhe_decrypt_and_decode_sharded(self._h, ctx_all._h, comm._h, m, _ptr(ct_re), _ptr(ct_im), _ptr(sk),
                                                  _ptr(msg), _stream_ptr(stream)), "decrypt_and_decode_sharded")
        return msg


class PolyPlan:
    """A polynomial evaluation plan (mfhe_poly_plan): the node list of a coefficient vector for one context, input
    level and input scale, and the device table of its constants' residues."""

    def __init__(self, ctx: "Context", coeffs, basis, in_scale, level):
        a = [float(v) for v in coeffs]
        arr = (_dbl * max(len(a), 1))(*a)
        h = _vp()
        check(lib.mfhe_poly_plan_create(ctx.handle, arr, len(a) - 1, basis, float(in_scale), level, ctypes.byref(h)),
              "poly_plan_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def info(self) -> PolyInfo:
        out = PolyInfo()
        check(lib.mfhe_poly_plan_info(self._h, ctypes.byref(out)), "poly_plan_info")
        return out

    def nodes(self) -> list[dict]:
        """Every node as a dict: dst, level, mul_a, mul_b, k_mul, terms [(src, k, coef)], addend_k, addend_coef, scale_in,
        scale_out."""
        out = []
        for i in range(self.info().nnodes):
            n = PolyNode()
            check(lib.mfhe_poly_plan_node(self._h, i, ctypes.byref(n)), "poly_plan_node")
            out.append(dict(dst=n.dst, level=n.level, mul_a=n.mul_a, mul_b=n.mul_b, k_mul=n.k_mul,
                            terms=[(n.term_src[j], n.term_k[j], n.term_coef[j]) for j in range(n.nterms)],
                            addend_k=n.addend_k, addend_coef=n.addend_coef, scale_in=n.scale_in, scale_out=n.scale_out))
        return out

    def constants(self) -> list[int]:
        """The constants as Python integers."""
        out = []
        for i in range(self.info().nconst):
            neg, lo, hi = _int(), ctypes.c_uint64(), ctypes.c_uint64()
            check(lib.mfhe_poly_plan_constant(self._h, i, ctypes.byref(neg), ctypes.byref(lo), ctypes.byref(hi)),
                  "poly_plan_constant")
            v = (hi.value << 64) | lo.value
            out.append(-v if neg.value else v)
        return out

    def table_ptr(self) -> int:
        """Device address of the [nconst][level] residue table (row stride `level` words)."""
        p = _vp()
        check(lib.mfhe_poly_plan_table(self._h, ctypes.byref(p)), "poly_plan_table")
        return p.value

    def close(self):
        if self._h:
            check(lib.mfhe_poly_plan_destroy(self._h), "poly_plan_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fnwt_1d(data, tw, tw_shoup, dmod, dim, coeff_modulus_size, start_modulus_idx=0, batch=1, stream=None):
    """phantom fnwt_1d (ntt/ntt_1d.cu) over raw table pointers; batch polys at once."""
    check(lib.mfhe_fnwt_1d(_ptr(data), tw, tw_shoup, dmod, dim, coeff_modulus_size, start_modulus_idx, batch,
                           _stream_ptr(stream)), "fnwt_1d")


def inwt_1d(data, itw, itw_shoup, dmod, scalar, scalar_shoup, dim, coeff_modulus_size, start_modulus_idx=0, batch=1,
            stream=None):
    check(lib.mfhe_inwt_1d(_ptr(data), itw, itw_shoup, dmod, scalar, scalar_shoup, dim, coeff_modulus_size,
                           start_modulus_idx, batch, _stream_ptr(stream)), "inwt_1d")


# ---- host/device array helpers (uint64 stored in int64 tensors) ----
def galois_elt(step: int, log_n: int) -> int:
    """The Galois element of a slot rotation by `step`: 5^step mod 2N (the inverse of 5 for negative steps)."""
    m = 2 << log_n
    return pow(5, step, m) if step >= 0 else pow(pow(5, -1, m), -step, m)


def galois_conj(log_n: int) -> int:
    """The Galois element of the conjugation: 2N - 1."""
    return (2 << log_n) - 1


def bsgs_plan(steps, n1: int, log_n: int) -> dict:
    """Split the slot rotations `steps` (the diagonals of a matrix; taken mod N/2, duplicates dropped) for a
    baby-step giant-step transform with n1 baby steps: k = a n1 + b, 0 <= b < n1.  Returns the lists Context.lt_apply
    takes and what the caller needs to lay out plaintexts and keys:
      baby_steps / giant_steps   rotations of the steps in use, ascending, entry 0 is 0 (giant steps are multiples of n1)
      baby_elt / giant_elt       their Galois elements (galois_elt), entry 0 is 1
      term_step                  the rotation k of term t, sorted by (giant, baby): plaintext t holds diagonal k,
                                 pre-rotated by -giant_steps[term_giant[t]]
      term_giant / term_baby     indices into giant_steps / baby_steps
      key_steps                  the rotations a Galois key is needed for: every step in use but 0"""
    if n1 < 1:
        raise ValueError("bsgs_plan: n1 < 1")
    nslots = 1 << (log_n - 1)
    ks = sorted({int(k) % nslots for k in steps})
    baby_steps = sorted({0} | {k % n1 for k in ks})
    giant_steps = sorted({0} | {k - k % n1 for k in ks})
    return {
        "baby_steps": baby_steps,
        "giant_steps": giant_steps,
        "baby_elt": [galois_elt(b, log_n) for b in baby_steps],
        "giant_elt": [galois_elt(g, log_n) for g in giant_steps],
        "term_step": ks,
        "term_giant": [giant_steps.index(k - k % n1) for k in ks],
        "term_baby": [baby_steps.index(k % n1) for k in ks],
        "key_steps": sorted({s for s in baby_steps + giant_steps if s}),
    }


def to_device_u64(arr, device="cuda"):
    import numpy as np
    import torch
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host_u64(t):
    import numpy as np
    return t.detach().cpu().numpy().view(np.uint64)
