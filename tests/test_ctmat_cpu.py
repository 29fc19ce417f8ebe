"""CPU checks of the ciphertext matrix product's surface (csrc/ctmat.hip; include/mfhe.h mfhe_ctmat_tensor,
mfhe_ctmat_apply, mfhe_ctmat_reserve): the symbols, the Python methods, and the bytes model of the tiled tensor sum
that tools/ctmat_bench.py exports and DESIGN.md 3.13 states."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _bench_tool():
    spec = importlib.util.spec_from_file_location("ctmat_bench", ROOT / "tools" / "ctmat_bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)   # the tool imports torch and the library in main() only
    return mod


def test_symbols_and_methods(mfhe):
    names = mfhe.declared_symbols()
    for name in ("mfhe_ctmat_tensor", "mfhe_ctmat_apply", "mfhe_ctmat_reserve"):
        assert name in names, name
        assert hasattr(mfhe.lib, name), name
    for method in ("ctmat_tensor", "ctmat_reserve", "ctmat"):
        assert callable(getattr(mfhe.Context, method, None)), method


def test_bytes_model():
    """8 N level npoly (2 k (m ceil(n / TN) + n ceil(m / TM)) + 3 m n): one output of one term is ctmul_tensor's
    8 N level npoly (4 + 3), whatever the tile; a full 2 x 2 tile at 8 terms streams 19 polynomials per output where
    separate dot products stream 35."""
    tool = _bench_tool()
    n, level, npoly = 1 << 16, 11, 4
    for tm, tn in ((2, 2), (2, 4), (4, 2)):
        assert tool.tensor_model_bytes(n, level, npoly, 1, 1, 1, tm, tn) == 8 * n * level * npoly * (4 * 1 + 3)
    unit = 8 * n * level * npoly
    assert tool.tensor_model_bytes(n, level, npoly, 4, 4, 8, 2, 2) == unit * 16 * 19
    assert tool.tensor_model_bytes(n, level, npoly, 4, 4, 8, 1, 1) == unit * 16 * 35
    # edges: 3 x 2 outputs in 2 x 2 tiles read A's 3 rows once (one tile column) and B's 2 columns twice (two tile rows)
    assert tool.tensor_model_bytes(n, level, npoly, 3, 2, 7, 2, 2) == unit * (2 * 7 * (3 * 1 + 2 * 2) + 3 * 6)
