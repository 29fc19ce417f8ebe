// keyswitch.hpp -- launchers of the hybrid key-switching kernels (keyswitch.hip).
#pragma once
#include "mfhe_ctx.hpp"

namespace mfhe {

// Geometry of a key switch: Q limbs [0, level) of a key made at key_level, the K = nspecial special limbs from
// special_start (>= key_level).  A (level + K)-row block has modulus limb r on row r < level, else limb
// special_start + r - level; its key row is r, else key_level + r - level.
struct KsGeom {
    int level, key_level, special_start, nspecial;
    int rows() const { return level + nspecial; }
    int key_rows() const { return key_level + nspecial; }
};

// Kernel arguments of the inner product.  Strides and ncoeff in units of V words (V = 1 scalar, V = 2 the 16-byte
// form).  raised [ndigits][npoly][rows][ncoeff], ksk [ndigits][2][key_rows][ncoeff] dense, acc [npoly][2][rows][ncoeff].
struct KsipArgs {
    const void* raised;
    const void* ksk;
    void* acc;
    uint64_t digit_stride, poly_stride, acc_stride;
    uint64_t ncoeff;       // elements per row
    uint64_t npoly, prun;  // polynomials of the batch; polynomials one thread walks (grid z = ceil(npoly / prun))
    int ndigits;
    KsGeom g;
};

// One launch: acc[p][c][r] = sum_j raised[j][p][r] ksk[j][c][keyrow(r)] mod q_r.  Strides and ncoeff given in words;
// the 16-byte form is chosen here when ncoeff and every stride are even and the three buffers 16-byte aligned.
int launch_ksk_inner_product(mfhe_ctx* c, KsipArgs a, hipStream_t st);

}  // namespace mfhe
