// keyswitch.hpp -- launchers of the hybrid key-switching kernels (keyswitch.hip).
#pragma once
#include <vector>

#include "bconv.hpp"
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
    uint32_t galois_elt;   // the gathered instantiations alone read these two: the Galois element (0: no gather) and
    int log_n;             // log2 of the row in words, whatever V
};

// One launch: acc[p][c][r] = sum_j raised[j][p][r] ksk[j][c][keyrow(r)] mod q_r.  Strides and ncoeff given in words;
// the 16-byte form is chosen here when ncoeff and every stride are even and the three buffers 16-byte aligned.
// a.galois_elt != 0: the raised digits are read through the gather of that Galois element (galois.hpp),
// raised[j][p][r][pi_g(i)]; ncoeff must then be a power of two and galois_elt odd and below 2 ncoeff.
int launch_ksk_inner_product(mfhe_ctx* c, KsipArgs a, hipStream_t st);

// ---- shared with galois.hip ----
// Argument checks (nothing here touches the device).
int ks_check_ctx(const mfhe_ctx* c);
int ks_check_geom(const mfhe_ctx* c, const KsGeom& g, const char* what);
int ks_check_galois(const mfhe_ctx* c, int galois_elt, const char* what);
// words spanned by npoly blocks of `words` words, `stride` apart
size_t ks_span(size_t npoly, size_t stride, size_t words);
bool ks_ranges_overlap(const uint64_t* a, size_t na, const uint64_t* b, size_t nb);
// words of the key switch's block of the workspace: raised digits, acc, the inner calls' scratch
size_t ks_ws_words(size_t npoly, int beta, size_t rows, size_t N);

// the tables of one key switch geometry: per digit the ModUp plan with its tables, and ModDown's
struct KsTables {
    std::vector<ModUpPlan> plan;
    std::vector<const uint64_t*> tab;   // [beta][3]
    const uint64_t* down = nullptr;
    int beta = 0;
};
int ks_tables(mfhe_ctx* c, const KsGeom& g, int alpha, KsTables& t);

// ---- shared with lintrans.hip ----
// [key_level] P mod q_r on the device, cached per (key_level, special range); built and uploaded on first use
int ksk_pmod_table(mfhe_ctx* c, int key_level, int sp, int nsp, const uint64_t** tab);
// galois.hip: ModUp of every digit of d_in into raised [beta][npoly][rows][N] (strides in words); scratch: npoly rows N
// words
int raise_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* raised, size_t digit_stride,
               size_t poly_stride, size_t npoly, const KsGeom& g, int alpha, const KsTables& t, uint64_t* scratch,
               hipStream_t st);

}  // namespace mfhe
