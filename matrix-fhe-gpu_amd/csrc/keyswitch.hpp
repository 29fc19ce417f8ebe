// keyswitch.hpp -- launchers of the hybrid key-switching kernels and the host pipeline its drivers share
// (keyswitch.hip).
#pragma once
#include <string>
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

// ---- shared with the drivers on the key switch's layout (galois.hip, lintrans.hip, ctmul.hip, ctmat.hip) ----
// Argument checks (nothing here touches the device); ks_host.hpp has their arithmetic.
int ks_check_ctx(const mfhe_ctx* c);
int ks_check_geom(const mfhe_ctx* c, const KsGeom& g, const char* what);
// alpha >= 1, then ks_check_geom
int ks_check_digits(const mfhe_ctx* c, int alpha, const KsGeom& g, const char* what);
int ks_check_galois(const mfhe_ctx* c, int galois_elt, const char* what);
// no output may overlap an input or another output (ks_find_overlap as an error under the entry point's name)
int ks_check_overlap(const std::string& w, const KsRange* in, size_t nin, const KsRange* out, size_t nout);
inline int ks_check_overlap(const std::string& w, std::initializer_list<KsRange> in,
                            std::initializer_list<KsRange> out) {
    return ks_check_overlap(w, in.begin(), in.size(), out.begin(), out.size());
}

// The tables of one key switch geometry: per digit the ModUp plan with its tables, and ModDown's; on request the
// rescale's (limb level - 1 -> [0, level - 1)) and [key_level] P mod q_r (ksk_pmod_table).
struct KsTables {
    std::vector<ModUpPlan> plan;
    std::vector<const uint64_t*> tab;   // [beta][3]
    const uint64_t *down = nullptr, *rescale = nullptr, *pmod = nullptr;
    int beta = 0;
};
enum { kKsRescale = 1, kKsPmod = 2 };
// Everything a driver needs before its first launch, the same from its reserve call and from the call itself: the
// tables of (g, alpha), those of `extra` (kKs* bits), and the context workspace grown to ws_words words.
int ks_prepare(mfhe_ctx* c, const KsGeom& g, int alpha, int extra, size_t ws_words, KsTables& t);
// the body of mfhe_keyswitch_reserve and mfhe_galois_reserve: checks, then ks_prepare for the key switch's block
int ks_reserve(mfhe_ctx* c, size_t npoly, const KsGeom& g, int alpha, const char* what);
// [key_level] P mod q_r on the device, cached per (key_level, special range); built and uploaded on first use
int ksk_pmod_table(mfhe_ctx* c, int key_level, int sp, int nsp, const uint64_t** tab);

// ---- the pipeline: raise, inner product, ModDown of the pair (arguments checked, ks_prepare done) ----
// raised digits [beta][npoly][rows][N] as a step reads them, strides in words
struct KsRaised {
    const uint64_t* p;
    size_t digit_stride, poly_stride;
};
// the two components of a result, [npoly][level][N] at `stride`; bit k of `add`: component k is added into its output
struct KsOut {
    uint64_t *out0, *out1;
    size_t stride;
    int add;
};
// the raised digits of the key switch's block of the workspace, dense
inline KsRaised ks_ws_raised(const mfhe_ctx* c, size_t npoly, const KsGeom& g) {
    const size_t pw = (size_t)g.rows() * c->N;
    return {(const uint64_t*)c->ws, npoly * pw, pw};
}
// ModUp of every digit of d_in into raised [beta][npoly][rows][N] (strides in words); scratch: npoly rows N words
int raise_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* raised, size_t digit_stride,
               size_t poly_stride, size_t npoly, const KsGeom& g, int alpha, const KsTables& t, uint64_t* scratch,
               hipStream_t st);
// raise_body into ks_ws_raised, with the block's scratch
int ks_raise_ws(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, size_t npoly, const KsGeom& g, int alpha,
                const KsTables& t, hipStream_t st);
// launch_ksk_inner_product of x with d_ksk into d_acc; galois_elt 0: the plain product
int ks_inner_product(mfhe_ctx* c, const KsRaised& x, const uint64_t* d_ksk, uint64_t* d_acc, size_t acc_stride,
                     size_t npoly, int ndigits, const KsGeom& g, uint32_t galois_elt, hipStream_t st);
// ModDown of both components of acc [npoly][2][rows][N] as one batch of 2 npoly polynomials (scratch: 2 npoly rows N
// words), then one tail per component into o
int ks_moddown_pair(mfhe_ctx* c, const uint64_t* acc, uint64_t* scratch, const KsOut& o, size_t npoly, const KsGeom& g,
                    const KsTables& t, hipStream_t st);
// inner product of x into the block's acc, then ks_moddown_pair into o
int ks_apply_raised(mfhe_ctx* c, const KsRaised& x, const uint64_t* d_ksk, const KsOut& o, size_t npoly,
                    const KsGeom& g, const KsTables& t, uint32_t galois_elt, hipStream_t st);
// the key switch of d_in: ks_raise_ws, then ks_apply_raised
int ks_switch_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, const uint64_t* d_ksk, const KsOut& o,
                   size_t npoly, const KsGeom& g, int alpha, const KsTables& t, hipStream_t st);

}  // namespace mfhe
