// bconv.hpp -- launchers of the RNS basis conversion kernels (bconv.hip).
#pragma once
#include "ks_host.hpp"
#include "mfhe_ctx.hpp"

namespace mfhe {

// One destination limb range of a conversion: `count` limbs from context limb `limb`, written to output rows
// row .. row + count - 1, with the cached device table of (source range, this range).
struct BconvRange {
    const uint64_t* tab;
    int limb, row, count, pad;
};

// Device table of one (source range of ns limbs, destination range of nd limbs), u64 words:
//   [ns][4]       s_i, (S/s_i)^-1 mod s_i, its Shoup companion, bits of 1/s_i as f64
//   [nd][4 + ns]  (-S) mod d_j, S^-1 mod d_j, its Shoup companion, 0, then c_ij = (S/s_i) mod d_j for i < ns
constexpr int kBconvSrcWords = 4;
constexpr int kBconvDstHead = 4;

// Kernel arguments.  Strides, ncoeff and total are in units of V words (V = 1 scalar, V = 2 the 16-byte form).
struct BconvArgs {
    const void* in;
    void* out;
    uint64_t in_stride, out_stride;   // per polynomial
    uint64_t total, ncoeff;           // threads of the launch; elements per row
    int lg;                           // log2 ncoeff, or -1
    int ns, src_row;                  // source residues: rows src_row .. src_row + ns - 1 of `in`
    int copy_row;                     // >= 0: the source residues are also stored to output rows copy_row + i
    int nr;                           // destination ranges in use
    BconvRange r[3];
    const uint64_t* dmod;             // [L][3] {q, floor(2^128 / q) low, high}
};

enum { kBconvFast = 0, kBconvCentered = 1, kBconvModDown = 2 };

// Cached device table of a (source, destination) pair of limb ranges; built and uploaded on first use.
int bconv_table(mfhe_ctx* c, int src_start, int src_count, int dst_start, int dst_count, const uint64_t** tab);

// One launch: the conversion of `a` (strides and ncoeff given in words; the 16-byte form is chosen here when
// ncoeff and both strides are even and both buffers 16-byte aligned).  kernel_mode: kBconv*.
int launch_bconv(BconvArgs a, size_t npoly, int kernel_mode, hipStream_t st);

// ---- shared with keyswitch.hip and slot.hip ----
// One launch: dst[p][w] = src[p][w] for w < words, the npoly blocks src_stride / dst_stride words apart.
int launch_copy_rows(const uint64_t* src, size_t src_stride, uint64_t* dst, size_t dst_stride, size_t npoly,
                     size_t words, hipStream_t st);

// The destination ranges of a ModUp of digit [ds, ds + dc) at `level`: below the digit, above it, the special limbs
// (the non-empty ones), each with its first context limb, its first output row and its count.
struct ModUpPlan {
    int nr = 0;
    int limb[3], row[3], count[3];
};
int check_modup(const mfhe_ctx* c, int level, int ds, int dc, int sp, int nsp, ModUpPlan& pl);
int ntt_modup_tables(mfhe_ctx* c, int digit_start, int digit_count, const ModUpPlan& pl, const uint64_t* tab[3]);

// Bodies of mfhe_ntt_modup / mfhe_ntt_moddown (arguments already checked, tables already built) with the scratch base
// as an argument.  ntt_modup_body: scratch of npoly * (level + nspecial) * N words.  ntt_moddown_center: scratch of
// npoly * (keep_count + drop_count) * N words; *cen = the centred conversion of the dropped rows in the evaluation
// domain, dense [npoly][keep_count][N] inside scratch.  launch_sub_scale: ModDown's tail,
// out = (in - cen) P^-1 (+ d_add, same layout as out, when not null) on the kept rows.
int ntt_modup_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                   size_t npoly, int digit_start, int digit_count, const ModUpPlan& pl, const uint64_t* const tab[3],
                   uint64_t* scratch, hipStream_t st);
int ntt_moddown_center(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, size_t npoly, int keep_count,
                       int drop_start, int drop_count, const uint64_t* tab, uint64_t* scratch, const uint64_t** cen,
                       hipStream_t st);
int launch_sub_scale(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, const uint64_t* cen, size_t cen_stride,
                     uint64_t* d_out, size_t out_stride, const uint64_t* d_add, size_t npoly, int keep_count,
                     int drop_count, const uint64_t* tab, hipStream_t st);

}  // namespace mfhe
