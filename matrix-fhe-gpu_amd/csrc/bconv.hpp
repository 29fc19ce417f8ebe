// bconv.hpp -- launchers of the RNS basis conversion kernels (bconv.hip).
#pragma once
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

}  // namespace mfhe
