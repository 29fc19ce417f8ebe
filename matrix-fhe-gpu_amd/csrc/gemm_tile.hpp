// gemm_tile.hpp -- the tile shape and the B / C address map shared by the VALU modular GEMM (wcrt_gemm.hip) and
// the complex GEMMs (cdft.hip): LDS-tiled 64 x 64 output tiles, 256 threads, 4 x 4 outputs per thread.  B and C
// are addressed through a (k|m, pos) -> offset map  k*sK + (pos >> log_n)*sY + (pos & (n-1)) so the same kernel
// serves matrix-major and poly-major layouts (HE.cu:744-746, 773, 778).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfhe {

constexpr int TM = 64, TP = 64, TK = 16, NTH = 256;

__device__ __forceinline__ uint64_t b_off(uint64_t k, uint32_t p, uint64_t sK, uint64_t sY, int log_n) {
    return k * sK + (uint64_t)(p >> log_n) * sY + (p & ((1u << log_n) - 1));
}

}  // namespace mfhe
