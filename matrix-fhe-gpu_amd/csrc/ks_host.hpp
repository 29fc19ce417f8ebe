// ks_host.hpp -- the host arithmetic of the key switch and its drivers (keyswitch.hip, galois.hip, lintrans.hip,
// ctmul.hip, ctmat.hip, bconv.hip): spans and overlaps of strided buffers, the key switch's block of the workspace and
// the launch geometry of the row kernels.  Plain integer code with no HIP dependency that returns values and sets no
// error (tests/cpp/ks_host_main.cpp includes this file with a host compiler alone).
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace mfhe {

// digits of a call at `level`: runs of alpha consecutive Q limbs
inline int ks_beta(int level, int alpha) { return (level + alpha - 1) / alpha; }

// words spanned by npoly blocks of `words` words, `stride` apart
inline size_t ks_span(size_t npoly, size_t stride, size_t words) { return npoly ? (npoly - 1) * stride + words : 0; }
// whether two ranges of na and nb words share a word (an empty range overlaps nothing)
inline bool ks_ranges_overlap(const uint64_t* a, size_t na, const uint64_t* b, size_t nb) {
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    return na && nb && ua < ub + nb * 8 && ub < ua + na * 8;
}

// A range of device words, for the overlap checks.
struct KsRange {
    const uint64_t* p;
    size_t words;
};
enum { kKsNoOverlap = 0, kKsInputOverlap = 1, kKsOutputOverlap = 2 };
// no output may overlap an input or another output; the first offence, output by output
inline int ks_find_overlap(const KsRange* in, size_t nin, const KsRange* out, size_t nout) {
    for (size_t k = 0; k < nout; ++k) {
        for (size_t i = 0; i < nin; ++i)
            if (ks_ranges_overlap(in[i].p, in[i].words, out[k].p, out[k].words)) return kKsInputOverlap;
        for (size_t j = 0; j < k; ++j)
            if (ks_ranges_overlap(out[j].p, out[j].words, out[k].p, out[k].words)) return kKsOutputOverlap;
    }
    return kKsNoOverlap;
}

// words of the key switch's block of the workspace: raised digits, acc, the inner calls' scratch (the ModDown of both
// components at once: 2 npoly polynomials)
inline size_t ks_ws_words(size_t npoly, int beta, size_t rows, size_t N) { return ((size_t)beta + 4) * npoly * rows * N; }

// The key switch's block, at word 0 of the context workspace: offsets in words of raised [beta][npoly][rows][N],
// acc [npoly][2][rows][N] and the scratch of 2 npoly rows N words; `end` is where a driver's own buffers start.
struct KsWs {
    size_t raised, acc, scratch, end;
};
inline KsWs ks_ws(size_t npoly, int beta, size_t rows, size_t N) {
    const size_t pw = rows * N;   // one raised polynomial
    KsWs w;
    w.raised = 0;
    w.acc = w.raised + (size_t)beta * npoly * pw;
    w.scratch = w.acc + 2 * npoly * pw;
    w.end = w.scratch + 2 * npoly * pw;
    return w;
}

// The row kernels give one thread one element of a row: `block` threads (a whole number of waves, 256 from 256
// elements on) and bx blocks along x cover the ncoeff elements.
struct KsRowGrid {
    uint32_t block;
    uint64_t bx;
};
inline KsRowGrid ks_row_grid(uint64_t ncoeff) {
    KsRowGrid g;
    g.block = ncoeff >= 256 ? 256 : (uint32_t)((ncoeff + 63) / 64 * 64);
    g.bx = g.block ? (ncoeff + g.block - 1) / g.block : 0;
    return g;
}

// The 16-byte form of a row kernel: taken when every stride (the row length among them) is even and every buffer
// 16-byte aligned, and then the strides are halved in place, to units of two words.
inline bool ks_wide(std::initializer_list<uint64_t*> strides, std::initializer_list<const void*> ptrs) {
    uint64_t odd = 0;
    uintptr_t bits = 0;
    for (const uint64_t* s : strides) odd |= *s;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    if (odd % 2 || (bits & 15)) return false;
    for (uint64_t* s : strides) *s /= 2;
    return true;
}

// A thread keeps its slice of the key (of the plaintexts) across `prun` of the n polynomials: as long a run as still
// leaves about 4096 workgroups (16 per CU) in a grid of bx x rows x runs, never shorter than min_run (or the batch),
// and long enough for grid z <= 65535.  runs = ceil(n / prun).
struct KsRuns {
    uint64_t prun, runs;
};
inline KsRuns ks_runs(uint64_t n, uint64_t bx, uint64_t rows, uint64_t min_run) {
    KsRuns r{0, 0};
    if (n == 0 || bx * rows == 0) return r;
    r.runs = 4096 / (bx * rows);
    r.runs = r.runs < 1 ? 1 : r.runs;
    r.prun = (n + r.runs - 1) / r.runs;
    if (r.prun < min_run) r.prun = n < min_run ? n : min_run;
    if ((n + r.prun - 1) / r.prun > 65535) r.prun = (n + 65534) / 65535;   // grid z limit
    r.runs = (n + r.prun - 1) / r.prun;
    return r;
}

// `total` (polynomial, row) pairs folded over grid y and z so that gy <= 65535; the caller rejects gz > 65535
struct KsFold {
    uint64_t gy, gz;
};
inline KsFold ks_fold(uint64_t total) {
    KsFold f;
    f.gy = total < 65535 ? total : 65535;
    f.gz = f.gy ? (total + f.gy - 1) / f.gy : 0;
    return f;
}

}  // namespace mfhe
