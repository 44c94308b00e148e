// rs_correct.hip -- correction per byte column of up to two damaged rows
// (rsgpu_correct_blocks) for gfx950.
//
// With s the syndromes of a byte column (stored ^ recomputed parity) and h_r
// what a unit change of row r adds to them (column r of the matrix for a data
// row, the unit vector of p for parity row k + p; include/rsgpu.h), a column
// is corrected in the one row r with s = x h_r, or, with t == 2 and no such
// row, in the one pair {a, b} with s = x h_a + y h_b, x and y non-zero.
//
// k_correct_compare is k_repair_compare (rs_kernels.hip) in its COLUMNS mode:
// the encode dispatch has written the parity of the sources to `calc`, a
// thread ORs the syndromes of 16 columns per 16-byte load and walks them only
// when one is bad, trying the one-row explanation (rs_lane.h scrub_locate_row)
// and correcting where it holds.  What differs is the walk, which is uniform
// over the wave, so that the columns the one-row explanation leaves (t == 2)
// can go to the wave as a whole, one at a time as in k_locate_span: lane p
// holds s_p, and the candidate pairs are spread over the lanes --
//   two parity rows   the column's only non-zero syndromes are s_p and s_q:
//                     read off the ballot, no search
//   a data row r and  a lane per r.  p >= 1: x = s_0 / c[0][r], and s_q = c[q][r]
//   a parity row      x fails at exactly one q, which is p.  p == 0: x = s_1 /
//                     c[1][r] holds at every q >= 2
//   two data rows     a lane per b, every a < b in turn.  Coordinates 0 and 1
//                     give x = u_b / det, y = u_a / det with u_r = s_0 c[1][r] ^
//                     s_1 c[0][r] and det = c[0][a] c[1][b] ^ c[1][a] c[0][b],
//                     which is non-zero for a locatable matrix; coordinate 2
//                     is tested in the form (s_2 c[0][a]) c[1][b] ^ (s_2 c[1][a])
//                     c[0][b] ^ c[2][a] u_b ^ c[2][b] u_a = 0: the logarithms of
//                     the eight factors are laid out per row and column before
//                     the search, so a pair costs one 8-byte read that is the
//                     same in every lane and four table reads that do not
//                     depend on each other, and 255 of 256 pairs end there;
//                     the rest is verified coordinate by coordinate
// Every pair of the (k + e)(k + e - 1) / 2 is covered by exactly one of the
// three; matches are counted, up to two, and the column is written when the
// count is one.  The tables are read at lane-dependent indices, which
// constant memory would serialise: each wave keeps them in LDS, with the
// logarithms of rows 0 to 2 of the matrix, filled when it meets its first
// such column, so a wave of clean columns pays nothing for them.  Writing in
// place is safe as in
// k_repair_compare: a column is read and written by its wave only, and `calc`
// holds the parity of the sources as they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rs_pairs.h"
#include "rs_span.h"

namespace rsgpu {

static_assert(sizeof(CorrectFold) == sizeof(rsgpu_correct_report) && sizeof(CorrectFold) == 32 &&
                  offsetof(rsgpu_correct_report, status) == offsetof(CorrectFold, hi1) &&
                  offsetof(rsgpu_correct_report, two_row_columns) == offsetof(CorrectFold, two),
              "the fold lives in the report");

namespace {

constexpr int kCorThreads = 256, kCorWaves = kCorThreads / 64;

alignas(16) __device__ const GfTables kCorGf = make_gf_tables();

// What a wave keeps in LDS for its pair searches (rs_pairs.h: the logarithms
// as the search keeps them, kLogZero, and CorRow, what it keeps of a data row
// per column)
struct CorWave {
    uint8_t log[256];
    uint8_t ex[2 * kLogZero + 4];
    uint8_t l0[256], l1[256], c2[256];  // of the matrix: log c[0][r], log c[1][r] (never 0), c[2][r]
    CorRow row[256];
    uint8_t syn[64];  // the column's syndromes
};

__device__ __forceinline__ unsigned cor_log(const CorWave& w, uint8_t v) { return v ? w.log[v] : kLogZero; }

// a b and a / b (b != 0) on the wave's tables
__device__ __forceinline__ uint8_t cor_mul(const CorWave& w, uint8_t a, uint8_t b)
{
    return w.ex[cor_log(w, a) + cor_log(w, b)];
}

__device__ __forceinline__ uint8_t cor_div(const CorWave& w, uint8_t a, uint8_t b)
{
    return a ? w.ex[w.log[a] + 255 - w.log[b]] : 0;
}

// The wave's tables: the field's, and of rows 0 to 2 of the matrix.
__device__ __forceinline__ void cor_tables(CorWave& w, const uint8_t* coef, int k, int lane)
{
    for (int i = lane; i < 256; i += 64)
        w.log[i] = kCorGf.log[i];
    for (int i = lane; i < (int)sizeof w.ex; i += 64)
        w.ex[i] = i < 510 ? kCorGf.exp[i] : 0;
    for (int r = lane; r < k; r += 64) {
        w.l0[r] = kCorGf.log[coef[r]];
        w.l1[r] = kCorGf.log[coef[k + r]];
        w.c2[r] = coef[2 * k + r];
    }
    // what a lane wrote is read by the other lanes of the wave from here on
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// what a lane has counted
struct CorLane {
    unsigned long long bad, rep, two;
    unsigned hi1, lo1;
};

// Byte column i of a block, as scrub_column of rs_kernels.hip in the repair's
// COLUMNS mode: counted when bad, corrected and folded when one row explains
// it.  True when it is bad and no row explains it.
__device__ __forceinline__ bool correct_one_row(const CorrectCmpArgs& a, const uint8_t* calc, uint8_t* src,
                                                uint8_t* par, long long i, CorLane& c)
{
    int nz = 0, p0 = 0;
    uint8_t s0 = 0, s1 = 0;
    for (int p = 0; p < a.e; ++p) {
        const uint8_t s = calc[(size_t)p * a.pitch + i] ^ par[(size_t)p * a.pitch + i];
        s0 = p == 0 ? s : s0;
        s1 = p == 1 ? s : s1;
        if (s) {
            ++nz;
            p0 = p;
        }
    }
    if (!nz)
        return false;
    ++c.bad;
    const int row = scrub_locate_row(a.k, a.e, a.rowtab, a.coef, kCorGf, s0, s1, nz, p0, [&](int p) {
        return (uint8_t)(calc[(size_t)p * a.pitch + i] ^ par[(size_t)p * a.pitch + i]);
    });
    if (row < 0)
        return true;
    if (row < a.k)
        src[(size_t)row * a.pitch + i] ^= loc_div(kCorGf, s0, a.coef[row]);
    else  // the stored byte becomes the computed one
        par[(size_t)p0 * a.pitch + i] = calc[(size_t)p0 * a.pitch + i];
    ++c.rep;
    c.hi1 = max(c.hi1, (unsigned)row + 1);
    c.lo1 = max(c.lo1, kScrubBias - (unsigned)row);
    return false;
}

// Byte column i of a block that no single row explains, the whole wave on it
// under uniform control (5 <= e <= 64): the search described at the top, and
// the correction by the lane that holds the only match, which returns true.
__device__ __forceinline__ bool correct_two_rows(const uint8_t* calc, uint8_t* src, uint8_t* par, const uint8_t* coef,
                                                 long long pitch, int k, int e, long long i, CorWave& w, int lane)
{
    CorPairs c{};
    uint8_t s = 0;
    if (lane < e)
        s = calc[(size_t)lane * pitch + i] ^ par[(size_t)lane * pitch + i];
    const uint8_t s0 = lane_byte(s, 0), s1 = lane_byte(s, 1), s2 = lane_byte(s, 2);
    const unsigned ls0 = cor_log(w, s0), ls1 = cor_log(w, s1), ls2 = cor_log(w, s2);
    w.syn[lane] = s;
    for (int r = lane; r < k; r += 64) {
        const unsigned l0 = w.l0[r], l1 = w.l1[r];
        CorRow row;
        row.a0 = (uint16_t)cor_log_mul(ls2, l0);
        row.a1 = (uint16_t)cor_log_mul(ls2, l1);
        row.c2 = (uint16_t)cor_log(w, w.c2[r]);
        row.u = (uint16_t)cor_log(w, w.ex[ls0 + l1] ^ w.ex[ls1 + l0]);
        w.row[r] = row;
    }
    // what a lane wrote is read by the other lanes of the wave from here on
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    // two parity rows
    const unsigned long long nzm = __ballot(s != 0);
    if (__popcll(nzm) == 2 && lane == 0) {
        const int p = __ffsll(nzm) - 1, q = 63 - __clzll(nzm);
        pair_found(c, k + p, k + q, w.syn[p], w.syn[q]);
    }

    // a data row and a parity row: syndromes 1 and 2 from the wave's tables,
    // the others, for the few rows that get there, from the matrix
    for (int r = lane; r < k; r += 64) {
        const unsigned l0 = w.l0[r], l1 = w.l1[r], l2 = cor_log(w, w.c2[r]);
        if (s0) {  // parity row k + p, p >= 1
            const unsigned lx = cor_log_mul(ls0, 255 - l0);
            const uint8_t x = w.ex[lx];
            int miss = 0, p = 0;
            if (w.syn[1] != w.ex[l1 + lx]) {
                ++miss;
                p = 1;
            }
            if (w.syn[2] != w.ex[l2 + lx]) {
                ++miss;
                p = 2;
            }
            for (int q = 3; q < e && miss < 2; ++q)
                if (w.syn[q] != cor_mul(w, coef[(size_t)q * k + r], x)) {
                    ++miss;
                    p = q;
                }
            if (miss == 1)
                pair_found(c, r, k + p, x, w.syn[p] ^ cor_mul(w, coef[(size_t)p * k + r], x));
        }
        if (s1) {  // parity row k
            const unsigned lx = cor_log_mul(ls1, 255 - l1);
            const uint8_t x = w.ex[lx];
            bool ok = w.syn[2] == w.ex[l2 + lx];
            for (int q = 3; q < e && ok; ++q)
                ok = w.syn[q] == cor_mul(w, coef[(size_t)q * k + r], x);
            const uint8_t y = s0 ^ w.ex[l0 + lx];
            if (ok && y)
                pair_found(c, r, k, x, y);
        }
    }

    // two data rows: a lane per rb, every ra below it
    for (int base = 0; base < k; base += 64) {
        const int rb = base + lane;
        if (rb < k) {
            const unsigned lb0 = w.l0[rb], lb1 = w.l1[rb];
            const CorRow b = w.row[rb];
            for (int ra = 0; ra < rb && b.u != kLogZero; ++ra) {
                const CorRow a = w.row[ra];
                // det s_2 ^ c[2][ra] u_rb ^ c[2][rb] u_ra
                if ((w.ex[a.a0 + lb1] ^ w.ex[a.a1 + lb0] ^ w.ex[a.c2 + b.u] ^ w.ex[b.c2 + a.u]) != 0 ||
                    a.u == kLogZero)
                    continue;
                const uint8_t det = w.ex[w.l0[ra] + lb1] ^ w.ex[w.l1[ra] + lb0];
                if (!det)
                    continue;
                const uint8_t x = cor_div(w, w.ex[b.u], det), y = cor_div(w, w.ex[a.u], det);
                bool ok = true;
                for (int p = 3; p < e && ok; ++p)
                    ok = w.syn[p] ==
                         (cor_mul(w, coef[(size_t)p * k + ra], x) ^ cor_mul(w, coef[(size_t)p * k + rb], y));
                if (ok)
                    pair_found(c, ra, rb, x, y);
            }
        }
        // two matches: the verdict is in
        if (__ballot(c.cnt >= 2) || __popcll(__ballot(c.cnt != 0)) >= 2)
            break;
    }

    const bool several = __ballot(c.cnt >= 2) != 0;
    const int holders = __popcll(__ballot(c.cnt == 1));
    const bool mine = !several && holders == 1 && c.cnt == 1;
    if (mine) {
        if (c.ra < k)
            src[(size_t)c.ra * pitch + i] ^= c.xa;
        else
            par[(size_t)(c.ra - k) * pitch + i] ^= c.xa;
        if (c.rb < k)
            src[(size_t)c.rb * pitch + i] ^= c.xb;
        else
            par[(size_t)(c.rb - k) * pitch + i] ^= c.xb;
    }
    // the next column's syndromes overwrite what the lanes still read here
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return mine;
}

// The columns the lanes of a wave have left (`pend`: bit j of a lane is
// column col + j of that lane), one after the other, the whole wave on each.
__device__ __forceinline__ void correct_pending(const CorrectCmpArgs& a, const uint8_t* calc, uint8_t* src,
                                                uint8_t* par, long long col, unsigned pend, CorWave& w, bool& tables,
                                                int lane, CorLane& c)
{
    unsigned long long todo = __ballot(pend != 0);
    if (todo && !tables) {
        cor_tables(w, a.coef, a.k, lane);
        tables = true;
    }
    while (todo) {
        const int from = __ffsll(todo) - 1;
        todo &= todo - 1;
        unsigned m = (unsigned)__builtin_amdgcn_readlane((int)pend, from);
        const long long col0 = ((long long)__builtin_amdgcn_readlane((int)(col >> 32), from) << 32) |
                               (unsigned)__builtin_amdgcn_readlane((int)col, from);
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            if (correct_two_rows(calc, src, par, a.coef, a.pitch, a.k, a.e, col0 + j, w, lane)) {
                ++c.rep;
                ++c.two;
                // no common row of the block's corrected columns
                c.hi1 = kScrubNoRow;
                c.lo1 = kScrubNoRow;
            }
        }
    }
}

// A thread owns units of the row: the 16-byte groups of 16-byte aligned rows,
// then the bytes they leave (every byte of unaligned rows).  A wave walks its
// units under uniform control.
__global__ __launch_bounds__(kCorThreads) void k_correct_compare(CorrectCmpArgs a)
{
    __shared__ CorWave cw[kCorWaves];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
    const uint8_t* calc = a.calc + b * a.e * a.pitch;
    uint8_t* src = a.src + b * a.k * a.pitch;
    uint8_t* par = a.par + b * a.e * a.pitch;
    CorLane c{};
    bool tables = false;  // the wave's copy in cw is filled
    // the wave's first thread of the grid: the walk is the same in all its lanes
    const long long first = (long long)blockIdx.x * kCorThreads + wave * 64;
    const long long nthr = (long long)gridDim.x * kCorThreads;
    const bool vec = ((reinterpret_cast<uintptr_t>(calc) | reinterpret_cast<uintptr_t>(par) |
                       (uintptr_t)a.pitch) & 15) == 0;
    const long long groups = vec ? a.len >> 4 : 0, units = groups + (a.len - groups * 16);
    for (long long base = first; base < units; base += nthr) {
        const long long unit = base + lane;
        const long long col = unit < groups ? unit * 16 : unit - groups + groups * 16;
        unsigned pend = 0;
        if (unit < groups) {
            uint4 any = make_uint4(0, 0, 0, 0);
            for (int p = 0; p < a.e; ++p) {
                const uint4 x = *reinterpret_cast<const uint4*>(calc + (size_t)p * a.pitch + col);
                const uint4 y = *reinterpret_cast<const uint4*>(par + (size_t)p * a.pitch + col);
                any.x |= x.x ^ y.x;
                any.y |= x.y ^ y.y;
                any.z |= x.z ^ y.z;
                any.w |= x.w ^ y.w;
            }
            if ((any.x | any.y | any.z | any.w) != 0)
                for (int j = 0; j < 16; ++j)
                    if (correct_one_row(a, calc, src, par, col + j, c))
                        pend |= 1u << j;
        } else if (unit < units && correct_one_row(a, calc, src, par, col, c)) {
            pend = 1;
        }
        if (a.t == 2)
            correct_pending(a, calc, src, par, col, pend, cw[wave], tables, lane, c);
    }
    for (int off = 32; off > 0; off >>= 1) {
        c.bad += __shfl_down(c.bad, off, 64);
        c.rep += __shfl_down(c.rep, off, 64);
        c.two += __shfl_down(c.two, off, 64);
        c.hi1 = max(c.hi1, (unsigned)__shfl_down((int)c.hi1, off, 64));
        c.lo1 = max(c.lo1, (unsigned)__shfl_down((int)c.lo1, off, 64));
    }
    if (lane == 0 && c.bad) {
        CorrectFold* f = &a.fold[b];
        atomicAdd(&f->bad, c.bad);
        if (c.rep)
            atomicAdd(&f->rep, c.rep);
        if (c.two)
            atomicAdd(&f->two, c.two);
        if (c.hi1) {
            atomicMax(&f->hi1, c.hi1);
            atomicMax(&f->lo1, c.lo1);
        }
    }
}

// The fold of every block into its report: the status by the counts, `row`
// where the maxima name one row (fold_one_row: no two-row correction then).
__global__ __launch_bounds__(256) void k_correct_finalise(void* report, long long blocks)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= blocks)
        return;
    const CorrectFold f = static_cast<const CorrectFold*>(report)[b];
    rsgpu_correct_report r;
    r.bad_columns = f.bad;
    r.corrected_columns = f.rep;
    r.two_row_columns = f.two;
    r.status = f.bad == 0       ? RSGPU_REPAIR_CLEAN
               : f.rep == f.bad ? RSGPU_REPAIR_REPAIRED
               : f.rep == 0     ? RSGPU_REPAIR_DAMAGED
                                : RSGPU_REPAIR_PARTIAL;
    r.row = (f.bad != 0 && fold_one_row(f)) ? (int)f.hi1 - 1 : -1;
    static_cast<rsgpu_correct_report*>(report)[b] = r;
}

}  // namespace

hipError_t launch_correct_compare(const CorrectCmpArgs& a, hipStream_t st)
{
    if (a.blocks <= 0 || a.blocks > (long long)kMaxGridBlocks || a.len <= 0 || a.pitch < a.len || a.k <= 0 ||
        a.k + a.e > RSGPU_MAX_SOURCES || !a.src || !a.par || !a.calc || !a.fold || !a.rowtab || !a.coef ||
        !((a.t == 1 && a.e >= 3) || (a.t == 2 && a.e >= 5 && a.e <= 64)))
        return hipErrorInvalidValue;
    // a thread per unit of the kernel's walk, no workgroup without one
    const bool vec = (((uintptr_t)a.calc | (uintptr_t)a.par | (uintptr_t)a.pitch) & 15) == 0;
    const long long units = vec ? a.len / 16 + a.len % 16 : a.len;
    const long long gx = std::min<long long>((units + kCorThreads - 1) / kCorThreads, 1024);
    hipLaunchKernelGGL(k_correct_compare, dim3((unsigned)gx, (unsigned)a.blocks), dim3(kCorThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_correct_finalise(void* report, long long blocks, hipStream_t st)
{
    hipLaunchKernelGGL(k_correct_finalise, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, report, blocks);
    return hipGetLastError();
}

}  // namespace rsgpu
