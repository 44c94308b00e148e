// rs_lane.h -- what the kernels of the scrub family share (rs_kernels.hip's
// scrub and repair, rs_update.hip, rs_degraded.hip, rs_rebuild.hip, rs_locate.hip, rs_correct.hip): the lane's building
// blocks (v_perm multiply, three-way XOR, the 3-3-2 selector split of a dword
// and the table multiply on it, a column of one row), the fold of a wave's bad
// columns into a block's report, the verdict on a finished fold, and the
// launch rules of the column kernels: their grid, the dispatch of the group
// size G (rs_kernels.h lane_group) to a template argument and the LDS their
// tables take.  Internal to librsgpu's .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"

namespace rsgpu {

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

__device__ __forceinline__ uint32_t vperm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// One dword of a column as the three v_perm selector dwords of the 3-3-2
// split: bits 0-2, 3-5 and 6-7 of every byte.
__device__ __forceinline__ void sel_split(uint32_t x, uint32_t& s0, uint32_t& s1, uint32_t& s2)
{
    s0 = x & 0x07070707u;
    s1 = (x >> 3) & 0x07070707u;
    s2 = (x >> 6) & 0x03030303u;
}

// c * x for the dword x of those selectors and the tables (t, tc) of the
// coefficient c (gf256.h perm_tables: words 0-3 and word 4)
__device__ __forceinline__ uint32_t sel_mul(const uint4& t, uint32_t tc, uint32_t s0, uint32_t s1, uint32_t s2)
{
    return xor3(vperm(t.y, t.x, s0), vperm(t.w, t.z, s1), vperm(tc, tc, s2));
}

// Row pointers fetched from memory are generic (flat) pointers; loads through
// them would be flat_load (out-of-order vs LDS, forcing vmcnt(0)+lgkmcnt(0)
// waits).  All rows live in global memory, so address-space-cast them.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 g_cu32x4;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) const uint8_t g_cu8;
typedef __attribute__((address_space(1))) uint8_t g_u8;

// A lane's column of one row: W dwords.  W = 4 is the 16-byte vector path
// (16-byte aligned rows), W = 1 the byte path (one byte in the low bits).
template <int W>
struct Col {
    uint32_t d[W];
};

template <int W>
__device__ __forceinline__ Col<W> col_load(const uint8_t* row, long long c)
{
    Col<W> r;
    if constexpr (W == 4) {
        const u32x4 v = ((g_cu32x4*)row)[c];
        r.d[0] = v.x; r.d[1] = v.y; r.d[2] = v.z; r.d[3] = v.w;
    } else {
        r.d[0] = ((g_cu8*)row)[c];
    }
    return r;
}

template <int W>
__device__ __forceinline__ void col_store(uint8_t* row, long long c, const Col<W>& v)
{
    if constexpr (W == 4) {
        u32x4 t;
        t.x = v.d[0]; t.y = v.d[1]; t.z = v.d[2]; t.w = v.d[3];
        ((g_u32x4*)row)[c] = t;
    } else {
        ((g_u8*)row)[c] = (uint8_t)v.d[0];
    }
}

// The row that explains a bad byte column of a locatable matrix (rsgpu.h), or
// -1: with s_0 and s_1 non-zero the ratio s_1 / s_0 picks the only source row
// r that can (rowtab, 255: none), x = s_0 / c[0][r], and every other syndrome
// must equal c[p][r] x; a column whose only non-zero syndrome is s_p0 is
// parity row k + p0.  nz: the column's non-zero syndromes (>= 1), p0: the
// last of them, syn(p): syndrome p of the column.  coef: the e x k matrix.
// One copy for k_scrub_compare, k_repair_compare (rs_kernels.hip), the
// generated scrub's cold path (rs_jit.hip) and k_correct_compare (rs_correct.hip).
template <class Syn>
__host__ __device__ __forceinline__ int scrub_locate_row(int k, int e, const uint8_t* rowtab, const uint8_t* coef,
                                                         const GfTables& gf, uint8_t s0, uint8_t s1, int nz, int p0,
                                                         Syn&& syn)
{
    if (s0 && s1) {
        const int r = rowtab[gf.exp[gf.log[s1] + 255 - gf.log[s0]]];
        if (r == 255)
            return -1;
        // log x of x = s_0 / c[0][r] (c[0][r] != 0: the matrix is locatable), in [0, 255)
        int lx = gf.log[s0] + 255 - gf.log[coef[r]];
        lx = lx >= 255 ? lx - 255 : lx;
        bool ok = true;
        for (int p = 2; p < e; ++p) {
            const uint8_t c = coef[(size_t)p * k + r];
            ok &= (uint8_t)syn(p) == (c ? gf.exp[gf.log[c] + lx] : 0);
        }
        return ok ? r : -1;
    }
    return nz == 1 ? k + p0 : -1;
}

// A wave's bad columns into its block's fold (rs_kernels.h ScrubFold): one
// atomic per wave and field, none for a wave without a bad column.
__device__ __forceinline__ void scrub_fold_wave(ScrubFold* f, unsigned long long bad, unsigned hi1, unsigned lo1)
{
    for (int off = 32; off > 0; off >>= 1) {
        bad += __shfl_down(bad, off, 64);
        hi1 = max(hi1, (unsigned)__shfl_down((int)hi1, off, 64));
        lo1 = max(lo1, (unsigned)__shfl_down((int)lo1, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && bad) {
        atomicAdd(&f->bad, bad);
        if (hi1) {
            atomicMax(&f->hi1, hi1);
            atomicMax(&f->lo1, lo1);
        }
    }
}

// the two maxima of a fold (ScrubFold, RepairFold) name the same row: every
// column that counted is explained by it
template <class F>
__device__ __forceinline__ bool fold_one_row(const F& f)
{
    return f.hi1 >= 1 && f.hi1 < kScrubNoRow && f.hi1 - 1 == kScrubBias - f.lo1;
}

// a block's finished fold as its report
__device__ __forceinline__ rsgpu_scrub_report scrub_verdict(const ScrubFold& f, int locate)
{
    rsgpu_scrub_report r;
    r.bad_columns = f.bad;
    const bool one = locate && fold_one_row(f);
    r.status = f.bad == 0 ? RSGPU_SCRUB_CLEAN : one ? RSGPU_SCRUB_ONE_ROW : RSGPU_SCRUB_DAMAGED;
    r.row = (f.bad != 0 && one) ? (int)f.hi1 - 1 : -1;
    return r;
}

// Workgroups per block of a kernel whose lanes own columns: enough columns
// each to amortise the staging of the block's tables, enough in all to fill
// the device when the batch is small.
inline unsigned columns_grid_x(long long ncols, long long blocks, int threads)
{
    const long long want = blocks >= 1024 ? 8 : (8192 + blocks - 1) / blocks;
    return (unsigned)std::max(1LL, std::min((ncols + threads - 1) / threads, want));
}

// f(std::integral_constant<int, G>) for g = lane_group(...) of rs_kernels.h:
// the runtime group size as the kernel's template argument.
template <class F>
inline void with_lane_group(int g, F&& f)
{
    switch (g) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

// LDS bytes of such a kernel: rows x g table entries (a uint4 of bits 0-5 and
// a dword of bits 6-7 each), then with `index` one dword per row.
inline size_t lane_tables_lds(int rows, int g, bool index)
{
    return (size_t)rows * g * (sizeof(uint4) + sizeof(uint32_t)) + (index ? (size_t)rows * sizeof(uint32_t) : 0);
}

}  // namespace rsgpu
