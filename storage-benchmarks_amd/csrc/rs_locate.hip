// rs_locate.hip -- locate several damaged rows per block (rsgpu_locate_blocks)
// for gfx950.  Nothing is written but the lists and the reports.
//
// With s_p the syndromes of a byte column (stored ^ recomputed parity) and
// h_r what a unit change of row r adds to them (column r of the matrix for a
// data row, a unit vector for a parity row), a block damaged in the rows R'
// has every syndrome column inside span(h_R').  W, the span of ALL the block's
// syndrome columns, is therefore a function of the block alone, and the rows
// are read off as R = { r : h_r in W }; the verdict stands when |R| = dim W =
// rank(h_R) (include/rsgpu.h).
//
// k_locate_span is the hot kernel, shaped like k_degraded_compare: a workgroup
// owns one block and a strided set of columns, a lane a 16-byte column (a byte
// in the byte kernel) whose syndromes it ORs over the e rows.  Bad columns go
// to the wave as a whole, under wave-uniform control: lane p loads syndrome p
// (hence e <= 64), and the vector is reduced against the wave's basis of W, at
// most u vectors in reduced echelon form in LDS; a non-zero residual is
// normalised and appended.  After a barrier wave 0 merges the workgroup's
// bases and writes the result to the workgroup's own slot of the block's
// candidate area.  k_locate_finish, one wave per block, merges the slots to
// W's basis, tests the k + e columns h_r, checks the count and the rank and
// writes the list and the report.  No workgroup waits for another one; W does
// not depend on the order in which its vectors are found, so neither does a
// byte of the output.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rs_span.h"

namespace rsgpu {

namespace {

constexpr int kLocThreads = 256, kLocWaves = kLocThreads / 64;
constexpr int kLocAhead = 4;  // rows (stored and computed) loaded together

__device__ const GfTables kLocGf = make_gf_tables();

// W: dwords per lane and row.  Columns [col0, col1) in units of 16 bytes (W =
// 4) or bytes (W = 1).  Workgroup x of block b writes slot slot0 + x.
template <int W>
__global__ __launch_bounds__(kLocThreads) void k_locate_span(LocateArgs a, long long col0, long long col1, int slot0)
{
    __shared__ GfTables gf;
    __shared__ SpanBasis sb[kLocWaves];
    const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
    const long long b = blockIdx.y;
    const int e = a.e;

    load_gf(gf, kLocGf, threadIdx.x, kLocThreads);
    sb[wave].n = 0;
    sb[wave].ovf = 0;
    __syncthreads();

    SpanBasis& s = sb[wave];
    const uint8_t* calcb = a.calc + b * e * a.pitch;
    const uint8_t* parb = a.par + b * e * a.pitch;
    const long long stride = (long long)gridDim.x * kLocThreads;
    unsigned long long bad = 0;  // the wave's bad byte columns, the same in every lane

    for (long long base = col0 + (long long)blockIdx.x * kLocThreads + wave * 64; base < col1; base += stride) {
        const long long col = base + lane;
        uint32_t any[W];
#pragma unroll
        for (int w = 0; w < W; ++w)
            any[w] = 0;
        if (col < col1) {
            for (int p0 = 0; p0 < e; p0 += kLocAhead) {
                Col<W> x[kLocAhead], y[kLocAhead];
#pragma unroll
                for (int q = 0; q < kLocAhead; ++q)
                    if (p0 + q < e) {
                        const long long off = (long long)(p0 + q) * a.pitch;
                        x[q] = col_load<W>(parb + off, col);
                        y[q] = col_load<W>(calcb + off, col);
                    }
#pragma unroll
                for (int q = 0; q < kLocAhead; ++q)
                    if (p0 + q < e) {
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            any[w] |= x[q].d[w] ^ y[q].d[w];
                    }
            }
        }
        uint32_t all = 0;
#pragma unroll
        for (int w = 0; w < W; ++w)
            all |= any[w];
        // the lanes with a bad column, one after the other, the whole wave on each
        unsigned long long todo = __ballot(all != 0);
        while (todo) {
            const int from = __ffsll(todo) - 1;
            todo &= todo - 1;
            const long long bc = base + from;
            uint32_t syn[W];  // lane p: syndrome p of the column's bytes
#pragma unroll
            for (int w = 0; w < W; ++w)
                syn[w] = 0;
            if (lane < e) {
                const long long off = (long long)lane * a.pitch;
                const Col<W> x = col_load<W>(parb + off, bc);
                const Col<W> y = col_load<W>(calcb + off, bc);
#pragma unroll
                for (int w = 0; w < W; ++w)
                    syn[w] = x.d[w] ^ y.d[w];
            }
#pragma unroll 1
            for (int j = 0; j < (W == 4 ? 16 : 1); ++j) {
                uint32_t d = syn[0];
                if constexpr (W == 4)
                    d = j < 4 ? syn[0] : j < 8 ? syn[1] : j < 12 ? syn[2] : syn[3];
                const uint8_t v = (uint8_t)(d >> (8 * (j & 3)));
                if (!__ballot(v != 0))
                    continue;
                ++bad;
                span_append(s, gf, lane, span_reduce(s, gf, lane, v), a.u);
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        // (rs_span.h span_publish, written out: through the call the compiler
        // lays this kernel's blocks out differently)
        for (int w = 1; w < kLocWaves; ++w) {
            const int nw = uni(sb[w].n);
            if (uni(sb[w].ovf))
                s.ovf = 1;
            for (int i = 0; i < nw; ++i)
                span_append(s, gf, lane, span_reduce(s, gf, lane, sb[w].v[i][lane]), a.u);
        }
        uint8_t* slot = a.cand + (size_t)b * a.cand_stride + (size_t)(slot0 + blockIdx.x) * kLocateSlotBytes;
        const int n = uni(s.n);
        if (lane == 0) {
            SlotHdr* hdr = reinterpret_cast<SlotHdr*>(slot);
            hdr->n = n;
            hdr->ovf = s.ovf;
        }
        for (int i = 0; i < n; ++i)
            slot[sizeof(SlotHdr) + i * 64 + lane] = s.v[i][lane];
    }
    if (lane == 0 && bad)
        atomicAdd(&reinterpret_cast<ScrubFold*>(a.report)[b].bad, bad);
}

// ---------------------------------------------------------------------------
// k_locate_finish: one wave per block.  The block's slots merged to W's basis
// (d = its size), every column h_r reduced against it (d steps each), the
// members counted and put through a second elimination for their rank; then
// the list and the report.  With !work (e == 0 or len == 0) every block is
// CLEAN.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_locate_finish(LocateArgs a)
{
    __shared__ GfTables gf;
    __shared__ SpanBasis wb, hb;  // W; the span of the members' columns
    __shared__ uint8_t found[kLocMax];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const int k = a.k, e = a.e;

    load_gf(gf, kLocGf, lane, 64);
    wb.n = wb.ovf = 0;
    hb.n = hb.ovf = 0;
    __syncthreads();

    const unsigned long long bad = a.work ? reinterpret_cast<const ScrubFold*>(a.report)[b].bad : 0;
    int status = RSGPU_SCRUB_CLEAN, d = 0;
    if (bad) {
        status = RSGPU_SCRUB_DAMAGED;
        const uint8_t* cand = a.cand + (size_t)b * a.cand_stride;
        // claimed (k_rs_bs_locate): only the block's dirty tiles wrote a slot, each
        // the next free one; their count stands where the status will
        int slots = a.slots;
        if (a.claimed)
            slots = min((int)reinterpret_cast<const ScrubFold*>(a.report)[b].hi1, slots);
        // 64 slot headers at a time; most slots of a lightly damaged block are empty
        for (int s0 = 0; s0 < slots; s0 += 64) {
            int n_l = 0, o_l = 0;
            if (s0 + lane < slots) {
                const SlotHdr* hdr = reinterpret_cast<const SlotHdr*>(cand + (size_t)(s0 + lane) * kLocateSlotBytes);
                n_l = hdr->n < kLocMax ? hdr->n : kLocMax;
                o_l = hdr->ovf;
            }
            if (__ballot(o_l != 0))
                wb.ovf = 1;
            unsigned long long todo = __ballot(n_l > 0);
            while (todo) {
                const int from = __ffsll(todo) - 1;
                todo &= todo - 1;
                const int n = __builtin_amdgcn_readlane(n_l, from);
                const uint8_t* vec = cand + (size_t)(s0 + from) * kLocateSlotBytes + sizeof(SlotHdr);
                for (int i = 0; i < n; ++i)
                    span_append(wb, gf, lane, span_reduce(wb, gf, lane, vec[i * 64 + lane]), a.u);
            }
        }
        d = uni(wb.n);
        if (!uni(wb.ovf)) {
            int cnt = 0;
            for (int r = 0; r < k + e && cnt <= d; ++r) {
                uint8_t h = 0;
                if (lane < e)
                    h = r < k ? a.coef[(size_t)lane * k + r] : (uint8_t)(lane == r - k);
                if (__ballot(span_reduce(wb, gf, lane, h) != 0))
                    continue;
                if (cnt < kLocMax)
                    found[cnt] = (uint8_t)r;
                ++cnt;
                span_append(hb, gf, lane, span_reduce(hb, gf, lane, h), kLocMax);
            }
            if (cnt == d && uni(hb.n) == d)
                status = d == 1 ? RSGPU_SCRUB_ONE_ROW : RSGPU_SCRUB_ROWS;
        }
    }
    __syncthreads();
    const bool located = status == RSGPU_SCRUB_ONE_ROW || status == RSGPU_SCRUB_ROWS;
    if (lane < a.u)
        a.rows[b * a.u + lane] = located && lane < d ? found[lane] : (uint8_t)RSGPU_LOST_NONE;
    if (lane == 0) {
        rsgpu_scrub_report rep;
        rep.bad_columns = bad;
        rep.status = status;
        rep.row = located ? found[0] : -1;
        a.report[b] = rep;
    }
}

bool args_ok(const LocateArgs& a)
{
    return a.blocks > 0 && a.blocks <= (long long)kMaxGridBlocks && a.k > 0 && a.e >= 0 && a.e <= 64 &&
           a.k + a.e <= RSGPU_MAX_SOURCES && a.u >= 1 && a.u <= kLocMax && a.report && a.slots >= 0 &&
           (a.slots == 0 || (a.cand && a.cand_stride >= (size_t)a.slots * kLocateSlotBytes));
}

}  // namespace

hipError_t launch_locate_span(const LocateArgs& a, bool bytes, long long col0, long long col1, unsigned gx, int slot0,
                              hipStream_t st)
{
    if (!args_ok(a) || !a.work || a.e < 1 || !a.calc || !a.par || col0 < 0 || col1 <= col0 ||
        col1 * (bytes ? 1 : 16) > a.len || gx < 1 || slot0 < 0 || (long long)slot0 + gx > a.slots)
        return hipErrorInvalidValue;
    const dim3 grid(gx, (unsigned)a.blocks), block(kLocThreads);
    if (bytes)
        hipLaunchKernelGGL(k_locate_span<1>, grid, block, 0, st, a, col0, col1, slot0);
    else
        hipLaunchKernelGGL(k_locate_span<4>, grid, block, 0, st, a, col0, col1, slot0);
    return hipGetLastError();
}

hipError_t launch_locate_finish(const LocateArgs& a, hipStream_t st)
{
    if (!args_ok(a) || !a.rows || (a.work && (!a.coef || a.slots < 1)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locate_finish, dim3((unsigned)a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace rsgpu
