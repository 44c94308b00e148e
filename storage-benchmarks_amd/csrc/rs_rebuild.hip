// rs_rebuild.hip -- rebuild in place (rsgpu_rebuild_blocks) for gfx950: the
// rows a block's list names as lost are written back where they belong, lost
// parity rows included; in the checked mode the one surviving row the degraded
// scrub names joins them, and a block the scrub calls DAMAGED is left alone.
//
// With D the lost data rows and Q the pivot parity rows (chosen as the
// degraded scrub chooses them, rs_pivots.h), the lost data bytes are the
// solution that zeroes the syndromes of the rows in Q,
//   x_D = (c[Q][D])^-1 (par_Q ^ c[Q][S] x_S),   S the surviving data rows,
// and a lost parity row is the encode of the completed data.  So every row to
// write is a fixed linear combination of the same k source rows, the k - |D|
// rows of S and the |D| rows of Q: k_rebuild_prepare writes that k x (<= 8)
// matrix per block, and k_rebuild_blocks is one walk over the k sources with
// no encode into scratch and no second pass.
//
// k_rebuild_blocks is built like k_update_blocks and k_degraded_compare: a
// workgroup owns one block and a strided set of columns, stages the v_perm
// tables of its block's matrix in LDS, and a lane owns a 16-byte column (a
// byte in the byte kernel): it keeps the <= G outputs of its column in
// registers, splits every source into the 3-3-2 selector dwords once and
// XORs its <= G products in.  A lane reads and writes its own column only,
// and no row is both read and written: no atomics, no order between
// workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rs_pivots.h"

namespace rsgpu {

namespace {

constexpr int kRebThreads = 256;
constexpr int kSrcAhead = 4;  // source rows loaded together

// ---------------------------------------------------------------------------
// k_rebuild_prepare: one wave per block.  Lane 0 validates the list, with
// check reads the block's degraded report (the located row of ONE_ROW joins
// the list, DAMAGED and BAD_MATRIX stop the block), chooses the pivots and
// inverts c[Q][D]; the wave then writes the block's matrix, a source per lane.
// Without check every report is written here; with check only the one
// verdict the scrub does not reach: BAD_MATRIX of a list with n == e.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rebuild_prepare(RebuildArgs a)
{
    __shared__ PivotWork w;
    __shared__ uint8_t rows[8];    // the rows to write, ascending
    __shared__ uint8_t srcl[256];  // the k source rows: S ascending, then k + Q
    __shared__ int sh_state, sh_n, sh_nd;

    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    const int k = a.k, e = a.e, m = a.k + a.e;
    uint8_t* tab = a.tab + (size_t)b * a.tab_stride;
    RebuildHdr* hdr = reinterpret_cast<RebuildHdr*>(tab);
    const uint8_t* list = a.lost + b * a.u;

    for (int r = lane; r < 256; r += 64)
        w.lost[r] = 0;
    __syncthreads();

    if (lane == 0) {
        int n = lost_list_rows(list, a.u, m, e);
        int state = kRebStop, status = RSGPU_SCRUB_CLEAN, nd = 0;
        bool report = !a.check;
        if (n < 0) {
            status = RSGPU_SCRUB_BAD_LIST;
            n = 0;
        } else if (a.work) {
            for (int i = 0; i < n; ++i)
                rows[i] = list[i];
            bool go = true;
            if (a.check) {
                const rsgpu_scrub_report r = a.report[b];
                if (r.status == RSGPU_SCRUB_ONE_ROW) {
                    // the located row joins the list, which stays ascending (there
                    // is room: u <= 7 with check, and ONE_ROW needs e - n >= 2)
                    go = r.row >= 0 && r.row < m && n < 8 && n < e;
                    int at = 0;
                    while (go && at < n && rows[at] < r.row)
                        ++at;
                    go = go && (at == n || rows[at] != r.row);
                    if (go) {
                        for (int i = n; i > at; --i)
                            rows[i] = rows[i - 1];
                        rows[at] = (uint8_t)r.row;
                        ++n;
                    }
                } else if (r.status != RSGPU_SCRUB_CLEAN && r.status != RSGPU_SCRUB_UNCHECKED) {
                    go = false;  // DAMAGED, BAD_MATRIX: the scrub's report is final
                }
            }
            if (go && n > 0) {
                nd = lost_pivots(w, rows, n, a.coef, k, e);
                if (nd < 0) {
                    status = RSGPU_SCRUB_BAD_MATRIX;
                    report = true;
                } else {
                    state = kRebRun;
                    int ns = 0;
                    for (int j = 0; j < k; ++j)
                        if (!w.lost[j])
                            srcl[ns++] = (uint8_t)j;
                    for (int q = 0; q < nd; ++q)
                        srcl[ns++] = (uint8_t)(k + w.ql[q]);
                }
            }
        }
        sh_state = state;
        sh_n = n;
        sh_nd = nd;
        if (report) {
            rsgpu_scrub_report r;
            r.bad_columns = 0;
            r.status = status;
            r.row = -1;
            a.report[b] = r;
        }
        hdr->state = state;
        hdr->nout = (uint8_t)(state == kRebRun ? n : 0);
    }
    __syncthreads();
    if (sh_state != kRebRun)
        return;
    const int n = sh_n, nd = sh_nd;
    if (lane < 8)
        hdr->out[lane] = lane < n ? rows[lane] : 0;
    uint8_t* t_src = tab + sizeof(RebuildHdr);
    uint8_t* t_m = t_src + a.src_bytes;
    for (int s = lane; s < k; s += 64) {
        const int r = srcl[s];
        t_src[s] = (uint8_t)r;
        // the factor of source s in lost data row D_i
        uint8_t mi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint8_t x = 0;
            if (i < nd) {
                if (r < k) {
                    for (int q = 0; q < nd; ++q)
                        x ^= gf_mul_slow(w.inv[i][q], a.coef[(size_t)w.ql[q] * k + r]);
                } else {
                    x = w.inv[i][s - (k - nd)];
                }
            }
            mi[i] = x;
        }
        // outputs: the rows of D first (the list is ascending), then parity rows
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            uint8_t x = 0;
            if (o < nd) {
                x = mi[o];
            } else if (o < n) {
                const size_t p = (size_t)(rows[o] - k) * k;
                x = r < k ? a.coef[p + r] : 0;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (i < nd)
                        x ^= gf_mul_slow(a.coef[p + w.dl[i]], mi[i]);
            }
            t_m[(size_t)s * 8 + o] = x;
        }
    }
}

// row r of [0, k + e) of a block
__device__ __forceinline__ uint8_t* block_row(uint8_t* srcb, uint8_t* parb, int r, int k, long long pitch)
{
    return r < k ? srcb + (long long)r * pitch : parb + (long long)(r - k) * pitch;
}

// ---------------------------------------------------------------------------
// k_rebuild_wide_prepare: lists of up to kWide rows, one wave per block.  Lane
// 0 judges the list and takes the verdict as k_rebuild_prepare does; the pivot
// walk and the elimination run on the whole wave (rs_pivots.h
// lost_pivots_wave); then a source per lane forms its row of the k x n matrix
// of factors M in LDS, by k_rebuild_prepare's formulas, and the wave writes
// what the kernels read: the lane tables of the passes of 8 outputs
// (k_rebuild_blocks) and the row pointers, handler addresses and row count of
// the threaded code (rs_tc.hip k_rs_tc, TcHooksPerBlock).
// ---------------------------------------------------------------------------
constexpr int kWide = RSGPU_REBUILD_MAX_LOST;

__global__ __launch_bounds__(64) void k_rebuild_wide_prepare(RebuildWideArgs wa)
{
    __shared__ PivotWave<kWide> w;
    __shared__ uint8_t rows[kWide];       // the rows to write, ascending
    __shared__ uint8_t srcl[256];         // the k source rows: S ascending, then k + Q
    __shared__ uint8_t mf[256][kWide];    // M[s][o]
    __shared__ int sh_go, sh_n, sh_status;

    const RebuildArgs& a = wa.r;
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    const int k = a.k, e = a.e, m = a.k + a.e;
    const uint8_t* list = a.lost + b * a.u;

    for (int r = lane; r < 256; r += 64)
        w.lost[r] = 0;
    if (lane == 0) {
        int n = lost_list_rows(list, a.u, m, e);
        bool go = false;
        sh_status = RSGPU_SCRUB_CLEAN;
        if (n < 0) {
            n = 0;
            sh_status = RSGPU_SCRUB_BAD_LIST;
        } else if (a.work) {
            for (int i = 0; i < n; ++i)
                rows[i] = list[i];
            go = true;
            if (a.check) {
                const rsgpu_scrub_report r = a.report[b];
                if (r.status == RSGPU_SCRUB_ONE_ROW) {
                    // the located row joins the list, which stays ascending
                    go = r.row >= 0 && r.row < m && n < kWide && n < e;
                    int at = 0;
                    while (go && at < n && rows[at] < r.row)
                        ++at;
                    go = go && (at == n || rows[at] != r.row);
                    if (go) {
                        for (int i = n; i > at; --i)
                            rows[i] = rows[i - 1];
                        rows[at] = (uint8_t)r.row;
                        ++n;
                    }
                } else if (r.status != RSGPU_SCRUB_CLEAN && r.status != RSGPU_SCRUB_UNCHECKED) {
                    go = false;  // DAMAGED, BAD_MATRIX: the scrub's report is final
                }
            }
            go = go && n > 0;
        }
        sh_go = go ? 1 : 0;
        sh_n = n;
    }
    __syncthreads();
    const int n = sh_n;
    int nd = -2;  // -2: the matrix is not looked at
    if (sh_go)
        nd = lost_pivots_wave(w, rows, n, a.coef, k, e, lane);
    const bool run = nd >= 0;
    if (lane == 0) {
        // without check every report is written here; with check only the one
        // verdict the scrub does not reach: BAD_MATRIX of a list with n == e
        if (nd == -1 || !a.check) {
            rsgpu_scrub_report r;
            r.bad_columns = 0;
            r.status = nd == -1 ? RSGPU_SCRUB_BAD_MATRIX : sh_status;
            r.row = -1;
            a.report[b] = r;
        }
        if (wa.slots > 0)
            wa.count[b] = run ? n : 0;
        if (run) {
            int ns = 0;
            for (int j = 0; j < k; ++j)
                if (!w.lost[j])
                    srcl[ns++] = (uint8_t)j;
            for (int q = 0; q < nd; ++q)
                srcl[ns++] = (uint8_t)(k + w.ql[q]);
        }
    }
    // the lane tables' headers: a pass the block has no row of does not run
    const size_t pass_stride = sizeof(RebuildHdr) + a.src_bytes + (size_t)k * 8;  // rebuild_tab_stride(k)
    uint8_t* tab0 = a.tab + (size_t)b * a.tab_stride;
    for (int p = lane; p < wa.passes; p += 64) {
        RebuildHdr* hdr = reinterpret_cast<RebuildHdr*>(tab0 + (size_t)p * pass_stride);
        const int np = run ? (n - 8 * p < 8 ? n - 8 * p : 8) : 0;
        hdr->state = np > 0 ? kRebRun : kRebStop;
        hdr->nout = (uint8_t)(np > 0 ? np : 0);
        for (int i = 0; i < 8; ++i)
            hdr->out[i] = i < np ? rows[8 * p + i] : 0;
    }
    if (!run)
        return;  // uniform
    __syncthreads();
    for (int s = lane; s < k; s += 64) {
        const int r = srcl[s];
        // the factor of source s in lost data row D_i
        for (int i = 0; i < nd; ++i) {
            uint8_t x = 0;
            if (r < k) {
                for (int q = 0; q < nd; ++q)
                    x ^= gf_mul_slow(w.inv(i, q), a.coef[(size_t)w.ql[q] * k + r]);
            } else {
                x = w.inv(i, s - (k - nd));
            }
            mf[s][i] = x;
        }
        // outputs: the rows of D first (the list is ascending), then parity rows
        for (int o = nd; o < kWide; ++o) {
            uint8_t x = 0;
            if (o < n) {
                const size_t p = (size_t)(rows[o] - k) * k;
                x = r < k ? a.coef[p + r] : 0;
                for (int i = 0; i < nd; ++i)
                    x ^= gf_mul_slow(a.coef[p + w.dl[i]], mf[s][i]);
            }
            mf[s][o] = x;
        }
    }
    __syncthreads();
    uint8_t* srcb = a.src + b * k * a.pitch;
    uint8_t* parb = a.par + b * e * a.pitch;
    for (int p = 0; p < wa.passes && 8 * p < n; ++p) {
        uint8_t* tab = tab0 + (size_t)p * pass_stride;
        uint8_t* t_src = tab + sizeof(RebuildHdr);
        uint8_t* t_m = t_src + a.src_bytes;
        for (int s = lane; s < k; s += 64)
            t_src[s] = srcl[s];
        for (int idx = lane; idx < k * 8; idx += 64)
            t_m[idx] = mf[idx >> 3][8 * p + (idx & 7)];
    }
    if (wa.slots > 0) {
        const int slots = wa.slots;
        for (int s = lane; s < k; s += 64)
            wa.srcs[(size_t)b * k + s] = block_row(srcb, parb, srcl[s], k, a.pitch);
        for (int o = lane; o < slots; o += 64)
            wa.dsts[(size_t)b * slots + o] = o < n ? block_row(srcb, parb, rows[o], k, a.pitch) : nullptr;
        unsigned long long* ad = wa.addr + (size_t)b * k * slots;
        for (int idx = lane; idx < k * slots; idx += 64) {
            const int s = idx / slots, o = idx - s * slots;
            ad[idx] = wa.tc_table[(o & 7) * 256 + (o < n ? mf[s][o] : 0)];
        }
    }
}

// A rebuilt column: nobody reads it again soon, so the 16-byte store is
// non-temporal (1 - 3 % of the call at one or two rows per block, nothing at
// eight; profiles/rebuild).
template <int W>
__device__ __forceinline__ void row_store(uint8_t* row, long long c, const Col<W>& v)
{
    if constexpr (W == 4) {
        u32x4 t;
        t.x = v.d[0]; t.y = v.d[1]; t.z = v.d[2]; t.w = v.d[3];
        __builtin_nontemporal_store(t, (g_u32x4*)row + c);
    } else {
        col_store<W>(row, c, v);
    }
}

// G: outputs a lane holds; W: dwords per lane and row.  Columns [col0, col1)
// in units of 16 bytes (W = 4) or bytes (W = 1).
template <int G, int W>
__global__ __launch_bounds__(kRebThreads) void k_rebuild_blocks(RebuildArgs a, long long col0, long long col1)
{
    extern __shared__ uint4 lt4[];  // [k][G] tables of bits 0-5, [k][G] dwords of bits 6-7, [k] source rows
    uint32_t* ltc = reinterpret_cast<uint32_t*>(lt4 + (size_t)a.k * G);
    uint32_t* lsrc = ltc + (size_t)a.k * G;
    const long long b = blockIdx.y;
    const uint8_t* tab = a.tab + (size_t)b * a.tab_stride;
    const RebuildHdr* hdr = reinterpret_cast<const RebuildHdr*>(tab);
    if (hdr->state != kRebRun)
        return;  // the whole workgroup: nothing of this block is written
    const int k = a.k;
    const int nout = hdr->nout < G ? hdr->nout : G;
    const uint8_t* t_src = tab + sizeof(RebuildHdr);
    const uint8_t* t_m = t_src + a.src_bytes;
    int outr[G];
#pragma unroll
    for (int i = 0; i < G; ++i)
        outr[i] = hdr->out[i];

    for (int idx = threadIdx.x; idx < k * G; idx += kRebThreads) {
        const int s = idx / G, i = idx - s * G;
        if (i < nout) {
            const uint8_t c = t_m[s * 8 + i];
            lt4[idx] = a.tab4[c];
            ltc[idx] = a.tabc[c];
        }
    }
    for (int s = threadIdx.x; s < k; s += kRebThreads)
        lsrc[s] = t_src[s];
    __syncthreads();

    uint8_t* srcb = a.src + b * k * a.pitch;
    uint8_t* parb = a.par + b * a.e * a.pitch;
    const long long stride = (long long)gridDim.x * kRebThreads;

    for (long long col = col0 + (long long)blockIdx.x * kRebThreads + threadIdx.x; col < col1; col += stride) {
        uint32_t acc[G][W];
#pragma unroll
        for (int i = 0; i < G; ++i)
#pragma unroll
            for (int w = 0; w < W; ++w)
                acc[i][w] = 0;
        // one walk over the sources, kSrcAhead loads in flight
        for (int s0 = 0; s0 < k; s0 += kSrcAhead) {
            Col<W> x[kSrcAhead];
#pragma unroll
            for (int q = 0; q < kSrcAhead; ++q)
                if (s0 + q < k) {
                    const int r = __builtin_amdgcn_readfirstlane((int)lsrc[s0 + q]);
                    x[q] = col_load<W>(block_row(srcb, parb, r, k, a.pitch), col);
                }
#pragma unroll
            for (int q = 0; q < kSrcAhead; ++q) {
                if (s0 + q < k) {
                    const uint4* t4 = lt4 + (size_t)(s0 + q) * G;
                    const uint32_t* tc = ltc + (size_t)(s0 + q) * G;
                    uint32_t v0[W], v1[W], v2[W];
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        sel_split(x[q].d[w], v0[w], v1[w], v2[w]);
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        if (i < nout) {
                            const uint4 t = t4[i];
                            const uint32_t c = tc[i];
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                acc[i][w] ^= sel_mul(t, c, v0[w], v1[w], v2[w]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (i < nout) {
                Col<W> v;
#pragma unroll
                for (int w = 0; w < W; ++w)
                    v.d[w] = acc[i][w];
                row_store<W>(block_row(srcb, parb, outr[i], k, a.pitch), col, v);
            }
        }
    }
}

template <int W>
hipError_t launch_w(const RebuildArgs& a, long long col0, long long col1, hipStream_t st)
{
    const dim3 grid(columns_grid_x(col1 - col0, a.blocks, kRebThreads), (unsigned)a.blocks), block(kRebThreads);
    const size_t lds = lane_tables_lds(a.k, a.g, true);
    with_lane_group(a.g, [&](auto G) {
        hipLaunchKernelGGL((k_rebuild_blocks<decltype(G)::value, W>), grid, block, lds, st, a, col0, col1);
    });
    return hipGetLastError();
}

bool args_ok(const RebuildArgs& a)
{
    return a.blocks > 0 && a.blocks <= (long long)kMaxGridBlocks && a.k > 0 && a.e >= 0 &&
           a.k + a.e <= RSGPU_MAX_SOURCES && a.u >= 1 && a.u <= 8 && a.lost && a.tab && a.report &&
           a.tab_stride >= rebuild_tab_stride(a.k) && a.src_bytes == rebuild_src_bytes(a.k);
}

}  // namespace

size_t rebuild_src_bytes(int k) { return ((size_t)k + 15) / 16 * 16; }

size_t rebuild_tab_stride(int k) { return sizeof(RebuildHdr) + rebuild_src_bytes(k) + (size_t)k * 8; }

hipError_t launch_rebuild_prepare(const RebuildArgs& a, hipStream_t st)
{
    if (!args_ok(a) || (a.work && !a.coef) || (a.check && a.u > 7))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rebuild_prepare, dim3((unsigned)a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_rebuild_wide_prepare(const RebuildWideArgs& wa, hipStream_t st)
{
    const RebuildArgs& a = wa.r;
    const int most = std::min(a.u + (a.check ? 1 : 0), a.e);
    if (a.blocks <= 0 || a.blocks > (long long)kMaxGridBlocks || a.k <= 0 || a.e < 0 ||
        a.k + a.e > RSGPU_MAX_SOURCES || a.u < 1 || a.u > kWide || (a.check && a.u > 7) || !a.lost || !a.report ||
        (a.work && (!a.coef || !a.src || !a.par)) || wa.passes < 0 || wa.slots < 0)
        return hipErrorInvalidValue;
    if (wa.passes > 0 && (!a.work || !a.tab || wa.passes * 8 < most || a.src_bytes != rebuild_src_bytes(a.k) ||
                          a.tab_stride < (size_t)wa.passes * rebuild_tab_stride(a.k)))
        return hipErrorInvalidValue;
    if (wa.slots > 0 && (!a.work || wa.slots != tc_rows_per_pass(most) || wa.slots > kWide || !wa.tc_table ||
                         !wa.srcs || !wa.dsts || !wa.addr || !wa.count))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rebuild_wide_prepare, dim3((unsigned)a.blocks), dim3(64), 0, st, wa);
    return hipGetLastError();
}

hipError_t launch_rebuild_blocks(const RebuildArgs& a, bool bytes, long long col0, long long col1, hipStream_t st)
{
    const int most = a.u + (a.check ? 1 : 0);  // rows of any block's list as it is rebuilt
    if (!args_ok(a) || !a.work || !a.src || !a.par || !a.tab4 || !a.tabc || col0 < 0 || col1 <= col0 ||
        col1 * (bytes ? 1 : 16) > a.len || a.len > a.pitch || a.g != lane_group(most < a.e ? most : a.e))
        return hipErrorInvalidValue;
    return bytes ? launch_w<1>(a, col0, col1, st) : launch_w<4>(a, col0, col1, st);
}

}  // namespace rsgpu
