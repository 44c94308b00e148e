// rs_degraded.hip -- degraded scrub (rsgpu_scrub_degraded_blocks) for gfx950:
// are the SURVIVING rows of a block consistent, when up to e of its k + e rows
// are known to be lost?  Nothing is rebuilt and no row is written.
//
// With D the lost data rows, P the lost parity rows and s_p the raw syndromes
// (stored ^ recomputed parity, the recomputed one over all k source rows as
// they lie in memory), a byte column is consistent when some choice of the
// lost bytes zeroes every syndrome.  The lost parity rows can always be
// chosen, so only the surviving parity rows S count, and the lost data bytes
// enter them through c[S][D]: the column is consistent when s_S lies in the
// column space of c[S][D].  k_degraded_prepare picks |D| pivot rows Q of S
// with c[Q][D] invertible and writes R = c[rest][D] (c[Q][D])^-1 for the
// other rows of S; the reduced syndromes
//   t_p = s_p ^ XOR_i R[p][i] * s_Q[i],   p in rest,
// are then zero exactly for a consistent column, and the bytes stored in the
// lost rows cancel out of them.  A surviving row r explains a bad column when
// t is a non-zero multiple of r's own reduced column h_r (prepare writes
// those too): c[rest][r] ^ R c[Q][r] for a data row, column i of R for the
// pivot parity row Q[i], a unit vector for a rest parity row.
//
// k_degraded_compare is the hot kernel, built like k_update_blocks: a
// workgroup owns one block and a strided set of columns, stages the v_perm
// tables of its block's R in LDS, and a lane owns a 16-byte column (a byte in
// the byte kernel): it loads the |Q| <= 8 pivot syndromes once, keeps them as
// the selector dwords of the 3-3-2 split, and walks the rest rows once.  Rows
// in P are never loaded: 2 (e - |P|) rows per block, each read once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rs_pivots.h"

namespace rsgpu {

namespace {

constexpr int kDegThreads = 256;
constexpr int kRestAhead = 4;  // rest rows (stored and computed) loaded together

// ---------------------------------------------------------------------------
// k_degraded_prepare: one wave per block.  Lane 0 validates the list, splits
// it, chooses the pivot rows greedily (ascending surviving parity rows, each
// kept when it raises the rank of c[Q][D]) and inverts c[Q][D]; the wave then
// writes R and, with locate, the reduced column of every row.  A block that
// never reaches the compare gets its final report here; the others get a
// zeroed fold.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_degraded_prepare(DegradedArgs a)
{
    __shared__ PivotWork w;         // the lost rows, D, Q and (c[Q][D])^-1 (rs_pivots.h)
    __shared__ uint8_t restl[256];  // rest parity indices, ascending
    __shared__ uint8_t rl[256 * 8]; // R [nrest][8]
    __shared__ int sh_state, sh_nd, sh_nrest;
    uint8_t (&lost)[256] = w.lost;
    uint8_t (&dl)[8] = w.dl, (&ql)[8] = w.ql;
    uint8_t (&inv)[8][8] = w.inv;

    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    const int k = a.k, e = a.e, m = a.k + a.e;
    uint8_t* tab = a.tab + (size_t)b * a.tab_stride;
    DegradedHdr* hdr = reinterpret_cast<DegradedHdr*>(tab);
    const uint8_t* list = a.lost + b * a.u;

    for (int r = lane; r < 256; r += 64)
        lost[r] = 0;
    __syncthreads();

    if (lane == 0) {
        const int n = lost_list_rows(list, a.u, m, e);
        int nd = 0;
        int state = kDegRun;
        if (n < 0) {
            state = RSGPU_SCRUB_BAD_LIST;
        } else if (!a.work) {
            state = kDegClean;
        } else if (n == e) {
            state = RSGPU_SCRUB_UNCHECKED;
        } else {
            nd = lost_pivots(w, list, n, a.coef, k, e);
            if (nd < 0) {
                state = RSGPU_SCRUB_BAD_MATRIX;
            } else {
                // the rest: surviving parity rows that are no pivot
                int nrest = 0, qi = 0;
                for (int p = 0; p < e; ++p) {
                    if (lost[k + p])
                        continue;
                    if (qi < nd && ql[qi] == p) {
                        ++qi;
                        continue;
                    }
                    restl[nrest++] = (uint8_t)p;
                }
                sh_nrest = nrest;
            }
        }
        sh_state = state;
        sh_nd = nd;
        // the report: final for a block that stops here, a zeroed fold otherwise
        rsgpu_scrub_report r;
        r.bad_columns = 0;
        r.status = state == kDegRun || state == kDegClean ? RSGPU_SCRUB_CLEAN : state;
        r.row = state == kDegRun ? 0 : -1;
        a.report[b] = r;
        hdr->state = state;
    }
    __syncthreads();
    if (sh_state != kDegRun)
        return;
    const int nd = sh_nd, nrest = sh_nrest;
    if (lane == 0) {
        hdr->nq = (uint8_t)nd;
        hdr->nrest = (uint8_t)nrest;
    }
    if (lane < 8)
        hdr->q[lane] = lane < nd ? ql[lane] : 0;
    uint8_t* t_rest = tab + sizeof(DegradedHdr);
    uint8_t* t_r = t_rest + a.rest_bytes;
    uint8_t* t_h = t_r + (size_t)e * 8;
    for (int pi = lane; pi < nrest; pi += 64)
        t_rest[pi] = restl[pi];
    // R[pi][i] = XOR_j c[rest_pi][D_j] * inv[j][i]
    for (int idx = lane; idx < nrest * 8; idx += 64) {
        const int pi = idx >> 3, i = idx & 7;
        uint8_t x = 0;
        if (i < nd)
            for (int j = 0; j < nd; ++j)
                x ^= gf_mul_slow(a.coef[(size_t)restl[pi] * k + dl[j]], inv[j][i]);
        rl[idx] = x;
        t_r[idx] = x;
    }
    if (!a.locate)
        return;
    __syncthreads();
    // the reduced column of every row, [k + e][e] with nrest entries used
    for (int idx = lane; idx < m * nrest; idx += 64) {
        const int r = idx / nrest, pi = idx - r * nrest;
        uint8_t h = 0;
        if (!lost[r]) {
            if (r < k) {
                h = a.coef[(size_t)restl[pi] * k + r];
                for (int i = 0; i < nd; ++i)
                    h ^= gf_mul_slow(rl[pi * 8 + i], a.coef[(size_t)ql[i] * k + r]);
            } else {
                const int p = r - k;
                if (restl[pi] == p)
                    h = 1;
                for (int i = 0; i < nd; ++i)
                    if (ql[i] == p)
                        h = rl[pi * 8 + i];
            }
        }
        t_h[(size_t)r * e + pi] = h;
    }
}

// ---------------------------------------------------------------------------
// The cold path: which surviving rows explain byte column ci of a block?
// Returns the row when exactly one does, else -1.  t is recomputed from
// memory, entry by entry; a candidate row r must have t = x h_r for one
// x != 0, tested without a division as t_p h_r[p*] == t_p* h_r[p] for every p,
// p* the first non-zero entry of t.  One other entry of t screens the rows
// before the full walk.
// ---------------------------------------------------------------------------
struct DegBlock {
    const uint8_t* calc;  // the block's recomputed parity rows
    const uint8_t* par;   // the block's stored parity rows
    const uint8_t* rest;  // [nrest]
    const uint8_t* r;     // [nrest][8]
    const uint8_t* h;     // [k + e][e]
    long long pitch;
    int nq, nrest, rows, e;
    uint8_t q[8];
};

__device__ __forceinline__ uint8_t deg_t(const DegBlock& d, unsigned long long sq, int pi, long long ci)
{
    const size_t off = (size_t)d.rest[pi] * d.pitch + ci;
    uint8_t t = d.calc[off] ^ d.par[off];
    for (int i = 0; i < d.nq; ++i)
        t ^= gf_mul_slow(d.r[pi * 8 + i], (uint8_t)(sq >> (8 * i)));
    return t;
}

__device__ __noinline__ int deg_locate(const uint8_t* tab, const uint8_t* calcb, const uint8_t* parb,
                                       long long pitch, int k, int e, int rest_bytes, long long ci)
{
    const DegradedHdr* hdr = reinterpret_cast<const DegradedHdr*>(tab);
    DegBlock d;
    d.calc = calcb;
    d.par = parb;
    d.rest = tab + sizeof(DegradedHdr);
    d.r = d.rest + rest_bytes;
    d.h = d.r + (size_t)e * 8;
    d.pitch = pitch;
    d.nq = hdr->nq;
    d.nrest = hdr->nrest;
    d.rows = k + e;
    d.e = e;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        d.q[i] = hdr->q[i];
    unsigned long long sq = 0;
    for (int i = 0; i < d.nq; ++i) {
        const size_t off = (size_t)d.q[i] * d.pitch + ci;
        sq |= (unsigned long long)(uint8_t)(d.calc[off] ^ d.par[off]) << (8 * i);
    }
    int ps = -1;
    uint8_t ts = 0, t0 = 0, t2 = 0;
    for (int pi = 0; pi < d.nrest; ++pi) {
        const uint8_t t = deg_t(d, sq, pi, ci);
        if (pi == 0)
            t0 = t;
        if (ps < 0 && t) {
            ps = pi;
            ts = t;
        } else if (ps >= 0 && pi == ps + 1) {
            t2 = t;
        }
    }
    if (ps < 0)
        return -1;  // not a bad column
    // the screen: entry 0 (zero) when p* > 0, else entry 1 when there is one
    const int p2 = ps > 0 ? 0 : d.nrest > 1 ? 1 : -1;
    if (ps > 0)
        t2 = t0;
    int found = 0, row = -1;
    for (int r = 0; r < d.rows && found < 2; ++r) {
        const uint8_t* h = d.h + (size_t)r * d.e;
        const uint8_t hs = h[ps];
        if (!hs)
            continue;
        if (p2 >= 0 && gf_mul_slow(t2, hs) != gf_mul_slow(ts, h[p2]))
            continue;
        bool ok = true;
        for (int pi = 0; pi < d.nrest && ok; ++pi)
            ok = gf_mul_slow(deg_t(d, sq, pi, ci), hs) == gf_mul_slow(ts, h[pi]);
        if (ok) {
            ++found;
            row = r;
        }
    }
    return found == 1 ? row : -1;
}

// G: pivot syndromes a lane holds; W: dwords per lane and row.  Columns
// [col0, col1) in units of 16 bytes (W = 4) or bytes (W = 1).
template <int G, int W>
__global__ __launch_bounds__(kDegThreads) void k_degraded_compare(DegradedArgs a, long long col0, long long col1)
{
    extern __shared__ uint4 lt4[];  // [e][G] tables of bits 0-5, [e][G] dwords of bits 6-7, [e] rest rows
    uint32_t* ltc = reinterpret_cast<uint32_t*>(lt4 + (size_t)a.e * G);
    uint32_t* lrest = ltc + (size_t)a.e * G;
    const long long b = blockIdx.y;
    const uint8_t* tab = a.tab + (size_t)b * a.tab_stride;
    const DegradedHdr* hdr = reinterpret_cast<const DegradedHdr*>(tab);
    if (hdr->state != kDegRun)
        return;  // the whole workgroup: the prepare has reported this block
    const int nq = hdr->nq < G ? hdr->nq : G, nrest = hdr->nrest;
    const uint8_t* t_rest = tab + sizeof(DegradedHdr);
    const uint8_t* t_r = t_rest + a.rest_bytes;

    for (int idx = threadIdx.x; idx < nrest * G; idx += kDegThreads) {
        const int pi = idx / G, i = idx - pi * G;
        if (i < nq) {
            const uint8_t c = t_r[pi * 8 + i];
            lt4[idx] = a.tab4[c];
            ltc[idx] = a.tabc[c];
        }
    }
    for (int pi = threadIdx.x; pi < nrest; pi += kDegThreads)
        lrest[pi] = t_rest[pi];
    __syncthreads();

    const uint8_t* calcb = a.calc + b * a.e * a.pitch;
    const uint8_t* parb = a.par + b * a.e * a.pitch;
    const long long stride = (long long)gridDim.x * kDegThreads;
    unsigned long long bad = 0;
    unsigned hi1 = 0, lo1 = 0;

    for (long long col = col0 + (long long)blockIdx.x * kDegThreads + threadIdx.x; col < col1; col += stride) {
        // the pivot syndromes of this column as v_perm selectors
        uint32_t s0[G][W], s1[G][W], s2[G][W];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (i < nq) {
                const long long off = (long long)hdr->q[i] * a.pitch;
                const Col<W> x = col_load<W>(parb + off, col);
                const Col<W> y = col_load<W>(calcb + off, col);
#pragma unroll
                for (int w = 0; w < W; ++w)
                    sel_split(x.d[w] ^ y.d[w], s0[i][w], s1[i][w], s2[i][w]);
            }
        }
        // one walk over the rest rows, 2 kRestAhead loads in flight
        uint32_t any[W];
#pragma unroll
        for (int w = 0; w < W; ++w)
            any[w] = 0;
        for (int p0 = 0; p0 < nrest; p0 += kRestAhead) {
            Col<W> x[kRestAhead], y[kRestAhead];
#pragma unroll
            for (int q = 0; q < kRestAhead; ++q)
                if (p0 + q < nrest) {
                    const long long off = (long long)lrest[p0 + q] * a.pitch;
                    x[q] = col_load<W>(parb + off, col);
                    y[q] = col_load<W>(calcb + off, col);
                }
#pragma unroll
            for (int q = 0; q < kRestAhead; ++q) {
                if (p0 + q < nrest) {
                    const uint4* t4 = lt4 + (size_t)(p0 + q) * G;
                    const uint32_t* tc = ltc + (size_t)(p0 + q) * G;
                    uint32_t t[W];
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        t[w] = x[q].d[w] ^ y[q].d[w];
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        if (i < nq) {
                            const uint4 tt = t4[i];
                            const uint32_t c = tc[i];
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                t[w] ^= sel_mul(tt, c, s0[i][w], s1[i][w], s2[i][w]);
                        }
                    }
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        any[w] |= t[w];
                }
            }
        }
        uint32_t all = 0;
#pragma unroll
        for (int w = 0; w < W; ++w)
            all |= any[w];
        if (all == 0)
            continue;
        // the bad byte columns of this lane's column
#pragma unroll
        for (int w = 0; w < W; ++w) {
            for (int j = 0; j < (W == 4 ? 4 : 1); ++j) {
                if (((any[w] >> (8 * j)) & 0xFFu) == 0)
                    continue;
                ++bad;
                if (!a.locate)
                    continue;
                const long long ci = W == 4 ? col * 16 + w * 4 + j : col;
                const int row = deg_locate(tab, calcb, parb, a.pitch, a.k, a.e, (int)a.rest_bytes, ci);
                hi1 = max(hi1, row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
                lo1 = max(lo1, row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
            }
        }
    }
    scrub_fold_wave(reinterpret_cast<ScrubFold*>(a.report) + b, bad, hi1, lo1);
}

// the fold of every block the compare ran on into its report; the prepare's
// reports stay as they are
__global__ __launch_bounds__(256) void k_degraded_finalise(DegradedArgs a)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.blocks)
        return;
    const DegradedHdr* hdr = reinterpret_cast<const DegradedHdr*>(a.tab + (size_t)b * a.tab_stride);
    if (hdr->state != kDegRun)
        return;
    a.report[b] = scrub_verdict(reinterpret_cast<const ScrubFold*>(a.report)[b], a.locate);
}

template <int W>
hipError_t launch_w(const DegradedArgs& a, long long col0, long long col1, hipStream_t st)
{
    const dim3 grid(columns_grid_x(col1 - col0, a.blocks, kDegThreads), (unsigned)a.blocks), block(kDegThreads);
    const int most = a.u < a.e ? a.u : a.e;  // pivot rows of any block: |D| <= n <= min(u, e)
    const int g = lane_group(most);
    const size_t lds = lane_tables_lds(a.e, g, true);
    with_lane_group(g, [&](auto G) {
        hipLaunchKernelGGL((k_degraded_compare<decltype(G)::value, W>), grid, block, lds, st, a, col0, col1);
    });
    return hipGetLastError();
}

bool args_ok(const DegradedArgs& a)
{
    return a.blocks > 0 && a.blocks <= (long long)kMaxGridBlocks && a.k > 0 && a.e >= 0 &&
           a.k + a.e <= RSGPU_MAX_SOURCES && a.u >= 1 && a.u <= 8 && a.lost && a.tab && a.report &&
           a.tab_stride >= degraded_tab_stride(a.k, a.e);
}

}  // namespace

hipError_t launch_degraded_prepare(const DegradedArgs& a, hipStream_t st)
{
    if (!args_ok(a) || (a.work && !a.coef))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_degraded_prepare, dim3((unsigned)a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_degraded_compare(const DegradedArgs& a, bool bytes, long long col0, long long col1,
                                   hipStream_t st)
{
    if (!args_ok(a) || !a.work || !a.calc || !a.par || !a.tab4 || !a.tabc || col0 < 0 || col1 <= col0 ||
        col1 * (bytes ? 1 : 16) > a.len)
        return hipErrorInvalidValue;
    return bytes ? launch_w<1>(a, col0, col1, st) : launch_w<4>(a, col0, col1, st);
}

hipError_t launch_degraded_finalise(const DegradedArgs& a, hipStream_t st)
{
    if (!args_ok(a))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_degraded_finalise, dim3((unsigned)((a.blocks + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace rsgpu
