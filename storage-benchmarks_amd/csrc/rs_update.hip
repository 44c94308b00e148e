// rs_update.hip -- partial-stripe update of parity (rsgpu_update_blocks) for
// gfx950: a caller overwrites a few of a block's k source rows, and the e
// parity rows follow by
//   parity[p][x] ^= XOR_i c[p][j_i] * delta_i[x],   delta_i = new_i ^ old_i
// (ISA-L's ec_encode_data_update algebra, isa/ec_base.c:307-321, batched and
// device-resident).
//
// The path is built for traffic, not arithmetic.  A workgroup owns one block
// and a strided set of columns; a lane owns its 16-byte column (a byte in the
// byte kernel) of every row it touches, so there are no atomics and no order
// between workgroups.  Per group of up to G <= 8 listed rows the lane
//   1. loads the update rows (and, unless they already are deltas, the old
//      source rows, which it overwrites with the new contents) -- once each,
//   2. keeps the deltas in registers as the three v_perm index dwords of the
//      3-3-2 split (bits 0-2, 3-5, 6-7 of every byte),
//   3. walks the e parity rows once: load, XOR the <= G products, store.
// So for u <= 8 every parity byte is read once and written once; a list of
// more rows takes ceil(n / 8) such walks.
//
// One kernel serves every matrix: the coefficient of (p, i) is read from the
// device-resident e x k matrix through the block's own list, and its v_perm
// tables (gf256.h perm_tables, a function of the coefficient's value alone)
// come from one 256-entry device table.  A workgroup stages the e x G entries
// of a group in LDS; the lanes read them as wave-uniform broadcasts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsgpu.h"
#include "rs_kernels.h"
#include "rs_lane.h"

namespace rsgpu {

namespace {

constexpr int kUpdThreads = 256;
constexpr int kParityAhead = 4;  // parity rows loaded before the first is stored

// G: deltas a lane holds (the group size); W: dwords per lane and row.
// Columns [col0, col1) in units of W * 4 bytes (W = 4) or bytes (W = 1).
template <int G, int W>
__global__ __launch_bounds__(kUpdThreads) void k_update_blocks(UpdateArgs a, long long col0, long long col1)
{
    extern __shared__ uint4 lt4[];  // [e][G] tables of bits 0-5, then [e][G] dwords of bits 6-7
    uint32_t* ltc = reinterpret_cast<uint32_t*>(lt4 + (size_t)a.e * G);
    const long long b = blockIdx.y;
    const uint8_t* cols = a.cols + b * a.u;

    // the list: rows in [0, k) strictly ascending, then only NONE
    int n = 0, prev = -1;
    bool ok = true, none = false;
    for (int i = 0; i < a.u; ++i) {
        const int j = cols[i];
        if (j == RSGPU_UPDATE_NONE) {
            none = true;
        } else {
            ok = ok && !none && j < a.k && j > prev;
            prev = j;
            ++n;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.status != nullptr)
        a.status[b] = ok ? 0 : -2;
    if (!ok || n == 0)
        return;  // the whole workgroup: nothing of this block is touched

    const uint8_t* updb = a.upd + b * a.u * a.pitch;
    uint8_t* srcb = a.delta ? nullptr : a.src + b * a.k * a.pitch;
    uint8_t* parb = a.par + b * a.e * a.pitch;
    const long long stride = (long long)gridDim.x * kUpdThreads;

    for (int i0 = 0; i0 < n; i0 += G) {
        const int gn = n - i0 < G ? n - i0 : G;
        if (a.e > 0) {
            if (i0 > 0)
                __syncthreads();  // the previous group's readers are done
            for (int idx = threadIdx.x; idx < a.e * G; idx += kUpdThreads) {
                const int p = idx / G, i = idx - p * G;
                if (i < gn) {
                    const uint8_t c = a.coef[(size_t)p * a.k + cols[i0 + i]];
                    lt4[idx] = a.tab4[c];
                    ltc[idx] = a.tabc[c];
                }
            }
            __syncthreads();
        }
        for (long long col = col0 + (long long)blockIdx.x * kUpdThreads + threadIdx.x; col < col1; col += stride) {
            // the deltas of this column as v_perm selectors
            uint32_t s0[G][W], s1[G][W], s2[G][W];
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if (i < gn) {
                    Col<W> x = col_load<W>(updb + (long long)(i0 + i) * a.pitch, col);
                    if (!a.delta) {
                        uint8_t* row = srcb + (long long)cols[i0 + i] * a.pitch;
                        const Col<W> old = col_load<W>(row, col);
                        col_store<W>(row, col, x);
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            x.d[w] ^= old.d[w];
                    }
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        sel_split(x.d[w], s0[i][w], s1[i][w], s2[i][w]);
                }
            }
            // one walk over the parity rows, kParityAhead loads in flight
            for (int p0 = 0; p0 < a.e; p0 += kParityAhead) {
                Col<W> acc[kParityAhead];
#pragma unroll
                for (int q = 0; q < kParityAhead; ++q)
                    if (p0 + q < a.e)
                        acc[q] = col_load<W>(parb + (long long)(p0 + q) * a.pitch, col);
#pragma unroll
                for (int q = 0; q < kParityAhead; ++q) {
                    if (p0 + q < a.e) {
                        const uint4* t4 = lt4 + (size_t)(p0 + q) * G;
                        const uint32_t* tc = ltc + (size_t)(p0 + q) * G;
#pragma unroll
                        for (int i = 0; i < G; ++i) {
                            if (i < gn) {
                                const uint4 t = t4[i];
                                const uint32_t c = tc[i];
#pragma unroll
                                for (int w = 0; w < W; ++w)
                                    acc[q].d[w] ^= sel_mul(t, c, s0[i][w], s1[i][w], s2[i][w]);
                            }
                        }
                        col_store<W>(parb + (long long)(p0 + q) * a.pitch, col, acc[q]);
                    }
                }
            }
        }
    }
}

template <int W>
hipError_t launch_w(const UpdateArgs& a, long long col0, long long col1, hipStream_t st)
{
    const dim3 grid(columns_grid_x(col1 - col0, a.blocks, kUpdThreads), (unsigned)a.blocks), block(kUpdThreads);
    const int g = lane_group(a.u);
    const size_t lds = lane_tables_lds(a.e, g, false);
    with_lane_group(g, [&](auto G) {
        hipLaunchKernelGGL((k_update_blocks<decltype(G)::value, W>), grid, block, lds, st, a, col0, col1);
    });
    return hipGetLastError();
}

}  // namespace

int update_group_rows() { return 8; }

hipError_t launch_update_blocks(const UpdateArgs& a, bool bytes, long long col0, long long col1, hipStream_t st)
{
    return bytes ? launch_w<1>(a, col0, col1, st) : launch_w<4>(a, col0, col1, st);
}

}  // namespace rsgpu
