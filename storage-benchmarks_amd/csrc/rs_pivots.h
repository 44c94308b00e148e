// rs_pivots.h -- what the prepare kernels of the degraded scrub
// (rs_degraded.hip k_degraded_prepare) and of the rebuild (rs_rebuild.hip
// k_rebuild_prepare) share: the judgement of a block's list of lost rows, the
// greedy choice of the pivot parity rows Q for its lost data rows D, and the
// inverse of c[Q][D].  The bound on |D| is a compile-time N.  With N = 8 (the
// degraded scrub, the narrow rebuild prepare) one lane of a wave runs them on a
// PivotWork in LDS and the other lanes read the result after a barrier.  With
// N = 32 (the wide rebuild prepare) the whole wave runs them on a PivotWave, a
// column of the matrix per lane: lost_pivots_wave.  Internal to librsgpu's
// .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsgpu.h"
#include "gf256.h"

namespace rsgpu {

// a^-1 = a^254
__device__ inline uint8_t deg_inv(uint8_t a)
{
    uint8_t r = 1, s = a;
    for (int bit = 1; bit < 8; ++bit) {  // 254 = 0b11111110
        s = gf_mul_slow(s, s);
        r = gf_mul_slow(r, s);
    }
    return r;
}

template <int N>
struct PivotWorkN {
    uint8_t lost[256];    // per row of [0, k + e): 1 when listed; zeroed by the caller
    uint8_t dl[N], ql[N]; // D (data rows), Q (parity indices), both ascending
    uint8_t basis[N][N];  // echelon form of the rows kept so far
    uint8_t bpiv[N];      // pivot column of each basis row
    uint8_t am[N][N], inv[N][N];  // inv = (c[Q][D])^-1
};
using PivotWork = PivotWorkN<8>;

// The list of a block: u entries, rows in [0, m) strictly ascending, then
// only RSGPU_LOST_NONE.  Returns the number of listed rows, or -1 for a
// malformed list (more than e rows included).
__device__ inline int lost_list_rows(const uint8_t* list, int u, int m, int e)
{
    int n = 0, prev = -1;
    bool ok = true, none = false;
    for (int i = 0; i < u; ++i) {
        const int j = list[i];
        if (j == RSGPU_LOST_NONE) {
            none = true;
        } else {
            ok = ok && !none && j < m && j > prev;
            prev = j;
            ++n;
        }
    }
    return ok && n <= e ? n : -1;
}

// Marks the n rows of `rows` in w.lost, splits off the data rows D (w.dl),
// chooses the pivot rows greedily (ascending surviving parity rows, each kept
// when it raises the rank of c[Q][D]; w.ql) and inverts c[Q][D] by
// Gauss-Jordan (w.inv).  Returns |D|, or -1 when the surviving parity rows do
// not determine D.  coef: the e x k matrix.
template <int N>
__device__ inline int lost_pivots(PivotWorkN<N>& w, const uint8_t* rows, int n, const uint8_t* coef, int k, int e)
{
    int nd = 0;
    for (int i = 0; i < n; ++i) {
        const int j = rows[i];
        w.lost[j] = 1;
        if (j < k)
            w.dl[nd++] = (uint8_t)j;
    }
    // greedy pivots: reduce each surviving parity row's c[p][D] by the
    // basis; what is left non-zero raises the rank
    int nq = 0;
    for (int p = 0; p < e && nq < nd; ++p) {
        if (w.lost[k + p])
            continue;
        uint8_t v[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
            v[i] = i < nd ? coef[(size_t)p * k + w.dl[i < nd ? i : 0]] : 0;
        for (int q = 0; q < nq; ++q) {
            uint8_t f = 0;
#pragma unroll
            for (int i = 0; i < N; ++i)
                f = i == w.bpiv[q] ? v[i] : f;
            if (f) {
#pragma unroll
                for (int i = 0; i < N; ++i)
                    v[i] ^= gf_mul_slow(f, w.basis[q][i]);
            }
        }
        int piv = -1;
#pragma unroll
        for (int i = N - 1; i >= 0; --i)
            piv = v[i] ? i : piv;
        if (piv < 0)
            continue;
        uint8_t lead = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
            lead = i == piv ? v[i] : lead;
        const uint8_t li = deg_inv(lead);
#pragma unroll
        for (int i = 0; i < N; ++i)
            w.basis[nq][i] = gf_mul_slow(li, v[i]);
        w.bpiv[nq] = (uint8_t)piv;
        w.ql[nq++] = (uint8_t)p;
    }
    if (nq < nd)
        return -1;
    // (c[Q][D])^-1 by Gauss-Jordan; the matrix has full rank
    for (int i = 0; i < nd; ++i)
        for (int j = 0; j < nd; ++j) {
            w.am[i][j] = coef[(size_t)w.ql[i] * k + w.dl[j]];
            w.inv[i][j] = i == j;
        }
    for (int col = 0; col < nd; ++col) {
        int pr = col;
        while (pr < nd && w.am[pr][col] == 0)
            ++pr;
        if (pr >= nd)
            break;  // cannot happen for a full-rank matrix
        if (pr != col)
            for (int j = 0; j < nd; ++j) {
                const uint8_t x = w.am[pr][j], y = w.inv[pr][j];
                w.am[pr][j] = w.am[col][j];
                w.inv[pr][j] = w.inv[col][j];
                w.am[col][j] = x;
                w.inv[col][j] = y;
            }
        const uint8_t li = deg_inv(w.am[col][col]);
        for (int j = 0; j < nd; ++j) {
            w.am[col][j] = gf_mul_slow(li, w.am[col][j]);
            w.inv[col][j] = gf_mul_slow(li, w.inv[col][j]);
        }
        for (int r = 0; r < nd; ++r) {
            const uint8_t f = w.am[r][col];
            if (r == col || f == 0)
                continue;
            for (int j = 0; j < nd; ++j) {
                w.am[r][j] ^= gf_mul_slow(f, w.am[col][j]);
                w.inv[r][j] ^= gf_mul_slow(f, w.inv[col][j]);
            }
        }
    }
    return nd;
}

// The same on a whole wave of 64 lanes, for bounds where an N^3 chain of
// gf_mul_slow on one lane would cost milliseconds: lane i holds column i of
// the row being reduced, and the Gauss-Jordan runs on the augmented matrix
// [c[Q][D] | I], its 2 N <= 64 columns one per lane.
template <int N>
struct PivotWave {
    uint8_t lost[256];     // per row of [0, k + e): 1 when listed; zeroed by the caller
    uint8_t dl[N], ql[N];  // D (data rows), Q (parity indices), both ascending
    uint8_t basis[N][N];   // echelon form of the rows kept so far
    uint8_t bpiv[N];       // pivot column of each basis row
    uint8_t aug[N][2 * N]; // [c[Q][D] | I] on the way to [I | (c[Q][D])^-1]
    uint8_t fcol[N];       // the column being cleared
    int nd;
    __device__ uint8_t inv(int i, int q) const { return aug[i][N + q]; }
};

// Every lane of the (one-wave) workgroup calls this with the same arguments;
// `rows` is visible to all of them.  Result and return value as lost_pivots,
// the inverse in w.inv(i, q).  The greedy choice is the same set Q: whether a
// row raises the rank does not depend on how the basis is kept.
template <int N>
__device__ inline int lost_pivots_wave(PivotWave<N>& w, const uint8_t* rows, int n, const uint8_t* coef, int k,
                                       int e, int lane)
{
    static_assert(2 * N <= 64, "the augmented matrix has a column per lane");
    if (lane == 0) {
        int nd0 = 0;
        for (int i = 0; i < n; ++i) {
            const int j = rows[i];
            w.lost[j] = 1;
            if (j < k)
                w.dl[nd0++] = (uint8_t)j;
        }
        w.nd = nd0;
    }
    __syncthreads();
    const int nd = w.nd;
    const int dcol = lane < nd ? w.dl[lane] : 0;
    int nq = 0;
    for (int p = 0; p < e && nq < nd; ++p) {
        if (w.lost[k + p])
            continue;
        int v = lane < nd ? coef[(size_t)p * k + dcol] : 0;
        for (int q = 0; q < nq; ++q) {
            const int f = __shfl(v, (int)w.bpiv[q]);
            if (f && lane < nd)
                v ^= gf_mul_slow((uint8_t)f, w.basis[q][lane]);
        }
        const unsigned long long nz = __ballot(v != 0);
        if (nz == 0)
            continue;
        const int piv = __ffsll((long long)nz) - 1;
        const uint8_t li = deg_inv((uint8_t)__shfl(v, piv));
        if (lane < N)
            w.basis[nq][lane] = gf_mul_slow(li, (uint8_t)v);
        if (lane == 0) {
            w.bpiv[nq] = (uint8_t)piv;
            w.ql[nq] = (uint8_t)p;
        }
        ++nq;
        __syncthreads();
    }
    if (nq < nd)
        return -1;
    const int j = lane & (N - 1);
    for (int i = 0; i < nd; ++i)
        w.aug[i][lane] = lane < N ? (j < nd ? coef[(size_t)w.ql[i] * k + w.dl[j]] : 0) : (uint8_t)(j == i);
    __syncthreads();
    for (int col = 0; col < nd; ++col) {
        int pr = col;
        while (pr < nd && w.aug[pr][col] == 0)
            ++pr;
        if (pr >= nd)
            break;  // cannot happen for a full-rank matrix
        const uint8_t li = deg_inv(w.aug[pr][col]);
        const uint8_t x = w.aug[pr][lane], y = w.aug[col][lane];
        const uint8_t prow = gf_mul_slow(li, x);
        __syncthreads();  // the pivot is read before its column's lane writes
        w.aug[pr][lane] = y;
        w.aug[col][lane] = prow;
        __syncthreads();
        if (lane < nd)
            w.fcol[lane] = w.aug[lane][col];
        __syncthreads();
        for (int r = 0; r < nd; ++r) {
            const uint8_t f = w.fcol[r];
            if (r != col && f)
                w.aug[r][lane] ^= gf_mul_slow(f, prow);
        }
        __syncthreads();
    }
    return nd;
}

}  // namespace rsgpu
