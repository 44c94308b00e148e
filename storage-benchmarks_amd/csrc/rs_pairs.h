// rs_pairs.h -- the pair search of rsgpu_correct_blocks (t == 2), the part of
// it that is one lane's: what a lane keeps of the pairs it meets, logarithms
// as the search keeps them, and the search itself for the gf_gen_rs_matrix
// codes, whose coefficients are c[p][r] = 2^(p r).  Shared by rs_correct.hip
// (k_correct_compare: the bookkeeping and the logarithms; its search reads any
// matrix from memory), rs_bitsliced.hip (k_rs_bs_correct) and the host
// (rsgpu_testhooks.cpp rsgpu_internal_rs_pair_search).  Nothing here crosses
// lanes: the ballots over the lanes' results and the write are the kernels'.
#pragma once
#include <stdint.h>

#include "gf256.h"

namespace rsgpu {

// Logarithms as the pair search keeps them: 16 bits, kLogZero for 0, so that a
// product is one read of `ex` at the sum of two of them -- ex[i] = 2^i below
// 510 (two real logarithms sum to 508 at the most) and 0 from there on.
constexpr unsigned kLogZero = 512;

// the field's tables of the search: 1284 bytes
struct PairGf {
    uint8_t log[256];
    uint8_t ex[2 * kLogZero + 4];
};

// byte i of a PairGf, from the field's tables
RS_HD inline uint8_t pair_gf_byte(const GfTables& gf, int i)
{
    return i < 256 ? gf.log[i] : i - 256 < 510 ? gf.exp[i - 256] : 0;
}

// what the search keeps of a data row r per column
struct CorRow {
    uint16_t a0, a1;  // log of s_2 c[0][r] and of s_2 c[1][r]
    uint16_t c2, u;   // log of c[2][r] and of u_r = s_0 c[1][r] ^ s_1 c[0][r]
};

// what a lane has found of a column's pairs
struct CorPairs {
    int cnt, ra, rb;  // matching pairs (up to 2); the first one, xa in row ra and xb in row rb
    uint8_t xa, xb;
};

RS_HD inline void pair_found(CorPairs& c, int ra, int rb, uint8_t xa, uint8_t xb)
{
    if (c.cnt == 0) {
        c.ra = ra;
        c.rb = rb;
        c.xa = xa;
        c.xb = xb;
    }
    c.cnt = c.cnt + 1 < 2 ? c.cnt + 1 : 2;
}

RS_HD inline unsigned pair_log(const PairGf& g, uint8_t v) { return v ? g.log[v] : kLogZero; }

// the sum of two real logarithms, or kLogZero, below 255 (a factor's logarithm)
RS_HD inline unsigned cor_log_mul(unsigned la, unsigned lb)
{
    const unsigned l = la + lb;
    return l >= kLogZero ? kLogZero : l >= 255 ? l - 255 : l;
}

// log c[p][r] of the gf_gen_rs_matrix codes
RS_HD inline unsigned rs_log_coef(int p, int r) { return (unsigned)(p * r) % 255u; }

// Row r of a column with syndromes s_0, s_1, s_2 for the search below:
// log c[0][r] = 0, log c[1][r] = r, log c[2][r] = 2 r mod 255.
RS_HD inline CorRow rs_pair_row(const PairGf& g, uint8_t s0, uint8_t s1, uint8_t s2, int r)
{
    const unsigned ls2 = pair_log(g, s2);
    CorRow row;
    row.a0 = (uint16_t)ls2;
    row.a1 = (uint16_t)cor_log_mul(ls2, (unsigned)r);
    row.c2 = (uint16_t)rs_log_coef(2, r);
    row.u = (uint16_t)pair_log(g, (uint8_t)(g.ex[pair_log(g, s0) + (unsigned)r] ^ s1));
    return row;
}

// What lane `lane` of 64 finds of the pairs {a, b} with syn = x h_a + y h_b, x
// and y non-zero, for a gf_gen_rs_matrix code (k, e), 3 <= e <= 64, k <= 255;
// syn: the column's e syndromes, row: rs_pair_row of every data row.  The
// search of rs_correct.hip's head, every pair met by exactly one lane:
//   two parity rows            lane 0
//   a data row, a parity row   the lane of r mod 64
//   two data rows a < b        the lane of b mod 64
// (The loops stay rolled: the fused kernels have no registers to unroll into.)
RS_HD inline CorPairs rs_pair_search_lane(const PairGf& g, int k, int e, const uint8_t* syn, const CorRow* row,
                                          int lane)
{
    CorPairs c{};
    const uint8_t s0 = syn[0], s1 = syn[1];
    const unsigned ls0 = pair_log(g, s0), ls1 = pair_log(g, s1);

    if (lane == 0) {  // the column's only non-zero syndromes are s_p and s_q
        int nz = 0, p = 0, q = 0;
#pragma unroll 1
        for (int i = 0; i < e; ++i)
            if (syn[i]) {
                p = nz == 0 ? i : p;
                q = i;
                ++nz;
            }
        if (nz == 2)
            pair_found(c, k + p, k + q, syn[p], syn[q]);
    }

    for (int r = lane; r < k; r += 64) {
        if (s0) {  // parity row k + p, p >= 1: x = s_0 fails at exactly one q, which is p
            const unsigned lx = ls0;
            int miss = 0, p = 0;
#pragma unroll 1
            for (int q = 1; q < e && miss < 2; ++q)
                if (syn[q] != g.ex[rs_log_coef(q, r) + lx]) {
                    ++miss;
                    p = q;
                }
            if (miss == 1)
                pair_found(c, r, k + p, s0, (uint8_t)(syn[p] ^ g.ex[rs_log_coef(p, r) + lx]));
        }
        if (s1) {  // parity row k: x = s_1 / c[1][r] holds at every q >= 2
            const unsigned lx = cor_log_mul(ls1, 255u - (unsigned)r);
            bool ok = true;
#pragma unroll 1
            for (int q = 2; q < e && ok; ++q)
                ok = syn[q] == g.ex[rs_log_coef(q, r) + lx];
            const uint8_t y = (uint8_t)(s0 ^ g.ex[lx]);
            if (ok && y)
                pair_found(c, r, k, g.ex[lx], y);
        }
    }

    for (int rb = lane; rb < k; rb += 64) {
        const CorRow b = row[rb];
#pragma unroll 1
        for (int ra = 0; ra < rb && b.u != kLogZero; ++ra) {
            const CorRow a = row[ra];
            // coordinate 2: det s_2 ^ c[2][ra] u_rb ^ c[2][rb] u_ra, det = 2^rb ^ 2^ra
            if ((g.ex[a.a0 + (unsigned)rb] ^ g.ex[a.a1] ^ g.ex[a.c2 + b.u] ^ g.ex[b.c2 + a.u]) != 0 ||
                a.u == kLogZero)
                continue;
            const unsigned ld = g.log[g.ex[ra] ^ g.ex[rb]];  // ra != rb below 255: never 0
            const uint8_t x = g.ex[b.u + 255u - ld], y = g.ex[a.u + 255u - ld];
            bool ok = true;
#pragma unroll 1
            for (int p = 3; p < e && ok; ++p)
                ok = syn[p] == (g.ex[rs_log_coef(p, ra) + g.log[x]] ^ g.ex[rs_log_coef(p, rb) + g.log[y]]);
            if (ok)
                pair_found(c, ra, rb, x, y);
        }
    }
    return c;
}

}  // namespace rsgpu
