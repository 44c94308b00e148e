// rs_pairs.h -- the pair search of rsgpu_correct_blocks (t == 2), the part of
// it that is one lane's: what a lane keeps of the pairs it meets, logarithms
// as the search keeps them, and the search itself for the gf_gen_rs_matrix
// codes, whose coefficients are c[p][r] = 2^(p r).  Shared by rs_correct.hip
// (k_correct_compare: the bookkeeping and the logarithms; its search reads any
// matrix from memory), rs_bitsliced.hip (k_rs_bs_correct) and the host
// (rsgpu_testhooks.cpp rsgpu_internal_rs_pair_search); below it the search for
// a matrix read from memory, shared by rs_jit.hip (k_rs_jit_correct,
// k_rs_jitw_correct) and the host (rsgpu_internal_pair_search).  Nothing here
// crosses lanes: the ballots over the lanes' results and the write are the
// kernels'.
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

// ---------------------------------------------------------------------------
// The same search for a matrix read from memory (rs_correct.hip's head): what
// k_rs_jit_correct / k_rs_jitw_correct (rs_jit.hip) and the host
// (rsgpu_testhooks.cpp rsgpu_internal_pair_search) run per lane.  The tables
// come as pointers of the caller's own kind -- LDS pointers in the kernels,
// plain ones on the host -- so every read is of a scalar member.
// ---------------------------------------------------------------------------

// Rows 0 to 2 of the matrix as the search keeps them, a byte per data row: the
// logarithm, 255 for a coefficient 0 (rows 0 and 1 of a locatable matrix have
// none).
constexpr unsigned kLog8Zero = 255;
RS_HD inline uint8_t pair_log8(const GfTables& gf, uint8_t v) { return v ? gf.log[v] : (uint8_t)kLog8Zero; }
RS_HD inline unsigned pair_log8_wide(unsigned l) { return l == kLog8Zero ? kLogZero : l; }

template <class GP>
RS_HD inline unsigned pair_logp(GP g, uint8_t v)
{
    return v ? g->log[v] : kLogZero;
}

// Row r of a column whose syndromes 0 to 2 have the logarithms ls0, ls1, ls2
// (pair_logp), l0 l1 l2 being the row's bytes of the three logarithm rows.
template <class GP>
RS_HD inline CorRow pair_row(GP g, unsigned ls0, unsigned ls1, unsigned ls2, unsigned l0, unsigned l1, unsigned l2)
{
    CorRow row;
    row.a0 = (uint16_t)cor_log_mul(ls2, l0);
    row.a1 = (uint16_t)cor_log_mul(ls2, l1);
    row.c2 = (uint16_t)pair_log8_wide(l2);
    // u_r = s_0 c[1][r] ^ s_1 c[0][r]
    row.u = (uint16_t)pair_logp(g, (uint8_t)(g->ex[ls0 + l1] ^ g->ex[ls1 + l0]));
    return row;
}

// What a lane has found, in two registers: cnt = the matching pairs so far (up
// to 2) | xb << 8, first = ra | rb << 9 | xa << 18 of the first one (rows below
// 512).
struct PairHits {
    unsigned cnt, first;
};

RS_HD inline void pair_hit(PairHits& h, unsigned ra, unsigned rb, unsigned xa, unsigned xb)
{
    const unsigned n = h.cnt & 3u;
    h.first = n == 0 ? (ra | rb << 9 | xa << 18) : h.first;
    h.cnt = (n == 0 ? xb << 8 : h.cnt & ~3u) | (n + 1 < 2 ? n + 1 : 2u);
}

RS_HD inline CorPairs pair_hits(const PairHits& h)
{
    CorPairs c{};
    c.cnt = (int)(h.cnt & 3u);
    c.ra = (int)(h.first & 511u);
    c.rb = (int)(h.first >> 9 & 511u);
    c.xa = (uint8_t)(h.first >> 18);
    c.xb = (uint8_t)(h.cnt >> 8);
    return c;
}

// What lane `lane` of 64 finds of the pairs {a, b} with syn = x h_a + y h_b, x
// and y non-zero, for the e x k matrix coef of a locatable code, 3 <= e <= 64,
// k <= 255.  syn[p * stride]: the column's syndrome p; l0, l1, l2 [k]: rows 0
// to 2 of coef as pair_log8 gives them; row [k]: pair_row of every data row for
// this column.  Every pair is met by exactly one lane, as in
// rs_pair_search_lane; survivors of the screen at syndrome 2 are verified
// coordinate by coordinate against coef.  uni(v): v, which is the same in
// every lane -- the kernels pass a readfirstlane, so that what is read at one
// address for all lanes lives in a scalar register.  (The wide generated
// kernels leave the compiler 40 VGPRs, and the search runs inside their cold
// path's walk: the loops stay rolled, the lane's matches are two registers,
// the matrix is read through a 32-bit index.)
template <class GP, class SP, class LP, class RP, class CP, class UNI>
RS_HD inline PairHits pair_search_lane(GP g, int k, int e, SP syn, int stride, LP l0, LP l1, LP l2, RP row, CP coef,
                                       int lane, UNI uni)
{
    PairHits h{0, 0};
    const unsigned s0 = uni(syn[0]), s1 = uni(syn[stride]);
    const unsigned ls0 = uni(pair_logp(g, (uint8_t)s0)), ls1 = uni(pair_logp(g, (uint8_t)s1));

    if (lane == 0) {  // the column's only non-zero syndromes are s_p and s_q
        unsigned nz = 0, p = 0, q = 0;
#pragma unroll 1
        for (int i = 0; i < e; ++i)
            if (syn[i * stride]) {
                p = nz == 0 ? (unsigned)i : p;
                q = (unsigned)i;
                ++nz;
            }
        if (nz == 2)
            pair_hit(h, (unsigned)k + p, (unsigned)k + q, syn[p * stride], syn[q * stride]);
    }

    // a data row and a parity row: syndromes 1 and 2 from the logarithm rows,
    // the others, for the few rows that get there, from the matrix
#pragma unroll 1
    for (int r = lane; r < k; r += 64) {
        if (s0) {  // parity row k + p, p >= 1: x = s_0 / c[0][r] fails at exactly one q, which is p
            const unsigned lx = cor_log_mul(ls0, 255u - l0[r]);
            unsigned miss = 0, p = 0;
            if (syn[stride] != g->ex[l1[r] + lx]) {
                ++miss;
                p = 1;
            }
            if (syn[2 * stride] != g->ex[pair_log8_wide(l2[r]) + lx]) {
                ++miss;
                p = 2;
            }
#pragma unroll 1
            for (int q = 3; q < e && miss < 2; ++q)
                if (syn[q * stride] != g->ex[pair_logp(g, coef[(unsigned)(q * k + r)]) + lx]) {
                    ++miss;
                    p = (unsigned)q;
                }
            if (miss == 1) {
                const unsigned cp = p == 1 ? l1[r] : p == 2 ? pair_log8_wide(l2[r])
                                                            : pair_logp(g, coef[(unsigned)((int)p * k + r)]);
                pair_hit(h, (unsigned)r, (unsigned)k + p, g->ex[lx], (unsigned)(syn[p * stride] ^ g->ex[cp + lx]));
            }
        }
        if (s1) {  // parity row k: x = s_1 / c[1][r] holds at every q >= 2
            const unsigned lx = cor_log_mul(ls1, 255u - l1[r]);
            bool ok = syn[2 * stride] == g->ex[pair_log8_wide(l2[r]) + lx];
#pragma unroll 1
            for (int q = 3; q < e && ok; ++q)
                ok = syn[q * stride] == g->ex[pair_logp(g, coef[(unsigned)(q * k + r)]) + lx];
            const unsigned y = s0 ^ g->ex[l0[r] + lx];
            if (ok && y)
                pair_hit(h, (unsigned)r, (unsigned)k, g->ex[lx], y);
        }
    }

    // two data rows: a lane per rb in bands of 64, every ra below it
#pragma unroll 1
    for (int rb = lane; rb < k; rb += 64) {
        const unsigned bu = row[rb].u;
        if (bu == kLogZero)
            continue;
#pragma unroll 1
        for (int ra = 0; ra < rb; ++ra) {
            const unsigned au = uni(row[ra].u);
            // coordinate 2: det s_2 ^ c[2][ra] u_rb ^ c[2][rb] u_ra
            if (au == kLogZero || (g->ex[uni(row[ra].a0) + l1[rb]] ^ g->ex[uni(row[ra].a1) + l0[rb]] ^
                                   g->ex[uni(row[ra].c2) + bu] ^ g->ex[row[rb].c2 + au]) != 0)
                continue;
            const unsigned det = g->ex[uni(l0[ra]) + l1[rb]] ^ g->ex[uni(l1[ra]) + l0[rb]];
            if (!det)
                continue;
            // x = u_rb / det, y = u_ra / det: non-zero, as u_ra and u_rb are
            const unsigned ld = 255u - g->log[det];
            const unsigned lx = g->log[g->ex[bu + ld]], ly = g->log[g->ex[au + ld]];
            bool ok = true;
#pragma unroll 1
            for (int p = 3; p < e && ok; ++p)
                ok = syn[p * stride] == (uint8_t)(g->ex[pair_logp(g, coef[(unsigned)(p * k + ra)]) + lx] ^
                                                  g->ex[pair_logp(g, coef[(unsigned)(p * k + rb)]) + ly]);
            if (ok)
                pair_hit(h, (unsigned)ra, (unsigned)rb, g->ex[lx], g->ex[ly]);
        }
    }
    return h;
}

}  // namespace rsgpu
