// plane_mul.h -- a run-time GF(2^8) constant times eight bit-planes (host +
// device).  Plane a holds bit a of 32 bytes (bitslice.h tr8); the product by c
// is GF(2)-linear, the 8 x 8 bit matrix whose column a is c 2^a: plane b of
// c x is the XOR of the planes a of x for which bit b of c 2^a is set.  The
// matrix is built from the byte with scalar code (c is wave-uniform where the
// kernels call this: the masks are SGPRs of 0 or ~0) and applied as masked
// XORs, one v_bitop3 per (a, b); no table per lane.  k_rs_bs_degraded reduces
// its syndromes with it (rs_bitsliced.hip degraded_tile); the CPU suite checks
// it against gf_mul through the test-hooks library.
#pragma once
#include <stdint.h>

#include "gf256.h"

namespace rsgpu {

// t ^= c * s, on planes
RS_HD inline void plane_mul_acc(uint32_t (&t)[8], const uint32_t (&s)[8], uint32_t c)
{
    uint32_t x = c & 0xFFu;  // c 2^a
#pragma unroll
    for (int a = 0; a < 8; ++a) {
#pragma unroll
        for (int b = 0; b < 8; ++b)
            t[b] ^= s[a] & (0u - ((x >> b) & 1u));
        x = ((x << 1) ^ ((x & 0x80u) ? 0x1Du : 0u)) & 0xFFu;
    }
}

}  // namespace rsgpu
