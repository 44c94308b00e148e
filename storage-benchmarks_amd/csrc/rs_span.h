// rs_span.h -- the wave-cooperative span arithmetic of the locate
// (rsgpu_locate_blocks): an echelon basis of at most RSGPU_LOCATE_MAX_ROWS
// vectors of GF(2^8)^64 in LDS, a lane per coordinate.  Shared by
// rs_locate.hip (k_locate_span, k_locate_finish; rs_correct.hip takes the
// lane helpers), rs_bitsliced.hip
// (k_rs_bs_locate) and rs_jit.hip (k_rs_jit_locate, k_rs_jitw_locate): one copy of the basis, the slot format, the reduction and
// the append.  The merge of a workgroup's bases into its slot (span_publish) is
// k_rs_bs_locate's; k_locate_span has the same steps written out, which keeps
// its instructions what they were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"

namespace rsgpu {

constexpr int kLocMax = RSGPU_LOCATE_MAX_ROWS;

// a basis in reduced echelon form: vector i is 1 at coordinate piv[i], its
// lowest non-zero one, and every other vector is 0 there
struct SpanBasis {
    uint8_t v[kLocMax][64];
    int piv[kLocMax];
    int n, ovf;  // vectors held; a vector outside the span met a full basis
};

// what a workgroup leaves of its columns: [n, ovf, pad | n vectors of 64 bytes]
struct SlotHdr {
    int n, ovf, pad[2];
};
static_assert(sizeof(SlotHdr) + kLocMax * 64 == kLocateSlotBytes, "slot layout");

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ uint8_t lane_byte(uint8_t v, int l)
{
    return (uint8_t)__builtin_amdgcn_readlane((int)v, l);
}

__device__ __forceinline__ uint8_t loc_mul(const GfTables& gf, uint8_t a, uint8_t b)
{
    return a && b ? gf.exp[gf.log[a] + gf.log[b]] : 0;
}

// a / b, b != 0
__device__ __forceinline__ uint8_t loc_div(const GfTables& gf, uint8_t a, uint8_t b)
{
    return a ? gf.exp[gf.log[a] + 255 - gf.log[b]] : 0;
}

// the tables `from` (device memory) into the workgroup's LDS copy
__device__ __forceinline__ void load_gf(GfTables& gf, const GfTables& from, int t, int threads)
{
    for (int i = t; i < 512; i += threads)
        gf.exp[i] = from.exp[i];
    for (int i = t; i < 256; i += threads)
        gf.log[i] = from.log[i];
}

// The wave's vector v (lane = coordinate) minus its components along the
// basis.  The basis is reduced, so every factor is read from v itself: one
// cross-lane read and one multiply per lane and step.  Whole wave, uniform
// control.
__device__ __forceinline__ uint8_t span_reduce(const SpanBasis& s, const GfTables& gf, int lane, uint8_t v)
{
    const int n = uni(s.n);
    uint8_t r = v;
    for (int i = 0; i < n; ++i) {
        const uint8_t f = lane_byte(v, uni(s.piv[i]));
        if (f)
            r ^= loc_mul(gf, f, s.v[i][lane]);
    }
    return r;
}

// r: a residual of span_reduce.  Zero: nothing.  Otherwise it is normalised at
// its lowest non-zero coordinate, cleared out of the vectors held and appended;
// with `cap` vectors held it raises ovf instead.  Whole wave, uniform control;
// the values that are the same in every lane are stored by every lane.
__device__ __forceinline__ void span_append(SpanBasis& s, const GfTables& gf, int lane, uint8_t r, int cap)
{
    const unsigned long long nz = __ballot(r != 0);
    if (!nz)
        return;
    const int n = uni(s.n);
    if (n >= cap) {
        s.ovf = 1;
        return;
    }
    const int pv = __ffsll(nz) - 1;
    const uint8_t lead = lane_byte(r, pv);
    const uint8_t w = r ? gf.exp[gf.log[r] + 255 - gf.log[lead]] : 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t g = (uint8_t)uni(s.v[i][pv]);
        if (g)
            s.v[i][lane] ^= loc_mul(gf, g, w);
    }
    s.v[n][lane] = w;
    s.piv[n] = pv;
    s.n = n + 1;
    // what a lane wrote is read by the other lanes of the wave from here on
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Wave 0 of a workgroup, after the barrier behind the last append: the bases
// sb[1 .. nw) merged into its own, s = sb[0] (ovf is sticky), and s written to
// `slot` of a candidate area.
__device__ __forceinline__ void span_merge(SpanBasis& s, const SpanBasis* sb, int nw, const GfTables& gf, int lane,
                                           int cap)
{
    for (int w = 1; w < nw; ++w) {
        const int n = uni(sb[w].n);
        if (uni(sb[w].ovf))
            s.ovf = 1;
        for (int i = 0; i < n; ++i)
            span_append(s, gf, lane, span_reduce(s, gf, lane, sb[w].v[i][lane]), cap);
    }
}

__device__ __forceinline__ void span_publish(SpanBasis& s, const SpanBasis* sb, int nw, const GfTables& gf, int lane,
                                             int cap, uint8_t* slot)
{
    span_merge(s, sb, nw, gf, lane, cap);
    const int n = uni(s.n);
    if (lane == 0) {
        SlotHdr* hdr = reinterpret_cast<SlotHdr*>(slot);
        hdr->n = n;
        hdr->ovf = s.ovf;
    }
    for (int i = 0; i < n; ++i)
        slot[sizeof(SlotHdr) + i * 64 + lane] = s.v[i][lane];
}

// load_gf and span_publish for the generated kernels (rs_jit.hip k_rs_jit_locate,
// k_rs_jitw_locate), whose compiler-allocated registers must end below the
// accumulators: the same copies and the same slot, every loop rolled.  The
// compiler unrolls the loops above eight and thirteen times with a 64-bit
// address per iteration, which took k_rs_jitw_locate's allocation past v39.
// Both tables are 4-byte aligned (the device copy alignas(16), the LDS copy
// where the kernel puts it).
__device__ __forceinline__ void load_gf_rolled(GfTables& gf, const GfTables& from, int t, int threads)
{
    static_assert(sizeof(GfTables) % 4 == 0, "copied as dwords");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&from);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&gf);
#pragma unroll 1
    for (int i = t; i < (int)(sizeof(GfTables) / 4); i += threads)
        dst[i] = src[i];
}

__device__ __forceinline__ void span_publish_rolled(SpanBasis& s, const SpanBasis* sb, int nw, const GfTables& gf,
                                                    int lane, int cap, uint8_t* slot)
{
    span_merge(s, sb, nw, gf, lane, cap);
    const int n = uni(s.n);
    if (lane == 0) {
        SlotHdr* hdr = reinterpret_cast<SlotHdr*>(slot);
        hdr->n = n;
        hdr->ovf = s.ovf;
    }
#pragma unroll 1
    for (int i = 0; i < n; ++i)
        slot[sizeof(SlotHdr) + i * 64 + lane] = s.v[i][lane];
}

}  // namespace rsgpu
